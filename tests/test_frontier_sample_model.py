"""csrc/pcb_frontier_sample.h -- the frontier step of pcbenv_frontier_sample as plain C++ -- against its specification,
pcbenv/search.py:frontier_sample_advance, on the CPU: tools/frontier_sample_check.cpp (AddressSanitizer + UBSan, a program
of its own, nothing preloaded) replays the call sequences of tests/frontier_sample_cases.py, and the specification runs the
same sequences from the same sentinel-filled tensors.  The two agree after every call on every tensor, floats by their
bits.  Then what the rule promises: the truncated Gumbel on a table of its arms, the exact maximum on every recorded call,
every leaf of a small tree exactly once, independence of the batch, and the distribution of the sample.

The reach assertions say what the table of cases contains, so that tests/test_frontier_sample_gpu.py, which holds the
kernel to the model on it, cannot be vacuous."""
import itertools
import math
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import frontier_sample_cases as sc
from pcbenv import search

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.mark.parametrize("name", list(sc.CASES))
def test_the_model_is_the_specification_after_every_call(name):
    c = sc.case(name)
    spec = sc.specify(c.P, c.W, c.K, c.T, c.seed, c.first_root, c.seq)
    assert len(spec) == len(c.states) == len(c.seq)
    for i, (a, b) in enumerate(zip(c.states, spec)):
        for f in sc.STATE_FIELDS:
            assert sc.same_bits(a[f], b[f]), (name, i, f)
        assert a["errors"] == b["errors"], (name, i)


def test_the_table_reaches_every_arm_of_the_rule():
    sc.assert_reach(list(sc.CASES))
    searched = sc.reach([n for n in sc.CASES if sc.CASES[n][4] != "hand"])  # the searches alone
    for arm in ("more_than_W", "fewer_than_W", "no_contender", "entry_survives", "entry_dropped", "finished_enters", "finished_cut", "expandable_cut",
                "enters_behind_a_survivor", "parent", "some_prior_bad", "cum_logp_not_finite"):
        assert searched.get(arm), arm
    hand = sc.reach(["hand"])
    assert not [a for a in sc.ARMS if a not in ("no_contender",) and not hand.get(a)]
    shapes = {(sc.CASES[n][1], sc.CASES[n][2]) for n in sc.CASES}
    assert {(1, 1), (3, 5), (4, 16), (64, 16), (16, 64), (1, 64)} <= shapes and {sc.CASES[n][3] for n in sc.CASES} >= {1, 5} and 5 in {sc.CASES[n][0] for n in sc.CASES}
    for n in ("W16_K64", "W64_K16"):  # the widest cases do fill up
        c = sc.case(n)
        assert sc.facts(c).get("more_than_W") and max(int(s["live"].max()) for s in c.states) == 1024 and (c.states[-1]["set_len"] >= 0).all()


def test_init_writes_the_out_set_the_set_lengths_and_nothing_else():
    c = sc.case("W3_K5")
    st = c.states[0]
    F = c.W * c.K
    want = np.full((c.P, F), -1)
    want[:, 0] = 0
    assert np.array_equal(st["path_len_0"].reshape(c.P, F), want) and (st["parent_row"] == -1).all() and (st["live"] == 1).all()
    for f in ("cum_logp_0", "gumbel_0"):
        x = st[f].reshape(c.P, F)
        assert (x[:, 0] == 0.0).all() and not np.signbit(x[:, 0]).any() and (x[:, 1:] == sc.FILL_F).all(), f
    assert (st["best_len"] == -1).all() and np.isneginf(st["best_value"]).all() and (st["set_len"] == -1).all()
    for f in ("paths_0", "paths_1", "path_len_1", "best_path", "set_path"):
        assert (st[f] == sc.FILL).all(), f
    for f in ("cum_logp_1", "gumbel_1", "set_gumbel", "set_logp", "set_value"):
        assert (st[f] == sc.FILL_F).all(), f


def test_what_the_hand_made_calls_come_to():
    """The outcomes the header promises, on the model's dump under the sanitizers (call i of hand_made is state i)."""
    c = sc.case("hand")
    W, K, T = c.W, c.K, c.T
    F = W * K
    rows = lambda st, f: st[f][F:2 * F]
    slots = lambda st, f: st[f][W:2 * W]
    inf = math.inf
    # 1: slot 0 survives untouched, slot 1 is freed and keeps everything but its length; both rows are kept
    st = c.states[1]
    assert slots(st, "set_len").tolist() == [2, -1, -1] and slots(st, "set_gumbel").tolist() == [-0.5, -5.0, sc.FILL_F]
    assert rows(st, "parent_row").tolist() == [0, 0, 3, -1, -1, -1] and st["live"][1] == 3
    # 2: row 4 (-0.2) into slot 0, row 2 (-0.3) into slot 2, behind the survivor in slot 1
    st = c.states[2]
    assert slots(st, "set_len").tolist() == [2, 1, 3] and slots(st, "set_gumbel").tolist() == [-0.2, -0.1, -0.3]
    assert slots(st, "set_logp").tolist() == [-2.5, -3.0, -1.25] and slots(st, "set_value").tolist() == [0.5, 0.125, 0.75]
    assert st["set_path"][:, W + 0].tolist() == [[0, 0, F + 4], [0, 1, F + 4], [sc.FILL] * 3, [sc.FILL] * 3]
    assert st["set_path"][:3, W + 2].tolist() == [[0, d, F + 2] for d in range(3)] and st["live"][1] == 0
    # 3: the entry, then rows 1 and 3; row 5 at the same key is cut.  Row 3 is finished and takes the lowest free slot
    st = c.states[3]
    assert slots(st, "set_len").tolist() == [1, -1, 2] and rows(st, "parent_row").tolist() == [1, 1, -1, -1, -1, -1]
    # 4: zeros of either sign are one key: the entry, rows 0 and 1
    st = c.states[4]
    assert slots(st, "set_len").tolist() == [-1, 2, -1] and rows(st, "parent_row").tolist() == [0, 0, 1, 1, -1, -1]
    # 5: +inf, 0.5, then NaN (row 0) before -inf (row 1); the children of +inf are +inf, those of NaN -inf
    st = c.states[5]
    assert rows(st, "parent_row").tolist() == [2, 2, 3, 3, 0, 0] and rows(st, "gumbel_1")[[0, 1, 4, 5]].tolist() == [inf, inf, -inf, -inf]
    assert max(rows(st, "gumbel_1")[2:4]) == 0.5
    # 6: a NaN entry, then -inf, NaN, NaN in the order of their ids: the entry, row 0, row 1; the finished row 4 is cut
    st = c.states[6]
    assert slots(st, "set_len").tolist() == [2, -1, -1] and rows(st, "parent_row").tolist() == [0, 0, 1, -1, -1, -1]
    # 7: no prior with a logarithm: every child at -inf; one good prior: that child has the parent's key
    st = c.states[7]
    assert rows(st, "gumbel_1")[:4].tolist() == [-inf, -inf, -inf, -1.5] and np.isneginf(rows(st, "cum_logp_1")[:3]).all()
    # 8: cum_logp -inf, NaN, +inf: children at -inf
    st = c.states[8]
    assert np.isneginf(rows(st, "gumbel_1")).all() and st["live"][1] == 6
    # 9: bit 2; the damaged slots are no entries, and the finished row takes slot 0; slot 2 keeps its damage
    st = c.states[9]
    assert st["errors"] == sc.ERR_SET and not c.states[8]["errors"] and slots(st, "set_len").tolist() == [2, -1, -2]
    # 10: bit 1
    st = c.states[10]
    assert st["errors"] == sc.ERR_SET | sc.ERR_ROW and rows(st, "parent_row").tolist() == [2, 2, -1, -1, -1, -1]
    # 11: five finished rows and an entry for three slots: rows 4, 1, 2 by key; the best by value is row 0, which is cut
    st = c.states[11]
    assert slots(st, "set_gumbel").tolist() == [-0.5, -1.0, -2.0] and slots(st, "set_len").tolist() == [1, 2, 3]
    assert math.isnan(slots(st, "set_value")[0]) and st["best_value"][1] == 0.99 and st["best_len"][1] == 2
    # 12: rows at T or without candidates are dropped whatever their key
    assert rows(c.states[12], "parent_row").tolist() == [2, 2, -1, -1, -1, -1]
    # the neighbours: one ordinary row and one entry each, in every call
    for st in c.states[1:]:
        assert st["live"][0] == 2 and st["live"][2] == K and st["set_len"][1] == 2 and st["set_len"][2 * W + 2] == 3


# ---- the truncated Gumbel ---------------------------------------------------------------------------------------------
def test_the_truncated_gumbel_on_a_table_of_its_arms():
    """(G_S, phi_c, G_c, Z) -> child_gumbel, model against specification bit for bit, and the arms one by one."""
    inf, nan = math.inf, math.nan
    Z = 1.25
    below = math.nextafter(Z, -inf)
    table = [
        (-3.0, -1.0, Z, Z),            # a == 0: the largest child has the parent's G
        (-3.0, -1.0, below, Z),        # one ulp below Z: exp(a) rounds to 1, d <= 0
        (-3.0, -1.0, 0.25, Z),         # v < 0
        (5.0, -1.0, 0.25, Z),          # v > 0
        (900.0, -1.0, -10.0, Z),       # v > 708: exp(-|v|) is 0
        (-900.0, -1.0, 1.0, Z),        # v < -708
        (0.0, -1.0, -800.0, Z),        # a < -708: exp(a) is 0, d is 1
        (1e308, -1.0, -1e308, Z),      # G_S - G_c overflows: -inf
        (-1e308, -1.0, -1e308, 1e308),  # a overflows to -inf
        (inf, -1.0, 0.25, Z), (-inf, -1.0, 0.25, Z), (-inf, -1.0, Z, Z),   # a parent that is not finite hands its G down
        (-3.0, -inf, -inf, Z), (-3.0, nan, nan, Z), (-3.0, inf, inf, Z), (inf, -inf, -inf, Z),  # a child without a finite phi
        (-0.0, -1.0, Z, Z), (0.0, -1.0, 0.25, Z),
    ]
    rng = np.random.default_rng(5)
    for _ in range(400):
        z = rng.normal(0, 3)
        table.append((rng.normal(0, 30), -1.0, z - rng.exponential(3.0) * rng.choice([1e-12, 1e-6, 1.0, 50.0]), z))
    t = np.array(table)
    got = sc.truncated_table(t)
    cols = [torch.from_numpy(np.ascontiguousarray(t[:, i])) for i in range(4)]
    want = search.truncated_gumbel(*cols).numpy()
    assert sc.same_bits(got, want)
    assert got[0] == -3.0 and got[1] == -3.0 and got[9] == inf and got[10] == -inf and got[11] == -inf and np.isneginf(got[12:16]).all()
    assert got[7] == -inf and got[8] == -1e308 and np.signbit(got[16]) and got[6] < 0.0
    assert not np.isnan(got).any() and (got <= t[:, 0]).all()
    # against the formula in libm: -ln(exp(-G_S) - exp(-Z) + exp(-G_c)), where that is well conditioned
    for i in (2, 3):
        G_S, _, G_c, _ = table[i]
        assert abs(got[i] - -math.log(math.exp(-G_S) - math.exp(-Z) + math.exp(-G_c))) < 1e-12


def test_the_largest_child_has_the_parents_gumbel_and_no_child_exceeds_it():
    checked = {n: sc.children_properties(sc.case(n)) for n in sc.CASES}
    assert all(checked[n] > 0 for n in sc.CASES), checked
    assert sum(checked.values()) > 400


# ---- what a search returns ----------------------------------------------------------------------------------------------
def _search(P, W, K, T, seed, evaluate, first_root=0, step_index=40):
    return search.frontier_sample_search(SimpleNamespace(num_envs=P, cfg=None, device="cpu"), evaluate, W, K, step_index, seed, first_root, max_steps=T)


def _leaves(res, P, W):
    """Per root the (path, gumbel, logp) of its entries in descending set_gumbel."""
    n, path, g, lp = res.set_len.view(P, W), res.set_path.view(-1, P, W, 3), res.set_gumbel.view(P, W), res.set_logp.view(P, W)
    out = []
    for p in range(P):
        es = [(tuple(int(path[d, p, j, 2]) for d in range(int(n[p, j]))), float(g[p, j]), float(lp[p, j])) for j in range(W) if int(n[p, j]) >= 0]
        out.append(sorted(es, key=lambda e: -e[1]))
    return out


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_a_frontier_as_wide_as_the_tree_returns_every_leaf_once(seed):
    """K = 2, T = 3, W = 8: all 8 leaves, each once, whatever the seed; their log-probabilities are those of the policy."""
    P, W, K, T = 3, 8, 2, 3
    res = _search(P, W, K, T, seed, sc.path_evaluator(K, T, 77, early=False))
    assert int(res.errors) == 0 and (res.live == 0).all() and (res.set_len == T).all()
    for es in _leaves(res, P, W):
        assert sorted(e[0] for e in es) == sorted(itertools.product(range(K), repeat=T))
        assert all(a[1] > b[1] for a, b in zip(es, es[1:])) and es[0][1] == 0.0  # the first has the root's G, exactly
    orders = {tuple(e[0] for e in es) for s in (1, 2, 3) for es in _leaves(_search(P, W, K, T, s, sc.path_evaluator(K, T, 77, early=False)), P, W)}
    assert len(orders) > 3  # and the order is a matter of the seed and the root


def test_a_root_draws_the_same_whatever_the_batch():
    """Roots 0 .. 7 in one search equal two searches of four roots with first_root 0 and 4, field by field."""
    W, K, T = 3, 4, 4
    ev = sc.path_evaluator(K, T, 31)
    whole = _search(8, W, K, T, 9, ev)
    halves = [_search(4, W, K, T, 9, ev, first_root=f) for f in (0, 4)]
    for f in ("set_len", "set_gumbel", "set_logp", "set_value", "best_value", "best_len"):
        a = getattr(whole, f).view(8, -1)
        b = torch.cat([getattr(h, f).view(4, -1) for h in halves])
        assert a.numpy().tobytes() == b.numpy().tobytes(), f
    assert torch.equal(whole.set_path.view(T, 8, W, 3), torch.cat([h.set_path.view(T, 4, W, 3) for h in halves], dim=1))
    other = _search(4, W, K, T, 9, ev, first_root=8)
    assert other.set_gumbel.numpy().tobytes() != halves[0].set_gumbel.numpy().tobytes()


# ---- the distribution ---------------------------------------------------------------------------------------------------
ROOT_PRIORS = (0.5, 0.2, 0.1)                       # unnormalised; child 1 is terminal
BELOW = {0: (0.5, 0.3, 0.2), 2: (0.7, 0.2, 0.1)}    # the priors under root children 0 and 2: they sum to 1, as the header asks below the root


def _tree_evaluator(paths, path_len, step_index0):
    paths, n = paths.numpy(), path_len.numpy()
    R = n.shape[0]
    first = paths[0, :, 2]
    prior = np.zeros((R, 3), np.float32)
    prior[:] = ROOT_PRIORS
    for a, row in BELOW.items():
        prior[(n == 1) & (first == a)] = row
    over = (n == 2) | ((n == 1) & (first == 1))
    actions = np.zeros((R, 3, 3), np.int32)
    actions[:, :, 2] = np.arange(3)
    return search.Evaluation(torch.zeros(R, dtype=torch.float64), torch.from_numpy(over.astype(np.uint8)), torch.full((R,), 3, dtype=torch.int32),
                             torch.from_numpy(actions), torch.from_numpy(prior))


def test_the_sample_has_the_distribution_of_sampling_without_replacement():
    """P = 20 000 roots of one tree, depth 2, K = 3, W = 2, unnormalised priors at the root, one leaf a depth early.  The first
    entry of a root is leaf i with probability q_i, the renormalised product of the priors on its path, and the ordered pair
    (i, j) has q_i q_j / (1 - q_i): 7 + 42 frequencies, each within 5 binomial standard deviations of its exact probability.
    (The factor of the root cancels; priors that do not sum to 1 BELOW the root do not, which the header says: with (0.3, 0.3,
    0.2) and (0.6, 0.1, 0.05) there the first entries stay exact and the pair ((0, 0), (1,)) comes at 0.0888 for 0.0765.)"""
    P, W, K, T = 20000, 2, 3, 2
    res = _search(P, W, K, T, 2019, _tree_evaluator)
    assert int(res.errors) == 0 and (res.live == 0).all() and (res.set_len >= 1).all()
    f32 = lambda xs: [float(np.float32(x)) for x in xs]
    root = f32(ROOT_PRIORS)
    q = {}
    for a, pa in enumerate(root):
        if a == 1:
            q[(a,)] = pa / sum(root)
        else:
            below = f32(BELOW[a])
            for b, pb in enumerate(below):
                q[(a, b)] = pa / sum(root) * pb / sum(below)
    assert len(q) == 7 and abs(sum(q.values()) - 1.0) < 1e-12
    n, g = res.set_len.view(P, W).numpy(), res.set_gumbel.view(P, W).numpy()
    path = res.set_path.view(T, P, W, 3).numpy()[:, :, :, 2]
    code = np.where(n == 1, path[0] * 10 + 9, path[0] * 10 + path[1])   # [P, W]: a leaf as a number
    name = lambda leaf: leaf[0] * 10 + (9 if len(leaf) == 1 else leaf[1])
    order = np.argsort(-g, axis=1)
    first, second = np.take_along_axis(code, order, 1)[:, 0], np.take_along_axis(code, order, 1)[:, 1]
    assert (first != second).all()
    worst, compared = 0.0, 0
    for i, qi in q.items():
        freq = float((first == name(i)).mean())
        z = abs(freq - qi) / math.sqrt(qi * (1.0 - qi) / P)
        worst, compared = max(worst, z), compared + 1
        assert z < 5.0, (i, freq, qi, z)
        for j, qj in q.items():
            if i == j:
                continue
            pij = qi * qj / (1.0 - qi)
            freq = float(((first == name(i)) & (second == name(j))).mean())
            z = abs(freq - pij) / math.sqrt(pij * (1.0 - pij) / P)
            worst, compared = max(worst, z), compared + 1
            assert z < 5.0, (i, j, freq, pij, z)
    assert compared == 49
    print(f"largest deviation over {compared} comparisons: {worst:.2f} standard deviations")
    # set_logp is the log-probability under the unnormalised priors
    lp = res.set_logp.view(P, W).numpy()
    k = (0, int(np.argmax(code[0] == name((0, 1))))) if (code[0] == name((0, 1))).any() else None
    if k is not None:
        assert abs(lp[k] - math.log(root[0] * f32(BELOW[0])[1])) < 1e-12
