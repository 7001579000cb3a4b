"""csrc/pcb_gumbel.h -- the Gumbel root rule as plain C++ -- against its specification in pcbenv/search.py, on the CPU:
tools/gumbel_check.cpp (AddressSanitizer + UBSan, a program of its own, nothing preloaded) runs the cases of
tests/gumbel_cases.py and returns the state after every call.  Level 0 of every SELECT and every CHOOSE must be
gumbel_select_root's and gumbel_choose's bit for bit; the levels below are redone in Python floats; ABSORB is held to
puct_search's through whole searches, gumbel_search recorded and replayed.  Then the table, the independence of a root from
its batch, the distribution of the first choice, Sequential Halving's budget and the policy target."""
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gumbel_cases as gc
import puct_cases as pc
from pcbenv.search import (Evaluation, considered_visits, gumbel_choose, gumbel_scores, gumbel_select_root, puct_reroot, search_tree)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _rule(c, q):
    return (c.C, c.rule[1], c.rule[2], q["seed"], q["step_index"], q["first_root"])


def _below_the_root(c, st, p, node, d):
    """csrc/pcb_puct.h's levels from (node, d) on in Python floats -> (selected, path_len)."""
    while d < gc.T and not st["terminal"][p, node] and st["num_children"][p, node] != 0:
        fc, sc = pc._scores(st, p, node, c.rule[0])
        node, d = fc + sc.index(max(sc)), d + 1
        assert (st["paths"][d - 1, p] == st["node_action"][p, node]).all()
    return node, d


def check_call(c, q, was, st, roots=None, damaged=()):
    """One call of the model against the specification: `was` the state before it, `st` after it."""
    tree, table = gc.tree_of(st), _t(c.table)
    bit = 0
    if q["phases"] & gc.SELECT:
        begun = q["phases"] & gc.BEGIN
        t0, v0 = (np.zeros_like(was["sim_index"]), np.zeros_like(was["sim_visits"])) if begun else (was["sim_index"], was["sim_visits"])
        sel = gumbel_select_root(tree, _t(t0), _t(v0), table, *_rule(c, q))
        assert np.array_equal(sel["sim_index"].numpy(), st["sim_index"]) and np.array_equal(sel["sim_visits"].numpy(), st["sim_visits"])
        assert sel["sim_index"].dtype == torch.int32 and sel["sim_visits"].dtype == torch.int32
        bit |= int(sel["errors"])
        for p in (range(c.P) if roots is None else roots):
            k, fc = int(st["num_children"][p, 0]), int(st["first_child"][p, 0])
            if p in damaged and bit:
                assert st["selected"][p] == 0 and st["path_len"][p] == 0
                continue
            if bool(sel["scheduled"][p]):
                node = fc + int(sel["child"][p])
                assert (st["paths"][0, p] == st["node_action"][p, node]).all()
                want = _below_the_root(c, st, p, node, 1)
            else:
                want = _below_the_root(c, st, p, 0, 0)
            assert want == (st["selected"][p], st["path_len"][p]), (p, want)
            assert (st["paths"][want[1]:, p] == was["paths"][want[1]:, p]).all()  # the rows not taken are untouched
        for f in gc.TREE_FIELDS:  # SELECT never stores to the tree (ABSORB may have: then the specification of whole searches speaks)
            if not q["phases"] & gc.ABSORB:
                assert pc.same_bits(st[f], was[f].astype(st[f].dtype)), f
    if q["phases"] & gc.CHOOSE:
        ch = gumbel_choose(tree, _t(st["sim_visits"]), *_rule(c, q))
        bit |= int(ch["errors"])
        for f in gc.OUT_FIELDS:
            got, want = st[f], ch[f].numpy()
            assert pc.same_bits(got, want if f in ("child_policy", "root_value") else want.astype(np.int64)), f
        for f in gc.STATE_FIELDS:
            assert pc.same_bits(st[f], was[f].astype(st[f].dtype)), f
    else:
        for f in gc.OUT_FIELDS:
            assert pc.same_bits(st[f], was[f]) if f in was else (st[f] == gc.FILL).all(), f
    if not q["phases"] & gc.ABSORB:
        assert st["errors"] == bit
    else:
        assert st["errors"] & gc.ERR_TREE == bit or damaged
    return bit


def test_the_cases_are_what_they_are_there_for():
    gc.check_cases()


@pytest.mark.parametrize("name", list(gc.CASES))
def test_the_model_is_the_specification_call_by_call(name):
    c = gc.case(name)
    before = {f: np.array(v) for f, v in c.states[-2].items() if f != "errors"}
    for i, (q, st) in enumerate(zip(c.seq, c.states)):
        was = dict(gc.before(c, i))
        assert check_call(c, q, was, st) == 0
    for f, v in before.items():  # the specification does not modify what it is given
        assert pc.same_bits(c.states[-2][f], v), f
    # what the kinds mean, on the result
    last = c.states[-1]
    for p, kind in enumerate(c.kinds):
        k = int(last["num_children"][p, 0])
        if kind == "term":
            assert k == 0 and last["move_slot"][p] == -1 and (last["sim_visits"][p] == 0).all() and last["sim_index"][p] == 0
        if k:
            fc = int(last["first_child"][p, 0])
            assert fc <= last["move_slot"][p] < fc + k and (last["move_action"][p] == last["node_action"][p, last["move_slot"][p]]).all()
            assert (last["child_weights"][p, k:] == 0).all() and (last["child_policy"][p, k:] == 0).all() and (last["child_actions"][p, k:] == 0).all()
            pol = last["child_policy"][p, :k].astype(np.float64)
            assert (pol >= 0).all() and abs(pol.sum() - 1.0) <= k * 2.0 ** -24
            assert abs(int(last["child_weights"][p, :k].sum()) - 2 ** 24) <= k / 2 + 1
            if c.rule[2] == 0.0:  # c_scale = 0: the float32 prior renormalised over the k children, to a float32 unit in the last place
                pr = np.clip(last["prior"][p, fc:fc + k], 2.0 ** -149, 1.0)
                assert np.abs(pol - pr / pr.sum()).max() <= 2.0 ** -24
        else:
            assert last["move_slot"][p] == -1 and not last["child_weights"][p].any() and not last["child_policy"][p].any()


@pytest.mark.parametrize("name", list(gc.DAMAGE))
def test_a_damaged_root_stops_where_the_contract_says(name):
    c, at, seq, states, p = gc.damaged(name)
    q, st, healthy = seq[-1], states[-1], c.states[at]
    was = {f: np.array(v) for f, v in gc.before(c, at).items() if f != "errors"}
    tensor, flat_index, value = q["pokes"][0]
    was[tensor].reshape(-1)[flat_index] = value
    counters = name.startswith(("sim_visits", "choose_sim_visits"))  # a counter is only ever compared: data, not damage
    if name.startswith("absorb_"):
        assert st["errors"] & gc.ERR_TREE and not healthy["errors"] & gc.ERR_TREE
        for f in gc.TREE_FIELDS:  # ABSORB stopped before its first store
            assert pc.same_bits(st[f][p], was[f][p].astype(st[f].dtype)), f
    else:
        bit = check_call(c, q, was, st, damaged=() if counters else (p,))
        assert bit == (0 if counters else gc.ERR_TREE)
    if name.startswith("sim_index"):
        assert st["sim_index"][p] == value and (st["sim_visits"][p] == was["sim_visits"][p]).all() and (st["paths"][:, p] == was["paths"][:, p]).all()
    if name.startswith("choose_") and not counters:
        assert st["move_slot"][p] == -1 and not st["move_action"][p].any() and not st["child_weights"][p].any() and not st["child_policy"][p].any() \
            and not st["child_actions"][p].any()
    others = [r for r in range(c.P) if r != p]
    for f in gc.STATE_FIELDS + gc.OUT_FIELDS:  # the neighbours are the healthy run's
        rows = (lambda a: a[:, others]) if f == "paths" else (lambda a: a[others])
        assert pc.same_bits(rows(st[f]), rows(healthy[f])), f


# ---- whole searches ------------------------------------------------------------------------------------------------------
SEARCH = dict(P=9, levels=5, n=8, Mc=4, C=4, K=4, rule=(1.25, 50.0, 1.0), key=dict(seed=gc.SEED ^ 5, step_index=(1 << 33) + 3, first_root=4))


def _replay(gs, calls, start, s=SEARCH):
    seq = gc.search_calls(calls, s["key"])
    states = gc.run(start, s["C"], s["K"], s["n"], s["Mc"], s["rule"], seq, levels=s["levels"])
    for m, st in enumerate(states[:len(calls)]):  # every selection is the recorded one
        want_paths, want_len = calls[m][0], calls[m][1]
        assert np.array_equal(st["path_len"], want_len)
        for p in range(s["P"]):
            assert np.array_equal(st["paths"][:want_len[p], p], want_paths[:want_len[p], p])
    last = states[-1]
    pc.compare_with_search(dict(last, errors=max(st["errors"] for st in states)), gs.search)
    assert np.array_equal(last["sim_index"], gs.sim_index.numpy()) and np.array_equal(last["sim_visits"], gs.sim_visits.numpy())
    for f in gc.OUT_FIELDS:
        want = getattr(gs, f).numpy()
        assert pc.same_bits(last[f], want if f in ("child_policy", "root_value") else want.astype(np.int64)), f
    return states


def test_a_search_and_the_search_that_follows_it_in_the_kept_tree():
    s = SEARCH
    N = 1 + 2 * (s["n"] + 1) * s["C"]
    ev = pc.synthetic_evaluator(s["P"], s["levels"], s["K"], 23)
    gs, calls = gc.record_search(s["P"], s["levels"], s["n"], s["Mc"], s["C"], ev, s["rule"], s["key"], capacity=N)
    assert len(calls) == s["n"] + 1
    states = _replay(gs, calls, gc.init_state(s["P"], N, s["C"], s["levels"]))
    # a fresh root spends evaluation 0 on its own expansion and then makes exactly n scheduled simulations
    expanded = states[1]["num_children"][:, 0] > 0
    assert expanded.any() and (~expanded).any()
    live = expanded & (states[-1]["terminal"][:, 0] == 0)
    assert (states[-1]["sim_index"][live] == s["n"]).all() and (states[-1]["sim_visits"][live].sum(axis=1) == s["n"]).all()
    assert (states[-1]["sim_index"][~expanded] == 0).all()
    # the move's subtree, kept: n scheduled simulations and one PUCT descent
    tree, _ = puct_reroot(search_tree(gs.search), gs.move_slot)
    key = dict(s["key"], step_index=s["key"]["step_index"] + 1)
    s2 = dict(s, key=key)
    gs2, calls2 = gc.record_search(s["P"], s["levels"], s["n"], s["Mc"], s["C"], pc.synthetic_evaluator(s["P"], s["levels"], s["K"], 29), s["rule"], key,
                                   tree=tree)
    states2 = _replay(gs2, calls2, gc.state_of(tree, s["P"], s["C"], s["levels"]), s2)
    kept = (states2[0]["num_children"][:, 0] > 0) & (states2[0]["terminal"][:, 0] == 0)
    assert kept.any() and (states2[-1]["sim_index"][kept] == s["n"]).all()
    assert (states2[-1]["visits"][kept, 0] - states2[0]["visits"][kept, 0] == s["n"] + 1).all()


# ---- the table -----------------------------------------------------------------------------------------------------------
def test_the_table():
    hand = {(2, 4): [0, 0, 1, 1], (3, 5): [0, 0, 0, 1, 1], (4, 8): [0, 0, 0, 0, 1, 1, 2, 2], (4, 16): [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5],
            (16, 16): [0] * 16, (64, 3): [0, 0, 0], (1, 4): [0, 1, 2, 3], (0, 3): [0, 0, 0]}
    for (m, n), row in hand.items():
        assert gc.model_row(m, n) == row, (m, n)
        if m >= 1:
            assert considered_visits(m, n)[m].tolist() == row and considered_visits(m, n)[0].tolist() == [0] * n
    for n in range(1, 65):
        table = considered_visits(64, n)
        assert table.shape == (65, n) and table.dtype == torch.int32
        for m in (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33, 63, 64):
            assert gc.model_row(m, n) == table[m].tolist(), (m, n)
        for m in range(1, 65):
            row = table[m].tolist()
            assert len(row) == n and row[:min(m, n)] == [0] * min(m, n) if m > 1 else row == list(range(n))
            # non-decreasing within a phase: a drop only where a phase of fewer candidates begins, and the row as a whole rises
            assert all(b >= a for a, b in zip(row, row[1:])), (m, n)


# ---- a root's draws are its own --------------------------------------------------------------------------------------------
def test_a_slice_of_a_batch_has_the_bits_of_the_batch():
    c = gc.case("G16_C16_P67")
    i = 4  # an ABSORB | SELECT call
    whole, q = c.states[i], c.seq[i]
    for a, b in ((0, 1), (5, 23), (64, 67), (66, 67)):
        part = {f: (v[:, a:b] if f == "paths" else v[a:b]) for f, v in gc.before(c, i).items() if f in gc.STATE_FIELDS}
        ev = tuple(x[a:b] for x in q["evaluation"])
        st = gc.run(part, c.C, c.K, c.n, c.Mc, c.rule, [dict(q, evaluation=ev, first_root=c.first_root + a)])[0]
        for f in gc.STATE_FIELDS:
            assert pc.same_bits(st[f], whole[f][:, a:b] if f == "paths" else whole[f][a:b]), f
    # and of the width: the first 3 children of 16 have the g of 3 alone
    tree = gc.tree_of(c.states[2])
    wide = gumbel_scores(tree, 16, 50.0, 1.0, gc.SEED, 9, 0)["g"]
    narrow = gumbel_scores(tree, 3, 50.0, 1.0, gc.SEED, 9, 0)["g"]
    assert pc.same_bits(wide[:, :3].contiguous().numpy(), narrow.numpy())


def test_another_key_gives_other_draws():
    tree = gc.tree_of(gc.case("G8_C8_P67").states[2])
    g = lambda **kw: gumbel_scores(tree, 8, 50.0, 1.0, **{**dict(seed=gc.SEED, step_index=77, first_root=0), **kw})["g"]
    g0 = g()
    for other in (g(step_index=78), g(seed=gc.SEED ^ 1), g(first_root=1), g(step_index=77 + (1 << 32))):
        assert (other != g0).all()
    assert all(len(set(row)) == 8 for row in g0.tolist())
    assert pc.same_bits(g(first_root=1)[:-1].contiguous().numpy(), g0[1:].contiguous().numpy())  # root p + 1 of one batch is root p of the next


# ---- the distribution of the first choice ---------------------------------------------------------------------------------
def _fresh_roots(P, k, priors):
    N = k + 1
    st = gc.init_state(P, N, k, gc.T)
    st["num_children"][:, 0], st["first_child"][:, 0], st["num_nodes"][:] = k, 1, N
    st["visits"][:, 0], st["value_sum"][:, 0], st["value_max"][:, 0], st["reward_lo"][:], st["reward_hi"][:] = 1, 0.5, 0.5, 0.5, 0.5
    st["parent"][:, 1:], st["depth"][:, 1:], st["prior"][:, 1:] = 0, 1, priors
    st["node_action"][:, 1:, 2] = np.arange(k)
    return st


@pytest.mark.parametrize("k", [8, 16])
def test_the_first_choice_is_a_draw_from_the_prior(k):
    """4 096 fresh roots with a geometric prior, after BEGIN | SELECT: argmax(g + logit) is a draw from the prior (the
    Gumbel-max trick; sigma is the same for every child of a root without visits below it).  The frequency of every child
    within 5 standard errors sqrt(p (1 - p) / 4096) of its prior."""
    P = 4096
    pri = np.array([2.0 ** -(c + 1) for c in range(k - 1)] + [2.0 ** -(k - 1)])
    assert pri.sum() == 1.0
    st = gc.run(_fresh_roots(P, k, pri), k, 1, 16, 16, (1.25, 50.0, 1.0), [gc.call(gc.BEGIN | gc.SELECT, step_index=3)])[0]
    assert st["errors"] == 0 and (st["sim_index"] == 1).all() and (st["sim_visits"].sum(axis=1) == 1).all() and (st["path_len"] == 1).all()
    freq = st["sim_visits"].mean(axis=0)
    z = (freq - pri) / np.sqrt(pri * (1.0 - pri) / P)
    print(f"k {k}: largest |z| of a child's frequency {np.abs(z).max():.2f}")
    assert np.abs(z).max() < 5.0
    sel = gumbel_select_root(gc.tree_of(st), torch.zeros(P, dtype=torch.int32), torch.zeros((P, k), dtype=torch.int32), considered_visits(16, 16), k, 50.0,
                             1.0, gc.SEED, 3, 0)
    assert np.array_equal(sel["sim_visits"].numpy(), st["sim_visits"])


# ---- Sequential Halving ------------------------------------------------------------------------------------------------------
def test_sequential_halving_spends_the_budget_on_the_best():
    """m = 4 candidates, n = 16 simulations: every candidate twice, then the better two four times more -- {6, 6, 2, 2} --
    with values 0.2 apart per child, a gap of 10 in sigma against a Gumbel spread of a few units; CHOOSE takes the better
    finalist."""
    P, C, n, Mc, levels = 6, 4, 16, 4, 3
    worth = np.array([[0.3, 0.9, 0.5, 0.7], [0.9, 0.7, 0.5, 0.3], [0.5, 0.3, 0.9, 0.7], [0.7, 0.5, 0.3, 0.9], [0.3, 0.5, 0.7, 0.9], [0.9, 0.3, 0.7, 0.5]])

    def evaluate(paths, path_len, s):
        at_root = path_len == 0
        c = paths[0, :, 2].to(torch.int64)
        value = torch.where(at_root, torch.full((P,), 0.6, dtype=torch.float64), torch.from_numpy(worth)[torch.arange(P), c.clamp(0, C - 1)])
        actions = torch.zeros((P, C, 3), dtype=torch.int32)
        actions[:, :, 2] = torch.arange(C, dtype=torch.int32)
        return Evaluation(value, torch.zeros(P, dtype=torch.uint8), torch.where(at_root, C, 0).to(torch.int32), actions, torch.full((P, C), 0.25))
    rule, key = (1.25, 50.0, 1.0), dict(seed=gc.SEED, step_index=12, first_root=0)
    gs, calls = gc.record_search(P, levels, n, Mc, C, evaluate, rule, key)
    _replay(gs, calls, gc.init_state(P, 1 + (n + 1) * C, C, levels), dict(P=P, levels=levels, n=n, Mc=Mc, C=C, K=C, rule=rule, key=key))
    for p in range(P):
        sims = gs.sim_visits[p].tolist()
        order = np.argsort(-worth[p])
        assert sorted(sims) == [2, 2, 6, 6] and {int(order[0]), int(order[1])} == {c for c in range(C) if sims[c] == 6}, (p, sims)
        assert int(gs.move_action[p, 2]) == int(order[0]) and int(gs.move_slot[p]) == 1 + int(order[0])


# ---- the policy target -------------------------------------------------------------------------------------------------------
def test_a_better_value_raises_the_target():
    c = gc.case("G8_C8_P67")
    st = c.states[-2]
    tree = gc.tree_of(st)
    p = next(r for r in range(c.P) if c.kinds[r] == "kept" and st["reward_hi"][r] > st["reward_lo"][r])
    fc = int(st["first_child"][p, 0])
    b = next(s for s in range(8) if st["visits"][p, fc + s] > 0)
    args = (_t(st["sim_visits"]), 8, 50.0, 1.0, gc.SEED, 77, 11)
    base = gumbel_choose(tree, *args)["child_policy"][p]
    tree["value_sum"] = tree["value_sum"].clone()
    tree["value_sum"][p, fc + b] += 0.05
    more = gumbel_choose(tree, *args)["child_policy"][p]
    assert more[b] > base[b] and all(more[s] <= base[s] for s in range(8) if s != b)
