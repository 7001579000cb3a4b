"""Cases, recordings and the CPU model of pcbenv_puct_advance_leaves (plain module, no test; needs no GPU).

The specification is pcbenv/search.py:puct_search(leaves=L).  `record` runs it on the CPU with an evaluator that writes
down, per iteration, the `paths` and `path_len` of the P * L rows it was asked for and the evaluation it gave back;
tests/puct_cases.py:search_calls turns such a recording into the sequence of calls `puct_search_device(leaves=L)` makes,
and `replay` feeds a sequence to tools/puct_leaves_check.cpp -- csrc/pcb_puct_leaves.h compiled for the CPU with
AddressSanitizer and UBSan, a program of its own -- which checks every selection against the recorded one and returns
the state after every call.  The GPU tests compare the kernel with those states.

`leaves_evaluator` is tests/puct_cases.py:synthetic_evaluator with root = row // L: a function of (root, path), so two
leaves of one launch that reach the same node are told the same.  Rows that are no leaf (path_len -1) get NaN for a
value and a count far out of range: a search that looked at them would show it.

`launch_facts` walks the L descents of every root of a SELECT again in Python floats -- the operations of
csrc/pcb_puct_leaves.h:leaves_score one by one -- checks the model's choice on the way and counts what the reach
assertions of tests/test_puct_leaves_model.py ask for."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import model_harness as mh
from pcbenv.search import Evaluation, puct_search
from puct_cases import ABSORB, INIT, SELECT, ERR_FULL, ERR_TREE, FLOATS, POKED_CALL, REPO, TREE_FIELDS, _words, flat, same_bits, search_calls, synthetic_evaluator  # noqa: F401
from puct_cases import PRIORS, _mix

STATE_FIELDS = ("selected", "path_len", "paths") + TREE_FIELDS + ("pending",)
LOADED_CALL = 16  # next to the phases of a call in the model's input: a tree follows (`load`: a dict of TREE_FIELDS tensors)
POKED = ("selected", "num_nodes", "parent", "num_children", "first_child", "pending")  # the tensors a call's pokes may name, by number


def shapes(P, N, T, L):
    R = P * L
    s = {"selected": (R,), "path_len": (R,), "paths": (T, R, 3), "num_nodes": (P,), "node_action": (P, N, 3), "reward_lo": (P,), "reward_hi": (P,)}
    s.update({n: (P, N) for n in ("parent", "depth", "visits", "num_children", "first_child", "prior", "value_sum", "value_max", "terminal", "pending")})
    return s


def program():
    """tools/puct_leaves_check.cpp as tests/model_harness.py:tool builds it; None without g++."""
    return mh.tool("puct_leaves_check")


def per_leaf(base, P, T, K, L):
    """An evaluator of P rows, a function of (root, path), on the P * L rows of a leaf-parallel search: row p * L + l is told
    what root p is told of that path.  Rows with path_len -1 come back with NaN, terminal, a count of K + 1000 and candidates of -9."""
    def evaluate(paths, path_len, step_index0):
        assert tuple(paths.shape) == (T, P * L, 3) and tuple(path_len.shape) == (P * L,) and path_len.dtype == torch.int32
        parts = [base(paths[:, l::L].contiguous(), path_len[l::L].clamp(min=0), step_index0) for l in range(L)]
        stack = lambda f: torch.stack([getattr(e, f) for e in parts], dim=1).reshape((P * L,) + tuple(getattr(parts[0], f).shape[1:])).clone()
        ev = Evaluation(stack("value").to(torch.float64), stack("terminal").to(torch.uint8), stack("cand_count"), stack("cand_actions"), stack("cand_prior"))
        none = path_len < 0
        ev.value[none], ev.terminal[none], ev.cand_count[none], ev.cand_actions[none], ev.cand_prior[none] = float("nan"), 1, K + 1000, -9, 0.5
        return ev
    return evaluate


_MUL, _M64 = np.uint64(0xBF58476D1CE4E5B9), 0xFFFFFFFFFFFFFFFF
_PRIORS32 = np.array(PRIORS, np.float32)


@functools.lru_cache(maxsize=None)
def _node(seed, T, K, p, path):
    """What tests/puct_cases.py:synthetic_evaluator says of the node `path` (a tuple of (o, y) pairs) of root p, the K
    candidates at once: -> (value, terminal, cand_count, cand_actions [K, 3], cand_prior [K])."""
    h = _mix(seed, p)
    for o, y in path:
        h = _mix(h, o, y)
    over = p % 7 == 6 or len(path) == T or (len(path) > 0 and (h >> 24) % 5 == 0)
    count = 0 if p % 7 == 5 else (h >> 32) % (K + 1) if (h >> 40) % 4 == 0 else K
    c = np.arange(K, dtype=np.uint64)
    h1 = _mix(h)  # _mix(h, c), the round that takes h
    h2 = (np.uint64(h1) ^ c) * _MUL
    h2 ^= h2 >> np.uint64(29)
    actions = np.stack([(h % 2 + np.arange(K)) % 2, np.zeros(K, np.int64), np.arange(K)], axis=1).astype(np.int32)
    return (0.25, 0.5, 0.75)[(h >> 16) % 3], int(over), count, actions, _PRIORS32[(h2 % np.uint64(len(PRIORS))).astype(np.int64)]


def leaves_evaluator(P, T, K, L, seed):
    """tests/puct_cases.py:synthetic_evaluator with root = row // L, as per_leaf makes it of that function -- the same
    outputs, bit for bit (tests/test_puct_leaves_model.py holds the two together) -- computed node by node, the candidates
    of a node at once and a node once: a search of 64 leaves asks for some ten thousand rows per launch."""
    def evaluate(paths, path_len, step_index0):
        assert tuple(paths.shape) == (T, P * L, 3) and tuple(path_len.shape) == (P * L,) and path_len.dtype == torch.int32
        pa, pl = paths.numpy(), path_len.numpy()
        R = P * L
        value, over, count = np.full(R, np.nan), np.ones(R, np.uint8), np.full(R, K + 1000, np.int32)
        actions, prior = np.full((R, K, 3), -9, np.int32), np.full((R, K), 0.5, np.float32)
        for r in np.flatnonzero(pl >= 0):
            value[r], over[r], count[r], actions[r], prior[r] = _node(seed, T, K, int(r) // L, tuple((int(a[0]), int(a[2])) for a in pa[:pl[r], r]))
        return Evaluation(torch.from_numpy(value), torch.from_numpy(over), torch.from_numpy(count), torch.from_numpy(actions), torch.from_numpy(prior))
    return evaluate


def record(P, T, L, iterations, c_puct, max_children, evaluate, step_index=0, capacity=None, tree=None):
    """puct_search(leaves=L) on the CPU -> (its result, [(paths [T, P * L, 3], path_len [P * L], value, leaf_terminal, cand_count,
    cand_actions, cand_prior)]), as tests/puct_cases.py:record."""
    calls = []

    def recording(paths, path_len, s):
        ev = evaluate(paths, path_len, s)
        calls.append((paths.clone().numpy(), path_len.clone().numpy(), ev.value.to(torch.float64).numpy().copy(),
                      ev.terminal.to(torch.uint8).numpy().copy(), ev.cand_count.to(torch.int32).numpy().copy(),
                      ev.cand_actions.to(torch.int32).numpy().copy(), ev.cand_prior.to(torch.float32).numpy().copy()))
        return ev
    root = SimpleNamespace(num_envs=P, device="cpu", cfg=None)
    ps = puct_search(root, iterations, step_index, recording, c_puct=c_puct, max_children=max_children, max_steps=T, capacity=capacity, tree=tree,
                     leaves=L)
    return ps, calls


def replay(P, N, C, T, K, L, c_puct, seq, via=0):
    """-> [state after call i]: dicts of STATE_FIELDS (int64; FLOATS as float64) and `errors`, as tests/puct_cases.py:replay.
    via=1 (L == 1 only): the same calls through csrc/pcb_puct.h.  A call may carry `load`, a tree that replaces the state's
    before its phases run."""
    R = P * L
    parts = [np.array([P, N, C, T, K, L, via, len(seq), mh.bits(c_puct)], np.int64)]
    for c in seq:
        pokes = c.get("pokes", ())
        load = c.get("load")
        parts.append(np.array([c["phases"] | (POKED_CALL if pokes else 0) | (LOADED_CALL if load is not None else 0), int(c["expect"] is not None)], np.int64))
        if load is not None:
            parts += [_words(load[f].numpy(), f in FLOATS) for f in TREE_FIELDS]
        if pokes:
            parts.append(np.array([len(pokes)] + [w for name, at, value in pokes for w in (POKED.index(name), at, value)], np.int64))
        if c["phases"] & ABSORB:
            value, over, count, actions, prior = c["evaluation"]
            assert actions.shape == (R, K, 3) and prior.shape == (R, K) and prior.dtype == np.float32
            parts += [_words(value, True), _words(over), _words(count), _words(actions), mh.float32_words(prior)]
        if c["expect"] is not None:
            parts += [_words(c["expect"][1]), _words(c["expect"][0])]
    return mh.cut(mh.run_words(program(), parts), len(seq), STATE_FIELDS, shapes(P, N, T, L), FLOATS)


def compare_with_search(state, ps):
    """The model's final state against puct_search's result, field by field, floats by their bits; nothing is pending."""
    for f in TREE_FIELDS:
        t = getattr(ps, f).numpy()
        if f in FLOATS:
            assert same_bits(state[f], t), f
        else:
            assert np.array_equal(state[f], t.astype(np.int64)), f
    assert state["errors"] == int(ps.errors)
    assert not state["pending"].any()


@functools.lru_cache(maxsize=None)
def synthetic(P, T, C, K, L, iterations, c_puct=1.25, seed=11, capacity=None, split=False):
    """-> SimpleNamespace(P, N, C, T, K, L, c_puct, ps, calls, seq, states): a recorded search with the synthetic evaluator and its replay."""
    ps, calls = record(P, T, L, iterations, c_puct, C, leaves_evaluator(P, T, K, L, seed), step_index=100, capacity=capacity)
    N = 1 + iterations * L * C if capacity is None else capacity
    seq = search_calls(calls, split)
    return SimpleNamespace(P=P, N=N, C=C, T=T, K=K, L=L, c_puct=c_puct, ps=ps, calls=calls, seq=seq, states=replay(P, N, C, T, K, L, c_puct, seq))


def repeat_share(case):
    """The share of leaf rows of the recorded launches that are no leaf."""
    lens = np.concatenate([c[1] for c in case.calls])
    return float((lens < 0).mean())


# ---- the launches again, in Python floats ---------------------------------------------------------------------------
def _score(st, p, node, ch, pending, c_puct, virtual=True):
    """csrc/pcb_puct_leaves.h:leaves_score of child ch of node; virtual=False: with nothing pending (csrc/pcb_puct.h:puct_score)."""
    lo, hi = float(st["reward_lo"][p]), float(st["reward_hi"][p])
    v_c, v_n = int(st["visits"][p, ch]), int(st["visits"][p, node])
    n_c = float(v_c + (pending[ch] if virtual else 0))
    q = ((float(st["value_sum"][p, ch]) / float(v_c) - lo) / (hi - lo)) * (float(v_c) / n_c) if v_c > 0 and hi > lo else 0.0
    n_p = v_n + (pending[node] if virtual else 0)
    return q + c_puct * float(st["prior"][p, ch]) * math.sqrt(float(max(n_p, 1))) / (1.0 + n_c)


def launch_facts(st, L, c_puct, T):
    """`st`: a healthy state dumped after a call with SELECT that found nothing pending.  Redoes the L descents of every root
    and checks selected / path_len / pending against them.  -> counts: all_real (roots all of whose L leaves are leaves),
    repeat_behind (roots with a repeat at l >= 1), bare_root (roots all of whose leaves select slot 0), terminal_twice
    (roots with a terminal node below the root selected by two leaves), parted (levels at which a descent chose another
    child than it would have with nothing pending), ties (levels at which the best score occurs twice)."""
    P = st["num_nodes"].shape[0]
    facts = dict(all_real=0, repeat_behind=0, bare_root=0, terminal_twice=0, parted=0, ties=0)
    for p in range(P):
        pending, chosen = {}, []
        for l in range(L):
            row = p * L + l
            node, d, passed = 0, 0, [0]
            while d < T and not st["terminal"][p, node] and st["num_children"][p, node] != 0:
                fc, k = int(st["first_child"][p, node]), int(st["num_children"][p, node])
                pend = {s: pending.get(s, 0) for s in [node] + list(range(fc, fc + k))}
                sc = [_score(st, p, node, fc + c, pend, c_puct) for c in range(k)]
                plain = [_score(st, p, node, fc + c, pend, c_puct, virtual=False) for c in range(k)]
                facts["ties"] += sc.count(max(sc)) > 1
                facts["parted"] += sc.index(max(sc)) != plain.index(max(plain))
                node, d = fc + sc.index(max(sc)), d + 1
                passed.append(node)
            if not st["terminal"][p, node] and st["num_children"][p, node] == 0 and pending.get(node, 0) > 0:
                assert (st["selected"][p * L + l:(p + 1) * L] == -1).all() and (st["path_len"][p * L + l:(p + 1) * L] == -1).all(), (p, l)
                facts["repeat_behind"] += l >= 1
                break
            assert node == st["selected"][row] and d == st["path_len"][row], (p, l, node, d)
            for s in passed:
                pending[s] = pending.get(s, 0) + 1
            chosen.append(node)
        want = np.zeros(st["pending"].shape[1], np.int64)
        for s, n in pending.items():
            want[s] = n
        assert np.array_equal(st["pending"][p], want), p
        facts["all_real"] += len(chosen) == L and L > 1
        facts["bare_root"] += len(chosen) == L and L > 1 and all(s == 0 for s in chosen)
        facts["terminal_twice"] += any(s != 0 and st["terminal"][p, s] and chosen.count(s) > 1 for s in chosen)
    return facts


def case_facts(case):
    """launch_facts summed over the calls of a healthy case that select."""
    total = {}
    for st, c in zip(case.states, case.seq):
        if c["phases"] & SELECT:
            for k, v in launch_facts(st, case.L, case.c_puct, case.T).items():
                total[k] = total.get(k, 0) + int(v)
    return total


# ---- the cases of the CPU model test --------------------------------------------------------------------------------
# (P, T, C, K, L, iterations): L in {1, 2, 3, 8} x C in {1, 3, 5}, K below, at and above C.  Root p % 7 == 5 never has a
# candidate and root p % 7 == 6 is terminal; a chain (C = 1) selects one leaf per launch until its end is terminal, so
# the iterations are many enough for the repeats to stay below half of all rows.
MODEL_CASES = [(14, 5, C, K, L, 14) for L in (1, 2, 3, 8) for C, K in ((1, 1), (1, 2), (3, 2), (3, 3), (5, 5), (5, 7))]

# ---- the cases of the GPU test: every group width x leaves, three blocks at G = 4 -------------------------------------
GPU_P, GPU_T = 130, 5
# (C, K, L, iterations); the capacity is 1 + 40 * C, which the searches with many leaves fill: ERR_FULL is part of them.  A chain
# (C = 1) has one leaf per launch until its end is terminal, after T + 1 launches at the latest: 14 launches keep its repeats
# below half.  With 64 leaves the first launch of a tree is one leaf and 63 rows that are none, and the second finds the
# root's children only: 64 leaves go with C = 64, and six launches bring the share below half (the launches behind the
# second have a quarter of their rows none).  C = 32 (K = 20) is there for the one group width the other values of C skip.
GPU_CASES = {
    "C1_L8": (1, 1, 8, 14), "C4_L1": (4, 4, 1, 8), "C5_L3": (5, 4, 3, 8), "C16_L2": (16, 16, 2, 6), "C16_L8": (16, 12, 8, 5),
    "C32_L2": (32, 20, 2, 5), "C33_L8": (33, 33, 8, 4), "C64_L2": (64, 64, 2, 5), "C64_L64": (64, 64, 64, 6),
}


def gpu_case(name, split=False):
    C, K, L, iterations = GPU_CASES[name]
    return synthetic(GPU_P, GPU_T, C, K, L, iterations, capacity=1 + 40 * C, split=split)


# ---- trees the caller has damaged -----------------------------------------------------------------------------------
DAMAGE_GAMES = {4: (9, 5, 3, 3, 4, 8, (1, 2, 3)), 16: (7, 5, 9, 9, 3, 8, (1, 2, 3)), 64: (4, 5, 33, 33, 2, 8, (2,))}  # G: P, T, C, K, L, iterations, roots
DAMAGE = ("selected_N", "selected_minus_2", "num_nodes_0", "num_nodes_N_plus_1", "first_child_0", "first_child_N", "first_child_plus_k_over_N",
          "num_children_minus_1", "num_children_C_plus_5", "parent_N", "parent_self", "pending_garbage")
DAMAGE_CASES = [(G, n) for G in DAMAGE_GAMES for n in DAMAGE]
GARBAGE = (2 ** 31 - 1, -2 ** 31, 12345, -1000000, 2 ** 30, 7)  # pending is data: any of these only changes which child wins


@functools.lru_cache(maxsize=None)
def damaged(G, name):
    """-> SimpleNamespace(P, N, C, T, K, L, c_puct, seq, states, base, k, p, node, name): a healthy prefix seq[:k] of the search of
    width G, after which root p is expanded and leaf 0 of root p is a node below the root that the evaluation of call k does
    not call terminal; call k (ABSORB | SELECT) with the pokes; then two more ABSORB | SELECT calls with the evaluations the
    healthy search got -- data by then, for the damaged root.  `base` is the healthy search: its states are those of the
    roots nothing was done to."""
    P, T, C, K, L, iterations, roots = DAMAGE_GAMES[G]
    base = synthetic(P, T, C, K, L, iterations)
    N, shp = base.N, shapes(P, base.N, T, L)
    p = roots[DAMAGE.index(name) % len(roots)]
    for k in range(1, len(base.seq) - 3):
        st = base.states[k - 1]
        node = int(st["selected"][p * L])
        if node > 0 and not st["terminal"][p, node] and st["num_nodes"][p] + C * L <= N and \
                all(base.seq[i]["phases"] == ABSORB | SELECT for i in range(k, k + 3)) and not base.seq[k]["evaluation"][1][p * L]:
            break
    else:
        raise AssertionError(f"no call of the healthy search after which root {p} suits {name}")
    assert st["errors"] == 0 and st["num_children"][p, 0] >= 1
    nch = int(st["num_children"][p, 0])
    pokes = []
    poke = lambda f, value, *index: pokes.append((f, flat(shp[f], *index), int(value)))
    if name.startswith("selected_"):
        poke("selected", N if name == "selected_N" else -2, p * L + (1 if st["selected"][p * L + 1] >= 0 else 0))
    elif name.startswith("num_nodes_"):
        poke("num_nodes", 0 if name == "num_nodes_0" else N + 1, p)
    elif name.startswith("first_child_"):
        poke("first_child", {"first_child_0": 0, "first_child_N": N, "first_child_plus_k_over_N": N - nch + 1}[name], p, 0)
    elif name.startswith("num_children_"):
        poke("num_children", -1 if name == "num_children_minus_1" else C + 5, p, 0)
    elif name.startswith("parent_"):
        poke("parent", N if name == "parent_N" else node, p, node)
    else:
        for s in range(N):
            poke("pending", GARBAGE[s % len(GARBAGE)], p, s)
    def finite(evaluation):  # a row that was no leaf of the healthy search may be one now: its value is a number then
        value = np.array(evaluation[0], copy=True)
        value[p * L:(p + 1) * L] = np.where(np.isnan(value[p * L:(p + 1) * L]), 0.5, value[p * L:(p + 1) * L])
        return (value,) + tuple(evaluation[1:])
    seq = base.seq[:k] + [dict(phases=ABSORB | SELECT, evaluation=finite(base.seq[k]["evaluation"]), expect=None, pokes=pokes)] + \
        [dict(phases=ABSORB | SELECT, evaluation=finite(base.seq[i]["evaluation"]), expect=None) for i in (k + 1, k + 2)]
    return SimpleNamespace(P=P, N=N, C=C, T=T, K=K, L=L, c_puct=base.c_puct, seq=seq, states=replay(P, N, C, T, K, L, base.c_puct, seq), base=base,
                           k=k, p=p, node=node, name=name)
