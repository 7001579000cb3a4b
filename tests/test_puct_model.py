"""csrc/pcb_puct.h -- selection, expansion and backup of pcbenv_puct_advance as plain C++ -- against its specification,
pcbenv/search.py:puct_search, on the CPU: tools/puct_model_check.cpp (AddressSanitizer + UBSan, a program of its own,
nothing preloaded) replays recorded searches call by call, checks every selection against the recorded one and returns
its final tree, which must be puct_search's field by field, floats by their bits (tests/puct_cases.py).

And the trees a caller has damaged (puct_cases.damaged): the outcome csrc/pcb_puct.h promises for each kind of damage is
asserted here on the model's dump, under the sanitizers; tests/test_puct_advance_gpu.py then holds the kernel to the model."""
import shutil

import numpy as np
import pytest

import puct_cases as pc
from test_puct_search import CASES as TOY, EXPECT_ROOT0, T as TOY_T, evaluator_for

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

SYNTHETIC = [(7, 5, 1, 3, 40), (7, 5, 3, 3, 40), (7, 5, 5, 3, 40), (14, 5, 3, 6, 40)]  # P, T, C, K, iterations: C == 1, K == C, K < C, K > C
WIDTHS = {(P, pc.WIDTH_T, C, K, iterations): name for name, (P, C, K, iterations, *_) in pc.WIDTHS.items()}  # every group width, three blocks


@pytest.mark.parametrize("iterations, c_puct, max_children, K", TOY)
def test_the_toy_game(iterations, c_puct, max_children, K):
    P = 4
    ps, calls = pc.record(P, TOY_T, iterations, c_puct, max_children, evaluator_for(P, K))
    seq = pc.search_calls(calls)
    states = pc.replay(P, 1 + iterations * max_children, max_children, TOY_T, K, c_puct, seq)
    pc.compare_with_search(states[-1], ps)
    assert states[-1]["errors"] == 0
    if (iterations, c_puct, max_children, K) == TOY[0]:  # the tree worked out on paper
        st, e = states[-1], EXPECT_ROOT0
        n = len(e["parent"])
        assert st["num_nodes"][0] == n
        for f in ("parent", "depth", "visits", "num_children", "first_child", "prior", "value_sum", "value_max"):
            assert st[f][0, :n].tolist() == e[f], f
        assert st["node_action"][0, :n, 2].tolist() == e["b"] and st["terminal"][0, :n].astype(bool).tolist() == e["terminal"]


@pytest.mark.parametrize("P, T, C, K, iterations", SYNTHETIC + list(WIDTHS))
def test_the_synthetic_evaluator(P, T, C, K, iterations):
    row = (P, T, C, K, iterations)
    case = pc.width_case(WIDTHS[row]) if row in WIDTHS else pc.synthetic(P, T, C, K, iterations)  # width_case: with the checks that the row reaches what it is there for
    pc.compare_with_search(case.states[-1], case.ps)
    st = case.states[-1]
    assert st["errors"] == 0
    assert int(st["num_children"].max()) == min(K, C) and (st["num_children"] >= 0).all()   # K > C: truncated; K < C: never more than K
    if P > 6:
        assert st["num_nodes"][5] == 1 and st["visits"][5, 0] == iterations and not st["terminal"][5, 0]  # no candidates: evaluated again and again, never expanded
        assert st["num_nodes"][6] == 1 and st["visits"][6, 0] == iterations and st["terminal"][6, 0]      # terminal at the root
    if C > 1:  # exact ties occurred and went to the lowest child: the selections were checked against puct_search's
        assert pc.ties(case) > 0
    if row not in WIDTHS:
        counts = np.concatenate([c["evaluation"][2] for c in case.seq if c["evaluation"] is not None])
        assert set(counts.tolist()) == set(range(K + 1))  # cand_count over 0 .. K
        revisited = (st["terminal"] != 0) & (st["visits"] > 1)
        assert revisited[:, 1:].any(), "no terminal leaf was visited twice"
        assert (st["num_children"][st["terminal"] != 0] == 0).all()  # a terminal node is never expanded
        assert (st["depth"][st["terminal"] != 0] <= T).all() and (st["depth"] <= T).all()


def test_one_phase_per_call_gives_the_same_states():
    both, split = pc.synthetic(7, 5, 3, 3, 16), pc.synthetic(7, 5, 3, 3, 16, split=True)
    for f in pc.STATE_FIELDS:
        assert pc.same_bits(both.states[-1][f], split.states[-1][f]), f


def test_a_full_tree_stops_growing_all_or_nothing():
    free = pc.synthetic(7, 5, 3, 3, 40)
    full = pc.synthetic(7, 5, 3, 3, 40, capacity=6)
    pc.compare_with_search(full.states[-1], full.ps)
    a, b = free.states[-1], full.states[-1]
    grew = a["num_nodes"] > 6
    assert grew.any() and (b["num_nodes"] <= 6).all()
    assert b["errors"] & pc.ERR_FULL and not a["errors"]
    for p in range(7):  # every node in use has all the children it was given: none was made in part
        n = int(b["num_nodes"][p])
        k, fc = b["num_children"][p, :n], b["first_child"][p, :n]
        assert 1 + k.sum() == n and (b["num_children"][p, n:] == 0).all()
        assert all(fc[s] + k[s] <= n for s in range(n) if k[s]) and (b["parent"][p, n:] == -1).all()
    assert (b["visits"][:, 0] == 40).all()  # every evaluation was backed up
    refused = [i for i, s in enumerate(full.states) if s["errors"] & pc.ERR_FULL]
    assert len(refused) > 10


# ---- trees the caller has damaged ----------------------------------------------------------------------------------
def _root(state, f, p):
    return state[f][:, p] if f == "paths" else state[f][p]


def _poked(state, pokes):
    st = {f: np.array(v) for f, v in state.items() if f != "errors"}
    for f, at, value in pokes:
        st[f].reshape(-1)[at] = value
    return st


@pytest.mark.parametrize("G, name", pc.DAMAGE_CASES)
def test_a_damaged_tree_ends_as_pcb_puct_h_promises(G, name):
    """The outcome csrc/pcb_puct.h states for each kind of damage, on the model's dump (the sanitizers saw no stray
    access: replay() asserts an empty stderr): the GPU test of the same scenario then only has to equal the model."""
    sc = pc.damaged(G, name)
    k, p, N, C, T, K, node = sc.k, sc.p, sc.N, sc.C, sc.T, sc.K, sc.node
    assert 0 < p < sc.P - 1 and pc.group_lanes(C) == G and len(sc.seq) == k + 3
    assert sc.states[k - 1]["errors"] == 0 and sc.states[k - 1]["num_children"][p, 0] >= 1
    before, after = _poked(sc.states[k - 1], sc.seq[k].get("pokes", ())), sc.states[k]
    others = [q for q in range(sc.P) if q != p]
    for i in (k, k + 1, k + 2):  # the other roots advance as in the healthy run
        for f in pc.STATE_FIELDS:
            axis = 1 if f == "paths" else 0
            assert pc.same_bits(np.take(sc.states[i][f], others, axis), np.take(sc.base.states[i][f], others, axis)), (i, f)
    grew = int(after["num_nodes"][p] - before["num_nodes"][p])
    visited = {int(s): int(n) for s, n in enumerate(after["visits"][p] - before["visits"][p]) if n}
    value, _, count, _, _ = sc.seq[k]["evaluation"]
    healthy_k = pc.kept(int(sc.base.seq[k]["evaluation"][2][p]), K, C)
    chain = []
    s = node
    while s >= 0:
        chain.append(s); s = int(sc.states[k - 1]["parent"][p, s])
    if name.startswith(("selected_", "num_nodes_")):  # the ABSORB of root p does nothing at all
        assert after["errors"] == pc.ERR_TREE
        for f in pc.TREE_FIELDS:
            assert pc.same_bits(_root(after, f, p), _root(before, f, p)), f
        assert (sc.base.states[k]["visits"][p] != before["visits"][p]).any()  # while the healthy run's did
    elif name.startswith(("first_child_", "num_children_")):  # the ABSORB is the healthy one; the SELECT stops at the root
        assert after["errors"] == pc.ERR_TREE and grew == healthy_k and visited == {s: 1 for s in chain}
        assert after["selected"][p] == 0 and after["path_len"][p] == 0
        assert pc.same_bits(after["paths"][:, p], before["paths"][:, p])
    elif name == "parent_N":  # the node is expanded and backed up, the walk stops at its parent
        assert after["errors"] == pc.ERR_TREE and grew == healthy_k and visited == {node: 1}
    elif name == "parent_self":  # a loop is walked T + 1 times and is no error
        assert after["errors"] == 0 and grew == healthy_k and visited == {node: T + 1}
        assert after["value_sum"][p, node] == before["value_sum"][p, node] + (T + 1) * value[p]
    else:  # cand_count out of range is data: clamped, no error bit
        assert all(s["errors"] == 0 for s in sc.states)
        assert count[p] in (-3, K + 5) and grew == (0 if count[p] < 0 else min(K, C)) and visited == {s: 1 for s in chain}
        assert after["num_children"][p, node] == grew and (grew == 0 or after["first_child"][p, node] == before["num_nodes"][p])


def test_every_group_width_has_its_cases():
    """Which k_puct_advance<G> a GPU test runs cannot be seen without a device, so the mapping is recorded: the host picks
    G = group_lanes(max_children) (csrc/pcb_group.h, mirrored by puct_cases.group_lanes)."""
    assert [pc.group_lanes(C) for C in (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)] == [4, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 64]
    by_width = {}
    for name, (P, C, K, iterations, G, blocks) in pc.WIDTHS.items():
        by_width.setdefault(G, []).append((C, K, blocks))
    assert sorted(by_width) == [4, 8, 16, 32, 64]
    for G, rows in by_width.items():
        assert any(C == G for C, _, _ in rows) and any(C == G // 2 + 1 for C, _, _ in rows) and any(blocks == 3 for _, _, blocks in rows), G
    ks = [(K > C) - (K < C) for rows in by_width.values() for C, K, _ in rows]
    assert {-1, 0, 1} <= set(ks)  # K once below, once equal to and once above C
    assert {G for G, _ in pc.DAMAGE_CASES} == {4, 16, 64} and all(pc.group_lanes(pc.DAMAGE_GAMES[G][2]) == G for G in pc.DAMAGE_GAMES)


INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
FAR = [(f, v) for f in ("selected", "num_nodes", "first_child", "num_children", "parent") for v in (INT_MAX, INT_MIN)]


@pytest.mark.parametrize("f, value", FAR)
def test_values_far_out_of_range_send_no_access_outside_the_tensors(f, value):
    """On the CPU alone, where AddressSanitizer and UBSan turn a miss into a failure of replay(): the extremes of int32 in
    every tensor that holds a slot number or a count."""
    sc = pc.damaged(4, "selected_N")  # a healthy prefix after which root p is expanded and its selected node a fresh leaf
    P, N, C, T, K, p, k, node = sc.P, sc.N, sc.C, sc.T, sc.K, sc.p, sc.k, sc.node
    shp = pc.shapes(P, N, T)
    at = {"selected": (p,), "num_nodes": (p,), "first_child": (p, 0), "num_children": (p, 0), "parent": (p, node)}[f]
    seq = sc.base.seq[:k] + [dict(phases=pc.ABSORB | pc.SELECT, evaluation=sc.base.seq[k]["evaluation"], expect=None, pokes=[(f, pc.flat(shp[f], *at), value)])] + \
        [dict(phases=pc.ABSORB | pc.SELECT, evaluation=sc.base.seq[i]["evaluation"], expect=None) for i in (k + 1, k + 2)]
    states = pc.replay(P, N, C, T, K, sc.c_puct, seq)
    stray = (f, value) != ("parent", INT_MIN)  # a negative parent ends the walk as -1 does
    assert states[k]["errors"] == (pc.ERR_TREE if stray else 0)
    others = [q for q in range(P) if q != p]
    for g in pc.STATE_FIELDS:
        axis = 1 if g == "paths" else 0
        assert pc.same_bits(np.take(states[-1][g], others, axis), np.take(sc.base.states[k + 2][g], others, axis)), g
