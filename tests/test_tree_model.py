"""csrc/pcb_tree.h -- selection, expansion and backup of pcbenv_tree_advance as plain C++ -- against its specification,
pcbenv/search.py:tree_search, on the CPU: tools/tree_model_check.cpp (AddressSanitizer + UBSan, a program of its own,
nothing preloaded) replays recorded searches call by call, checks every selection against the recorded one and returns
its final tree, which must be tree_search's field by field, floats by their bits (tests/tree_cases.py).

Also the condition under which the device search (whose ln n comes from a table) and tree_search (which calls log) cannot
part ways: no selection of any case the GPU tests use has two scores closer than 1e-12 that are not exactly equal.

And the trees a caller has damaged (tree_cases.damaged): the outcome csrc/pcb_tree.h promises for each kind of damage is
asserted here on the model's dump, under the sanitizers; tests/test_tree_advance_gpu.py then holds the kernel to the model."""
import shutil

import numpy as np
import pytest

import tree_cases as tc
from test_tree_search import EXPECT_ROOT0, T as TOY_T, backend_for

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

TOY = [(5, 1.0, 2), (24, 1.0, 2), (24, 0.3, 2), (16, 1.0, 1), (12, 2.0, 3)]  # tests/test_tree_search.py's
SYNTHETIC = [(7, 5, C, 40) for C in (1, 3, 5)]
WIDTHS = {(P, tc.WIDTH_T, C, iterations): name for name, (P, C, iterations, *_) in tc.WIDTHS.items()}  # every group width, three blocks


@pytest.mark.parametrize("iterations, c_uct, max_children", TOY)
def test_the_toy_game(iterations, c_uct, max_children):
    P = 3
    ts, calls = tc.record(P, TOY_T, iterations, c_uct, max_children, backend_for(P))
    seq = tc.search_calls(calls)
    states = tc.replay(P, iterations + 1, max_children, TOY_T, c_uct, seq)
    tc.compare_with_search(states[-1], ts, iterations + 1)
    assert states[-1]["errors"] == 0
    if (iterations, c_uct, max_children) == (5, 1.0, 2):  # the tree worked out on paper
        st, e = states[-1], EXPECT_ROOT0
        assert st["parent"][0].tolist() == e["parent"] and st["depth"][0].tolist() == e["depth"] and st["visits"][0].tolist() == e["visits"]
        assert st["node_action"][0, :, 2].tolist() == e["b"] and st["children"][0].tolist() == e["children"]
        assert st["value_sum"][0].tolist() == e["vsum"] and st["value_max"][0].tolist() == e["vmax"]
        assert st["terminal"][0].astype(bool).tolist() == e["terminal"]


@pytest.mark.parametrize("P, T, C, iterations", SYNTHETIC + list(WIDTHS))
def test_the_synthetic_game(P, T, C, iterations):
    row = (P, T, C, iterations)
    case = tc.width_case(WIDTHS[row]) if row in WIDTHS else tc.synthetic(P, T, C, iterations)  # width_case: with the checks that the row reaches what it is there for
    tc.compare_with_search(case.states[-1], case.ts, case.N)
    assert case.states[-1]["errors"] == 0
    st = case.states[-1]
    assert (st["num_nodes"][5] == 1) and st["visits"][5, 0] == iterations   # the refused root: every playout went into the root
    assert st["terminal"][6, 1:st["num_nodes"][6]].all()                      # the root whose episode is over: terminal children only
    if C > 1:  # exact ties occurred and went to the lowest slot: the selections were checked against tree_search's
        assert tc.ties(case) > 0


def test_a_full_tree_stops_growing():
    free = tc.synthetic(7, 5, 3, 40)
    full = tc.synthetic(7, 5, 3, 40, capacity=4)
    a, b = free.states[-1], full.states[-1]
    assert (a["num_nodes"] > 4).any()
    grew = a["num_nodes"] > 4
    assert (b["num_nodes"][grew] == 4).all() and (b["num_nodes"] <= 4).all()
    assert b["errors"] & 1 and not a["errors"]
    for f in ("parent", "depth", "node_action", "terminal"):  # the structure of the first four slots: the uncapped tree's
        for p in range(7):
            n = min(4, int(a["num_nodes"][p]))
            assert np.array_equal(a[f][p, :n], b[f][p, :n]), (f, p)
    assert (b["visits"][:, 0] == 40).all()  # every playout was absorbed: into existing nodes once the tree was full
    once_full = [s for s in full.states if (s["num_nodes"][grew] == 4).all()]
    assert len(once_full) > 10 and all((s["num_nodes"] <= 4).all() for s in once_full)


def test_no_selection_is_closer_than_a_rounding_of_log():
    """Over the recorded runs above and every search the GPU tests make on real roots."""
    found = {}
    for P, T, C, iterations in SYNTHETIC:
        case = tc.synthetic(P, T, C, iterations)
        found[f"synthetic C={C}"] = tc.min_gap(case.states, case.seq, C, case.c_uct, case.N)
    for name in tc.WIDTHS:
        case = tc.width_case(name)
        found[name] = tc.min_gap(case.states, case.seq, case.C, case.c_uct, case.N)
    for iterations, c_uct, C in TOY:
        ts, calls = tc.record(3, TOY_T, iterations, c_uct, C, backend_for(3))
        seq = tc.search_calls(calls)
        found[f"toy {iterations} {c_uct} {C}"] = tc.min_gap(tc.replay(3, iterations + 1, C, TOY_T, c_uct, seq), seq, C, c_uct, iterations + 1)
    for name, iterations in tc.ORACLE_CASES:
        case = tc.oracle_case(name, iterations)
        tc.compare_with_search(case.states[-1], case.ts, case.N)
        found[name] = tc.min_gap(case.states, case.seq, case.C, case.c_uct, case.N)
    print(found)
    for what, gap in found.items():
        assert gap > tc.GAP_BOUND, (what, gap)


# ---- trees the caller has damaged ----------------------------------------------------------------------------------
def _root(state, f, p):
    return state[f][:, p] if f in ("paths", "best_actions") else state[f][p]


def _poked(state, pokes):
    st = {f: np.array(v) for f, v in state.items() if f != "errors"}
    for f, at, value in pokes:
        st[f].reshape(-1)[at] = value
    return st


@pytest.mark.parametrize("G, name", tc.DAMAGE_CASES)
def test_a_damaged_tree_ends_as_pcb_tree_h_promises(G, name):
    """The outcome csrc/pcb_tree.h states for each kind of damage, on the model's dump (the sanitizers saw no stray
    access: replay() asserts an empty stderr): the GPU test of the same scenario then only has to equal the model."""
    sc = tc.damaged(G, name)
    k, p, N, C, T, node = sc.k, sc.p, sc.N, sc.C, sc.T, sc.node
    alone = name.endswith("absorb_alone")
    assert 0 < p < sc.P - 1 and tc.group_lanes(C) == G and len(sc.seq) == k + 3
    assert sc.states[k - 1]["errors"] == 0 and sc.states[k - 1]["num_children"][p, 0] == C
    before, after = _poked(sc.states[k - 1], sc.seq[k]["pokes"]), sc.states[k]
    others = [q for q in range(sc.P) if q != p]
    for i in (k,) if alone else (k, k + 1, k + 2):  # the other roots advance as in the healthy run
        for f in tc.TREE_FIELDS if alone else tc.STATE_FIELDS:
            axis = 1 if f in ("paths", "best_actions") else 0
            assert tc.same_bits(np.take(sc.states[i][f], others, axis), np.take(sc.base.states[i][f], others, axis)), (i, f)
    grew = int(after["num_nodes"][p] - before["num_nodes"][p])
    visited = {int(s): int(n) for s, n in enumerate(after["visits"][p] - before["visits"][p]) if n}
    reward = None if sc.hand is None else sc.hand[0]
    if name.startswith(("selected_", "num_nodes_")):  # 1, 2: the ABSORB of root p does nothing at all
        assert after["errors"] == tc.ERR_TREE
        for f in tc.TREE_FIELDS:
            assert tc.same_bits(_root(after, f, p), _root(before, f, p)), f
        assert (sc.base.states[k]["visits"][p] != before["visits"][p]).any()  # while the healthy run's did
    elif name.startswith("last_child_bad"):  # 3a: the match below the bad slot counts; the SELECT then stops at the root
        assert grew == 0 and visited == {0: 1, sc.child[0]: 1}
        assert after["value_sum"][p, sc.child[0]] == before["value_sum"][p, sc.child[0]] + reward
        if alone:
            assert after["errors"] == 0 and sc.states[k + 1]["errors"] == tc.ERR_TREE
            after = sc.states[k + 1]
        assert after["errors"] == tc.ERR_TREE and after["path_len"][p] == 0 and after["selected"][p] == 0
    elif "_child_bad" in name:  # 3b, 3c: nothing from the bad slot on counts; the playout goes into the root alone
        assert after["errors"] == tc.ERR_TREE and grew == 0 and visited == {0: 1}
        assert after["value_sum"][p, 0] == before["value_sum"][p, 0] + reward
    elif name == "parent_N":  # 4: the node is backed up, the walk stops at its parent
        assert before["depth"][p, node] == 1 and after["errors"] == tc.ERR_TREE and grew == 0 and visited == {node: 1}
    elif name == "parent_self":  # 5: a loop is walked T + 1 times and is no error
        assert before["depth"][p, node] == 1 and after["errors"] == 0 and grew == 0 and visited == {node: T + 1}
        assert after["value_sum"][p, node] == before["value_sum"][p, node] + (T + 1) * reward
    elif name == "root_its_own_child":  # 5: T levels, each the root's own action
        assert all(s["errors"] == 0 for s in sc.states)
        assert after["path_len"][p] == T and after["selected"][p] == 0
        assert (after["paths"][:, p] == before["node_action"][p, 0]).all()
    elif name.startswith("depth_"):  # 6: the action comes from the clamped row; the child's depth and flag follow the stored depth
        d, slot, nch = int(before["depth"][p, node]), int(before["num_nodes"][p]), int(before["num_children"][p, node])
        assert d in (-1, T, T + 3) and after["errors"] == 0 and grew == 1
        assert sc.hand[2] == min(max(d, 0), T - 1) and tuple(after["node_action"][p, slot]) == tc.NO_ACTION
        assert after["parent"][p, slot] == node and after["children"][p, node, nch] == slot and after["num_children"][p, node] == nch + 1
        assert after["depth"][p, slot] == d + 1 and after["terminal"][p, slot] == (sc.hand[1] <= d + 1)
        assert visited[slot] == 1 and visited[node] == 1
    else:  # 6: a child count out of range makes no child, and the walk over the children ends at C
        assert name.startswith("num_children_") and before["num_children"][p, 0] in (-1, C + 5)
        assert after["errors"] == 0 and grew == 0 and visited == {0: 1}
        assert (after["path_len"][p] == 0) == (name == "num_children_minus_1")


def test_every_group_width_has_its_cases():
    """Which k_tree_advance<G> a GPU test runs cannot be seen without a device, so the mapping is recorded: the host picks
    G = group_lanes(max_children) (csrc/pcb_group.h, mirrored by tree_cases.group_lanes), and the cases of
    tests/test_tree_advance_gpu.py are these (DESIGN.md lists them under k_tree_advance)."""
    from test_tree_advance_gpu import REPLAYS
    assert [tc.group_lanes(C) for C in (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)] == [4, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 64]
    by_width = {}
    for name, (P, T, C, iterations, capacity, split, cells) in REPLAYS.items():
        by_width.setdefault(tc.group_lanes(C), []).append((name, C, -(-P // (tc.BLOCK // tc.group_lanes(C)))))
    assert {G: sorted(n for n, _, _ in rows) for G, rows in by_width.items()} == {
        4: ["C3", "G4_C4_P130", "T1", "capacity4", "chain_C1", "one_phase_per_call"], 8: ["C5_P67", "G8_C8_P70"],
        16: ["G16_C16_P35", "G16_C9_P35"], 32: ["G32_C17_P19", "G32_C32_P19"], 64: ["C64_P1", "G64_C33_P9", "G64_C63_P9"]}
    for G, rows in by_width.items():  # every width: every lane with a child, the most idle lanes, a second and a third block
        assert any(C == G for _, C, _ in rows) and any(C == G // 2 + 1 for _, C, _ in rows) and any(blocks == 3 for _, _, blocks in rows), G
    assert {G for G, _ in tc.DAMAGE_CASES} == {4, 16, 64} and all(tc.group_lanes(tc.DAMAGE_GAMES[G][2]) == G for G in tc.DAMAGE_GAMES)


INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
FAR = [("selected", INT_MAX), ("selected", INT_MIN), ("num_nodes", INT_MAX), ("num_nodes", INT_MIN), ("children", INT_MAX), ("children", INT_MIN),
       ("parent", INT_MAX), ("parent", INT_MIN), ("num_children", INT_MAX), ("num_children", INT_MIN), ("depth", INT_MIN), ("depth", INT_MAX - 1)]


@pytest.mark.parametrize("f, value", FAR)
def test_values_far_out_of_range_send_no_access_outside_the_tensors(f, value):
    """On the CPU alone, where AddressSanitizer and UBSan turn a miss into a failure of replay(): the extremes of int32 in
    every tensor that holds a slot number or a count (depth == INT_MAX is left out: csrc/pcb_tree.h checks slot numbers, and
    make_child's depth + 1 is the caller's to keep in range)."""
    sc = tc.damaged(4, "first_child_bad")  # a healthy prefix after which root p is full
    P, N, C, T, p, k = sc.P, sc.N, sc.C, sc.T, sc.p, sc.k
    shp = tc.shapes(P, N, C, T)
    node = sc.child[0]
    at = {"selected": (p,), "num_nodes": (p,), "children": (p, 0, 1), "parent": (p, node), "num_children": (p, 0), "depth": (p, 0)}[f]
    pokes = [(f, tc.flat(shp[f], *at), value)]
    if f in ("children", "num_children", "depth"):
        pokes.append(("selected", p, 0))
    elif f == "parent":
        pokes.append(("selected", p, node))
    reward, length, actions = (np.array(a, copy=True) for a in sc.base.seq[k]["playout"])
    length[p], actions[:, p] = (1 if f == "parent" else T + 4), tc.NO_ACTION
    seq = sc.base.seq[:k] + [dict(phases=tc.ABSORB | tc.SELECT, playout=(reward, length, actions), expect=None, pokes=pokes)] + \
        [dict(phases=tc.ABSORB | tc.SELECT, playout=sc.base.seq[i]["playout"], expect=None) for i in (k + 1, k + 2)]
    states = tc.replay(P, N, C, T, sc.c_uct, seq)
    stray = f in ("selected", "num_nodes", "children") or (f, value) == ("parent", INT_MAX)  # a negative parent ends the walk as -1 does
    assert states[k]["errors"] == (tc.ERR_TREE if stray else 0)
    others = [q for q in range(P) if q != p]
    for g in tc.TREE_FIELDS:
        axis = 1 if g in ("paths", "best_actions") else 0
        assert tc.same_bits(np.take(states[-1][g], others, axis), np.take(sc.base.states[k + 2][g], others, axis)), g
