"""csrc/pcb_tree.h -- selection, expansion and backup of pcbenv_tree_advance as plain C++ -- against its specification,
pcbenv/search.py:tree_search, on the CPU: tools/tree_model_check.cpp (AddressSanitizer + UBSan, a program of its own,
nothing preloaded) replays recorded searches call by call, checks every selection against the recorded one and returns
its final tree, which must be tree_search's field by field, floats by their bits (tests/tree_cases.py).

Also the condition under which the device search (whose ln n comes from a table) and tree_search (which calls log) cannot
part ways: no selection of any case the GPU tests use has two scores closer than 1e-12 that are not exactly equal."""
import math
import shutil

import numpy as np
import pytest

import tree_cases as tc
from test_tree_search import EXPECT_ROOT0, T as TOY_T, backend_for

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

TOY = [(5, 1.0, 2), (24, 1.0, 2), (24, 0.3, 2), (16, 1.0, 1), (12, 2.0, 3)]  # tests/test_tree_search.py's
SYNTHETIC = [(7, 5, C, 40) for C in (1, 3, 5)]


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


@pytest.mark.parametrize("P, T, C, iterations", SYNTHETIC)
def test_the_synthetic_game(P, T, C, iterations):
    case = tc.synthetic(P, T, C, iterations)
    tc.compare_with_search(case.states[-1], case.ts, case.N)
    assert case.states[-1]["errors"] == 0
    st = case.states[-1]
    assert (st["num_nodes"][5] == 1) and st["visits"][5, 0] == iterations   # the refused root: every playout went into the root
    assert st["terminal"][6, 1:st["num_nodes"][6]].all()                      # the root whose episode is over: terminal children only
    if C > 1:  # exact ties occurred and went to the lowest slot: the selections were checked against tree_search's
        ties = sum(_exact_ties(s, C, case.c_uct, case.N) for s, c in zip(case.states, case.seq) if c["phases"] & tc.SELECT)
        assert ties > 0


def _exact_ties(state, C, c_uct, N):
    """Levels of the descents of `state` at which the best score occurs twice."""
    n = 0
    ln = tc.ln_table(N).numpy()
    for p in range(state["num_nodes"].shape[0]):
        lo, hi, node = float(state["reward_lo"][p]), float(state["reward_hi"][p]), 0
        while not state["terminal"][p, node] and state["num_children"][p, node] == C:
            sc = []
            for c in range(C):
                ch = int(state["children"][p, node, c])
                n_c = float(max(int(state["visits"][p, ch]), 1))
                q = (float(state["value_sum"][p, ch]) / n_c - lo) / (hi - lo) if hi > lo else 0.0
                sc.append(q + c_uct * math.sqrt(float(ln[max(int(state["visits"][p, node]), 1)]) / n_c))
            n += sc.count(max(sc)) > 1
            node = int(state["children"][p, node, sc.index(max(sc))])
    return n


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
