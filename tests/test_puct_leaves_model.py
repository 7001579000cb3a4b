"""csrc/pcb_puct_leaves.h -- leaf-parallel selection with pending visits, expansion and backup of
pcbenv_puct_advance_leaves as plain C++ -- against its specification, pcbenv/search.py:puct_search(leaves=L), on the CPU:
tools/puct_leaves_check.cpp (AddressSanitizer + UBSan, a program of its own, nothing preloaded) replays recorded searches
call by call, checks every selection against the recorded one and returns its final tree, which must be puct_search's
field by field, floats by their bits (tests/puct_leaves_cases.py).

The reach assertions say what the recorded cases contain -- launches all of whose leaves are real, repeats, a bare root
selected L times, a terminal leaf selected twice, descents the pending visits turned, exact ties -- so that
tests/test_puct_leaves_gpu.py, which holds the kernel to the model on such cases, cannot be vacuous.  And the trees a
caller has damaged: the outcome csrc/pcb_puct_leaves.h promises, asserted on the model's dump under the sanitizers."""
import shutil

import numpy as np
import pytest
import torch

import puct_cases as pc
import puct_leaves_cases as lc
from pcbenv.search import puct_choose, puct_reroot, search_tree
from test_puct_search import CASES as TOY, T as TOY_T, evaluator_for

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("iterations, c_puct, max_children, K", TOY)
def test_the_toy_game(iterations, c_puct, max_children, K, L):
    P = 4
    ps, calls = lc.record(P, TOY_T, L, iterations, c_puct, max_children, lc.per_leaf(evaluator_for(P, K), P, TOY_T, K, L))
    states = lc.replay(P, 1 + iterations * L * max_children, max_children, TOY_T, K, L, c_puct, lc.search_calls(calls))
    lc.compare_with_search(states[-1], ps)
    assert states[-1]["errors"] == 0
    assert (states[-1]["visits"][:3, 0] > iterations).all() and (states[-1]["visits"][:, 0] <= iterations * L).all()  # more than one leaf per launch


@pytest.mark.parametrize("P, T, C, K, L, iterations", lc.MODEL_CASES)
def test_the_synthetic_evaluator(P, T, C, K, L, iterations):
    case = lc.synthetic(P, T, C, K, L, iterations)
    lc.compare_with_search(case.states[-1], case.ps)
    st = case.states[-1]
    assert st["errors"] == 0
    assert int(st["num_children"].max()) == min(K, C) and (st["num_children"] >= 0).all()   # K > C: truncated; K < C: never more than K
    # a condition on the cases, not a measurement: the specification alone keeps the repeats below half of all leaf rows
    assert lc.repeat_share(case) <= 0.5, lc.repeat_share(case)
    real = sum(int((c[1] >= 0).sum()) for c in case.calls)
    assert int(st["visits"][:, 0].sum()) == real  # every leaf was backed up to its root, and no row that is none was
    assert st["num_nodes"][5] == 1 and not st["terminal"][5, 0] and st["visits"][5, 0] == iterations  # no candidates: one leaf per launch, the rest repeats
    assert st["num_nodes"][6] == 1 and st["terminal"][6, 0] and st["visits"][6, 0] == 1 + (iterations - 1) * L  # terminal at the root: known from the second launch on
    for s, c in zip(case.states, case.seq):  # what SELECT left pending is what it selected: one visit per node of every leaf's chain
        if c["phases"] & lc.SELECT:
            assert int(s["pending"][:, 0].sum()) == int((s["selected"] >= 0).sum())
    facts = lc.case_facts(case)  # the launches again, in Python floats: selected, path_len and pending of every SELECT
    if L == 1:
        assert not facts["parted"] and not facts["repeat_behind"] and not lc.repeat_share(case)


def test_the_node_wise_evaluator_is_the_synthetic_one():
    """puct_leaves_cases.leaves_evaluator against tests/puct_cases.py:synthetic_evaluator with root = row // L, every output of
    every row of recorded launches by its bits; and pcbenv.search.sqrt_rn, which the specification's score takes, is the
    correctly rounded root of every count up to 2^20 and of a spread of larger ones."""
    for P, T, K, L in ((14, 5, 3, 3), (14, 5, 7, 8)):
        slow = lc.per_leaf(lc.synthetic_evaluator(P, T, K, 11), P, T, K, L)
        _, calls = lc.record(P, T, L, 6, 1.25, 5, lc.leaves_evaluator(P, T, K, L, 11))
        for c in calls:
            ev = slow(torch.from_numpy(c[0]), torch.from_numpy(c[1]), 0)
            for a, b in zip(c[2:], (ev.value, ev.terminal, ev.cand_count, ev.cand_actions, ev.cand_prior)):
                assert a.tobytes() == b.numpy().tobytes()
    from pcbenv.search import sqrt_rn
    x = torch.cat([torch.arange(1, 1 << 20), torch.arange(1, 1 << 20) * 2039 + 7]).to(torch.float64)
    assert np.array_equal(sqrt_rn(x).numpy(), np.sqrt(x.numpy()))


def test_one_leaf_is_pcb_puct_h_call_by_call():
    """L = 1: the call sequence through csrc/pcb_puct_leaves.h and through csrc/pcb_puct.h gives identical states, and the
    states of tests/puct_cases.py's recording of the same search, which knows nothing of leaves; pending is zero after
    every ABSORB."""
    for C, K in ((1, 2), (3, 3), (5, 7)):
        case = lc.synthetic(14, 5, C, K, 1, 14)
        plain = lc.replay(case.P, case.N, C, 5, K, 1, case.c_puct, case.seq, via=1)
        old = pc.synthetic(14, 5, C, K, 14)
        assert len(plain) == len(case.states) == len(old.states)
        for a, b, o, c in zip(case.states, plain, old.states, case.seq):
            for f in pc.STATE_FIELDS:
                assert lc.same_bits(a[f], b[f]) and lc.same_bits(a[f], o[f]), f
            assert a["errors"] == b["errors"] == o["errors"]
            assert not b["pending"].any()
            if c["phases"] & lc.SELECT:  # the selection is pending, nothing else
                assert int(a["pending"].sum()) == int((a["path_len"] + 1).sum())
            else:
                assert not a["pending"].any()


@pytest.mark.parametrize("L, C, K", [(2, 3, 3), (3, 5, 7), (8, 3, 2), (8, 1, 1)])
def test_nothing_is_pending_after_an_absorb(L, C, K):
    """One phase per call: the state after every ABSORB has pending zero everywhere, and the split sequence ends as the
    combined one."""
    both, split = lc.synthetic(14, 5, C, K, L, 14), lc.synthetic(14, 5, C, K, L, 14, split=True)
    absorbs = 0
    for s, c in zip(split.states, split.seq):
        if c["phases"] == lc.ABSORB:
            absorbs += 1
            assert not s["pending"].any()
        elif c["phases"] == lc.SELECT:
            assert s["pending"].any()
    assert absorbs == 14
    for f in lc.STATE_FIELDS:
        assert lc.same_bits(both.states[-1][f], split.states[-1][f]), f


def test_a_searched_tree_is_rerooted_and_searched_again():
    """L = 4: the tree of a search, given to puct_choose / puct_reroot and searched again, is the specification's: the model
    continues in the rerooted tree (pending zero, as the first search left it)."""
    P, T, C, K, L, M = 14, 5, 3, 3, 4, 8
    first = lc.synthetic(P, T, C, K, L, M, capacity=1 + 2 * M * L * C)
    tree = search_tree(first.ps)
    move = puct_choose(tree, C)
    kept, remap = puct_reroot(tree, move["move_slot"])
    assert (move["move_slot"] > 0).sum() >= P // 2 and int((remap >= 0).sum(dim=1).max()) > 1 + C  # subtrees with more than a root's children
    ps, calls = lc.record(P, T, L, M, first.c_puct, C, lc.leaves_evaluator(P, T, K, L, 23), step_index=900, tree=kept)
    seq = lc.search_calls(calls)
    seq[0] = dict(seq[0], phases=lc.SELECT, load={f: kept[f] for f in lc.TREE_FIELDS})  # a kept tree: no INIT
    states = lc.replay(P, first.N, C, T, K, L, first.c_puct, seq)
    lc.compare_with_search(states[-1], ps)
    assert int(states[-1]["depth"].max()) >= 2 and (states[-1]["visits"][:, 0] > torch.as_tensor(kept["visits"])[:, 0].numpy()).all()


def test_a_full_tree_stops_growing_all_or_nothing():
    free = lc.synthetic(14, 5, 3, 3, 3, 14)
    full = lc.synthetic(14, 5, 3, 3, 3, 14, capacity=8)
    lc.compare_with_search(full.states[-1], full.ps)
    a, b = free.states[-1], full.states[-1]
    assert (a["num_nodes"] > 8).any() and (b["num_nodes"] <= 8).all()
    assert b["errors"] & lc.ERR_FULL and not a["errors"]
    for p in range(14):  # every node in use has all the children it was given: none was made in part
        n = int(b["num_nodes"][p])
        k, fc = b["num_children"][p, :n], b["first_child"][p, :n]
        assert 1 + k.sum() == n and (b["num_children"][p, n:] == 0).all()
        assert all(fc[s] + k[s] <= n for s in range(n) if k[s]) and (b["parent"][p, n:] == -1).all()
    real = sum(int((c[1] >= 0).sum()) for c in full.calls)
    assert int(b["visits"][:, 0].sum()) == real and not b["pending"].any()  # every leaf was backed up, refused or not
    assert sum(bool(s["errors"] & lc.ERR_FULL) for s in full.states) > 5


def test_the_recorded_cases_reach_what_the_gpu_test_relies_on():
    """At least one of each in the cases of this file, and in those the GPU test runs (tests/puct_leaves_cases.py:GPU_CASES)."""
    for cases in ([lc.synthetic(*row) for row in lc.MODEL_CASES if row[4] > 1], [lc.gpu_case(n) for n in lc.GPU_CASES if lc.GPU_CASES[n][2] > 1]):
        total = {}
        for case in cases:
            for k, v in lc.case_facts(case).items():
                total[k] = total.get(k, 0) + v
        assert total["all_real"] > 0, "no launch in which every leaf of some root is real"
        assert total["repeat_behind"] > 0, "no repeat at l >= 1"
        assert total["bare_root"] > 0, "no launch in which all L leaves select the bare root"
        assert total["terminal_twice"] > 0, "no terminal leaf selected twice in one launch"
        assert total["parted"] > 0, "no descent that a pending visit turned away from the child it would have taken"
        assert total["ties"] > 0, "no exact score tie"
    for name in lc.GPU_CASES:
        C, K, L, iterations = lc.GPU_CASES[name]
        case = lc.gpu_case(name)
        assert case.N == 1 + 40 * C and case.P == 130 and case.T == 5
        assert lc.repeat_share(case) <= 0.5, (name, lc.repeat_share(case))  # the condition on every case, whatever its L
    assert {lc.GPU_CASES[n][0] for n in lc.GPU_CASES} == {1, 4, 5, 16, 32, 33, 64} and {lc.GPU_CASES[n][2] for n in lc.GPU_CASES} == {1, 2, 3, 8, 64}
    assert [pc.group_lanes(C) for C in (1, 4, 5, 16, 32, 33, 64)] == [4, 4, 8, 16, 32, 64, 64] and -(-130 // (256 // 4)) == 3  # G = 4 spans three blocks
    assert any(lc.gpu_case(n).states[-1]["errors"] & lc.ERR_FULL for n in lc.GPU_CASES) and any(not lc.gpu_case(n).states[-1]["errors"] for n in lc.GPU_CASES)


# ---- trees the caller has damaged ----------------------------------------------------------------------------------
def _root(state, f, p, L):
    return state[f][:, p * L:(p + 1) * L] if f == "paths" else state[f][p * L:(p + 1) * L] if f in ("selected", "path_len") else state[f][p]


def _others(sc, state, f):
    keep = [q for q in range(sc.P) if q != sc.p]
    if f in ("selected", "path_len", "paths"):
        rows = [q * sc.L + l for q in keep for l in range(sc.L)]
        return np.take(state[f], rows, 1 if f == "paths" else 0)
    return np.take(state[f], keep, 0)


@pytest.mark.parametrize("G, name", lc.DAMAGE_CASES)
def test_a_damaged_tree_ends_as_pcb_puct_leaves_h_promises(G, name):
    """The sanitizers saw no stray access (replay() asserts an empty stderr), the other roots advance as in the healthy run,
    and the damaged root reports what the header says: the GPU test of the same scenario then only has to equal the model."""
    sc = lc.damaged(G, name)
    k, p, N, C, T, L, node = sc.k, sc.p, sc.N, sc.C, sc.T, sc.L, sc.node
    assert 0 < p < sc.P - 1 and pc.group_lanes(C) == G and len(sc.seq) == k + 3
    for i in (k, k + 1, k + 2):
        for f in lc.STATE_FIELDS:
            assert lc.same_bits(_others(sc, sc.states[i], f), _others(sc, sc.base.states[i], f)), (i, f)
    before, after = sc.states[k - 1], sc.states[k]
    real = int((before["selected"][p * L:(p + 1) * L] >= 0).sum())
    absorbed = int(after["visits"][p, 0] - before["visits"][p, 0])
    if name.startswith("selected_"):  # the leaves before the damaged row are absorbed, the root's phase ends at it
        assert after["errors"] == lc.ERR_TREE
        row = sc.seq[k]["pokes"][0][1] - p * L  # `selected` is [P * L]: the flat index is the row
        assert row in (0, 1) and absorbed == row
    elif name.startswith("num_nodes_"):  # the ABSORB of root p does nothing at all
        assert after["errors"] == lc.ERR_TREE and absorbed == 0
        for f in ("parent", "depth", "visits", "num_children", "first_child", "node_action", "prior", "value_sum", "value_max", "terminal", "reward_lo", "reward_hi"):
            assert lc.same_bits(after[f][p], before[f][p]), f
    elif name.startswith(("first_child_", "num_children_")):  # the ABSORB is the healthy one; every descent stops at the root
        assert after["errors"] == lc.ERR_TREE and absorbed == real
        assert (after["selected"][p * L:(p + 1) * L] == 0).all() and (after["path_len"][p * L:(p + 1) * L] == 0).all()
        assert lc.same_bits(after["paths"][:, p * L:(p + 1) * L], before["paths"][:, p * L:(p + 1) * L])
        assert after["pending"][p, 0] == L and int(after["pending"][p].sum()) == L
    elif name == "parent_N":  # the walk of leaf 0 stops at the node's parent, and with it the root's phase
        assert after["errors"] == lc.ERR_TREE and absorbed == 0 and after["visits"][p, node] == before["visits"][p, node] + 1
    elif name == "parent_self":  # a loop is walked T + 1 times and is no error
        assert after["errors"] == 0 and after["visits"][p, node] == before["visits"][p, node] + T + 1
    else:  # pending is data: whatever it holds, no error, no store out of range, and the tree stays a tree
        assert all(s["errors"] == 0 for s in sc.states) and absorbed == real
        n = int(after["num_nodes"][p])
        assert 1 <= n <= N and (after["parent"][p, 1:n] >= 0).all() and (after["parent"][p, 1:n] < n).all()
        assert (after["selected"][p * L:(p + 1) * L] < n).all()


INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
FAR = [(f, v) for f in ("selected", "num_nodes", "first_child", "num_children", "parent", "pending") for v in (INT_MAX, INT_MIN)]


@pytest.mark.parametrize("f, value", FAR)
def test_values_far_out_of_range_send_no_access_outside_the_tensors(f, value):
    """On the CPU alone, where AddressSanitizer and UBSan turn a miss -- or an int32 sum that overflows -- into a failure of
    replay(): the extremes of int32 in every tensor that holds a slot number or a count, and in pending."""
    sc = lc.damaged(4, "selected_N")
    P, N, C, T, K, L, p, k, node = sc.P, sc.N, sc.C, sc.T, sc.K, sc.L, sc.p, sc.k, sc.node
    shp = lc.shapes(P, N, T, L)
    at = {"selected": (p * L,), "num_nodes": (p,), "first_child": (p, 0), "num_children": (p, 0), "parent": (p, node), "pending": (p, 0)}[f]
    pokes = [(f, lc.flat(shp[f], *at), value)] + ([("pending", lc.flat(shp[f], p, node), value)] if f == "pending" else [])
    seq = sc.seq[:k] + [dict(sc.seq[k], pokes=pokes)] + sc.seq[k + 1:]
    states = lc.replay(P, N, C, T, K, L, sc.c_puct, seq)
    stray = f != "pending" and (f, value) != ("parent", INT_MIN)  # a negative parent ends the walk as -1 does; pending is data
    assert states[k]["errors"] == (lc.ERR_TREE if stray else 0)
    for g in lc.STATE_FIELDS:
        assert lc.same_bits(_others(sc, states[-1], g), _others(sc, sc.base.states[k + 2], g)), g
