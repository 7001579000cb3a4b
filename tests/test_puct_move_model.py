"""csrc/pcb_puct_move.h -- the choice of a move and the compaction of its subtree as plain C++ -- against its
specification, pcbenv/search.py:puct_choose and puct_reroot, on the CPU: tools/puct_move_check.cpp (AddressSanitizer +
UBSan, a program of its own, nothing preloaded) runs the cases of tests/puct_move_cases.py and returns every tensor after
every call, which must be the specification's field by field, floats by their bits.

And the trees a caller has damaged (puct_move_cases.damaged): untouched, remap -1, bit 1 -- asserted here on the model's
dump, under the sanitizers; tests/test_puct_move_gpu.py then holds the kernel to the model."""
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import puct_cases as pc
import puct_move_cases as mc
import sampling_contract as sc
from pcbenv.search import MOVE_GREEDY, MOVE_PROPORTIONAL, puct_choose, puct_reroot, puct_result, puct_search, search_tree

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _torch_tree(tree):
    return {f: torch.from_numpy(np.ascontiguousarray(v)) for f, v in tree.items()}


def _same(state, f, t):
    t = t.numpy() if isinstance(t, torch.Tensor) else t
    if f in mc.FLOATS:
        assert pc.same_bits(state[f], t.astype(np.float64)), f
    else:
        assert np.array_equal(state[f], t.astype(np.int64)), f


def _filled(state, fields, shp):
    for f in fields:
        assert (state[f] == (-7.0 if f in mc.FLOATS else mc.FILL)).all() and state[f].shape == shp[f], f


def test_the_cases_are_what_they_are_there_for():
    cases = mc.check_cases()
    assert (mc.CHOOSE, mc.REROOT, mc.GREEDY, mc.PROPORTIONAL) == (1, 2, MOVE_GREEDY, MOVE_PROPORTIONAL)
    blocks = [-(-c.P // 4) for c in cases]  # four roots per workgroup
    assert max(blocks) > 1 and any(c.P % 4 for c in cases)


def test_the_constructed_shapes_are_what_they_are_there_for():
    """The spans, chunks and chains of REROOT's three passes that each constructed shape reaches, counted from the trees and
    the moves (puct_move_cases.coverage); and the old shapes' counts, which say why they do not do."""
    cov = mc.check_constructed()
    assert set(cov) == set(mc.CONSTRUCTED) and mc.ALL_SHAPES == tuple(mc.SHAPES) + tuple(mc.CONSTRUCTED)
    old = [mc.coverage(mc.case(n)) for n in mc.SHAPES]
    assert sum(len(v.below_kept) for v in old) < 64 and max(v.longest for v in old) < mc.LANES - 1 and max(max(v.num_nodes) for v in old) <= 2 * mc.SPAN
    for name in mc.CONSTRUCTED:
        c = mc.case(name)
        for p in range(c.P):
            _well_formed({f: c.tree[f][p] for f in mc.TREE_FIELDS}, c.C)
            n = int(c.tree["num_nodes"][p])
            assert set(c.tree["visits"][p, :n][c.tree["num_children"][p, :n] == 0]) <= {0, 1, 2, 3} and set(c.tree["prior"][p, 1:n]) <= set(pc.PRIORS)


@pytest.mark.parametrize("way", mc.WAYS)
@pytest.mark.parametrize("name", mc.ALL_SHAPES)
def test_the_model_is_the_specification(name, way):
    c = mc.case(name)
    states = mc.modelled(name, way)
    shp = mc.shapes(c.P, c.N, c.C)
    tree = _torch_tree(c.tree)
    last = states[-1]
    assert all(s["errors"] == 0 for s in states)
    if way == "given_move":
        move = torch.from_numpy(c.move_slot)
        _filled(last, ("move_action", "child_visits", "child_actions", "root_value"), shp)  # a phase not asked for writes nothing
        assert np.array_equal(last["move_slot"], c.move_slot)
    else:
        ch = puct_choose(tree, c.C, c.mode, mc.SEED, mc.STEP, mc.FIRST_ROOT)
        for f in ("move_slot", "move_action", "child_visits", "child_actions", "root_value"):
            _same(states[0], f, ch[f])
        move = ch["move_slot"]
        if way == "two_launches":
            _filled(states[0], ("remap",), shp)
            for f in mc.TREE_FIELDS:
                _same(states[0], f, tree[f])
            for f in ("move_slot", "move_action", "child_visits", "child_actions", "root_value"):
                assert pc.same_bits(states[0][f], states[1][f]), f
    new, remap = puct_reroot(tree, move, torch.from_numpy(c.reset))
    for f in mc.TREE_FIELDS:
        _same(last, f, new[f])
    _same(last, "remap", remap)
    for f in mc.TREE_FIELDS:  # puct_reroot does not modify what it is given
        assert pc.same_bits(tree[f].numpy(), c.tree[f]), f
    if way == "given_move":  # what the kinds mean, on the result
        for p in range(c.P):
            n_new, kept = int(last["num_nodes"][p]), c.kept[p]
            if c.kinds[p] in ("minus_1", "reset"):
                assert n_new == 1 and (last["remap"][p] == -1).all() and last["visits"][p, 0] == 0 and np.isinf(last["reward_lo"][p])
            elif c.kinds[p] == "slot_0":
                assert n_new == c.tree["num_nodes"][p] and (last["remap"][p, :n_new] == np.arange(n_new)).all()
                for f in mc.TREE_FIELDS:
                    assert pc.same_bits(last[f][p], c.tree[f][p].astype(last[f].dtype)), f
            else:
                assert n_new == kept and sorted(np.flatnonzero(last["remap"][p] >= 0)) == mc.subtree(c.tree, p, int(c.move_slot[p]))
                assert last["visits"][p, 0] == c.tree["visits"][p, c.move_slot[p]] and last["parent"][p, 0] == -1 and last["depth"][p, 0] == 0
                if c.kinds[p] == "zero_visits":
                    assert n_new == 1
            _well_formed({f: last[f][p] for f in mc.TREE_FIELDS}, c.C)


def _well_formed(t, C):
    """The invariants of one root's tree: parents below children, children consecutive and in order, visits of a node >= the
    sum of its children's, depth = the parent's + 1, unused slots as INIT leaves them."""
    n = int(t["num_nodes"])
    assert 1 <= n <= len(t["parent"]) and t["parent"][0] == -1 and t["depth"][0] == 0
    owned = np.zeros(n, np.int64)  # how many child ranges a slot lies in
    for s in range(n):
        k, fc = int(t["num_children"][s]), int(t["first_child"][s])
        assert 0 <= k <= C
        if s:
            q = int(t["parent"][s])
            assert 0 <= q < s and t["depth"][s] == t["depth"][q] + 1 and t["first_child"][q] <= s < t["first_child"][q] + t["num_children"][q]
        if k:
            assert s < fc and fc + k <= n and (t["parent"][fc:fc + k] == s).all()  # consecutive, in order, above the parent
            assert t["visits"][s] >= t["visits"][fc:fc + k].sum()
            owned[fc:fc + k] += 1
        else:
            assert fc == -1
    assert owned[0] == 0 and (owned[1:] == 1).all()  # every node but the root is the child of exactly one node
    assert (t["parent"][n:] == -1).all() and (t["first_child"][n:] == -1).all() and (t["visits"][n:] == 0).all() and (t["num_children"][n:] == 0).all()
    assert (t["depth"][n:] == 0).all() and (t["node_action"][n:] == 0).all() and (t["prior"][n:] == 0).all() and (t["value_sum"][n:] == 0).all()
    assert np.isneginf(t["value_max"][n:]).all() and (t["terminal"][n:] == 0).all()


@pytest.mark.parametrize("name", list(mc.SHAPES))
def test_choose_is_puct_results_action(name):
    c = mc.case(name)
    ps, _ = mc.searched(name)
    st = mc.run(c.tree, c.C, [mc.call(mc.CHOOSE, mc.GREEDY)])[0]
    again = puct_result(dict(_torch_tree(c.tree), errors_dev=torch.zeros(1, dtype=torch.int32)), c.C)
    for res in (ps, again):
        _same(st, "move_action", res.action)
        _same(st, "child_visits", res.child_visits)
        _same(st, "child_actions", res.child_actions)
        _same(st, "root_value", res.root_value)
    has = c.tree["num_children"][:, 0] > 0
    assert (st["move_slot"][~has] == -1).all() and (st["move_slot"][has] >= 1).all()


def test_the_proportional_pick_is_the_contracts_draw():
    """One fixed root, 4 096 step indices: the model's pick is the Python restatement's every time, each child with visits
    is drawn at least once and no child without visits is."""
    c = mc.case("G16_C16_P35")
    for p in range(c.P):
        k, fc = int(c.tree["num_children"][p, 0]), int(c.tree["first_child"][p, 0])
        visits = c.tree["visits"][p, fc:fc + k]
        if k and (visits == 0).any() and (visits > 0).sum() >= 3:
            break
    else:
        raise AssertionError("no root with visited and unvisited children")
    one = {f: v[p:p + 1] for f, v in c.tree.items()}
    steps = range(1000, 1000 + 4096)
    states = mc.run(one, c.C, [mc.call(mc.CHOOSE, mc.PROPORTIONAL, step_index=s, first_root=p + 5) for s in steps])
    drawn = np.zeros(k, np.int64)
    for s, st in zip(steps, states):
        want = mc.proportional_pick(visits, mc.SEED, p + 5, s)
        assert st["move_slot"][0] == fc + want and st["errors"] == 0
        assert st["move_action"][0].tolist() == c.tree["node_action"][p, fc + want].tolist()
        drawn[want] += 1
    assert ((drawn > 0) == (visits > 0)).all()
    assert abs(drawn[int(np.argmax(visits))] / 4096 - visits.max() / visits.sum()) < 0.05  # and in proportion: a binomial's 6 sigma at most
    spec = puct_choose(_torch_tree(one), c.C, MOVE_PROPORTIONAL, mc.SEED, 1000, p + 5)
    assert int(spec["move_slot"][0]) == int(states[0]["move_slot"][0])
    assert sc.mix64(0) == 0  # the restatement's hash is tests/sampling_contract.py's


def test_three_moves_of_search_choose_reroot_continue():
    P, T, C, K, iterations = 9, 5, 3, 3, 12
    evaluate = pc.synthetic_evaluator(P, T, K, 11)
    root = SimpleNamespace(num_envs=P, device="cpu", cfg=None)
    N = 1 + 3 * iterations * C
    ps = puct_search(root, iterations, 100, evaluate, c_puct=1.25, max_children=C, max_steps=T, capacity=N)
    grown = 0
    for move in range(3):
        tree = search_tree(ps)
        for p in range(P):
            _well_formed({f: tree[f][p].numpy() for f in mc.TREE_FIELDS}, C)
        assert int(ps.errors) == 0
        same, remap = puct_reroot(tree, torch.zeros(P, dtype=torch.int64))  # slot 0: the identity
        for f in mc.TREE_FIELDS:
            assert pc.same_bits(same[f].numpy(), tree[f].numpy()), f
        assert all((remap[p, :int(tree["num_nodes"][p])] == torch.arange(int(tree["num_nodes"][p]))).all() for p in range(P))
        mode = MOVE_PROPORTIONAL if move % 2 else MOVE_GREEDY
        ch = puct_choose(tree, C, mode, mc.SEED, move, 0)
        new, remap = puct_reroot(tree, ch["move_slot"])
        numpy_tree = {f: tree[f].numpy() for f in mc.TREE_FIELDS}
        st = mc.run(numpy_tree, C, [mc.call(mc.CHOOSE | mc.REROOT, mode, step_index=move, first_root=0)])[0]
        for f in mc.TREE_FIELDS:
            _same(st, f, new[f])
        _same(st, "remap", remap)
        before = new["visits"][:, 0].clone()
        ps = puct_search(root, iterations, 100 + (move + 1) * iterations * T, evaluate, c_puct=1.25, max_children=C, max_steps=T, tree=new)
        assert (ps.visits[:, 0] == before + iterations).all()  # the visits below the move were kept, and every evaluation was backed up
        grown += int((before > 0).sum())
    assert grown > 0
    for p in range(P):
        _well_formed({f: search_tree(ps)[f][p].numpy() for f in mc.TREE_FIELDS}, C)


def test_a_continued_search_from_an_empty_tree_is_the_search():
    """tree= changes the loop bounds only: continuing in the tree INIT leaves gives the search that starts from nothing."""
    P, T, C, K, iterations = 7, 5, 3, 3, 16
    evaluate = pc.synthetic_evaluator(P, T, K, 11)
    root = SimpleNamespace(num_envs=P, device="cpu", cfg=None)
    a = puct_search(root, iterations, 100, evaluate, c_puct=1.25, max_children=C, max_steps=T)
    empty, _ = puct_reroot(search_tree(a), torch.full((P,), -1))
    b = puct_search(root, iterations, 100, evaluate, c_puct=1.25, max_children=C, max_steps=T, tree=empty)
    for f in mc.TREE_FIELDS:
        assert pc.same_bits(getattr(a, f).numpy(), getattr(b, f).numpy()), f


# ---- trees the caller has damaged ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.DAMAGE)
def test_a_damaged_tree_is_left_alone(name):
    d = mc.damaged(name)
    c, p, st, healthy = d.case, d.p, d.states[0], d.healthy[0]
    assert 0 < p < c.P - 1 and c.tree["num_children"][p, d.m] >= 2 and healthy["errors"] == 0 and healthy["num_nodes"][p] > 1 + c.C
    before = {f: np.array(c.tree[f]) for f in mc.TREE_FIELDS}
    for f, at, value in d.pokes:
        before[f].reshape(-1)[at] = value
    assert st["errors"] == mc.ERR_TREE
    assert (st["remap"][p] == -1).all()
    for f in mc.TREE_FIELDS:  # the root untouched: what the caller wrote is still there
        assert pc.same_bits(st[f][p], before[f][p].astype(st[f].dtype)), f
    others = [q for q in range(c.P) if q != p]
    for f in mc.TREE_FIELDS + ("remap",):  # the neighbouring roots exact
        assert pc.same_bits(np.take(st[f], others, 0), np.take(healthy[f], others, 0)), f


@pytest.mark.parametrize("shape, name", mc.DEEP_CASES)
def test_a_tree_damaged_in_its_third_span_is_left_alone(shape, name):
    """The damage is found after two spans of ranks are in remap: ERR_TREE, remap all -1, the root and its neighbours as they were."""
    d = mc.damaged_deep(shape, name)
    c, p, st, healthy = d.case, d.p, d.states[0], d.healthy[0]
    keep = mc.subtree(c.tree, p, d.m)
    assert 0 < p < c.P - 1 and 2 * mc.SPAN <= d.s < 3 * mc.SPAN and 2 * mc.SPAN <= d.node < 3 * mc.SPAN and d.s in keep and d.node in keep
    assert sum(s < 2 * mc.SPAN for s in keep) > 0 and c.tree["num_children"][p, d.node] > 0  # kept slots in the spans before: remap held ranks
    assert healthy["errors"] == 0 and healthy["num_nodes"][p] == len(keep) and (healthy["remap"][p, keep] == np.arange(len(keep))).all()
    before = {f: np.array(c.tree[f]) for f in mc.TREE_FIELDS}
    for f, at, value in d.pokes:
        before[f].reshape(-1)[at] = value
    if name == "child_range_not_kept":
        k, fc = int(c.tree["num_children"][p, d.node]), d.pokes[0][2]
        assert 1 <= fc <= d.n - k and not set(range(fc, fc + k)) & set(keep)  # a range of the tree, none of it kept
    assert st["errors"] == mc.ERR_TREE
    assert (st["remap"][p] == -1).all()
    for q in (p - 1, p, p + 1):  # untouched: what the caller wrote is still there
        for f in mc.TREE_FIELDS:
            assert pc.same_bits(st[f][q], before[f][q].astype(st[f].dtype)), (q, f)
    others = [q for q in range(c.P) if q != p]
    for f in mc.TREE_FIELDS + ("remap",):  # every other root as in the healthy call
        assert pc.same_bits(np.take(st[f], others, 0), np.take(healthy[f], others, 0)), f


def test_choose_on_a_damaged_root_addresses_nothing():
    """first_child / num_children of slot 0 out of range: CHOOSE treats the root as one without children and reports bit 1."""
    c = mc.case("G4_C3_P130")
    shp = mc.shapes(c.P, c.N, c.C)
    for f, value in (("first_child", c.N), ("first_child", 0), ("first_child", -(2 ** 31)), ("num_children", c.C + 1), ("num_children", -1),
                     ("num_children", 2 ** 31 - 1), ("first_child", c.N - 1)):
        st = mc.run(c.tree, c.C, [mc.call(mc.CHOOSE, mc.PROPORTIONAL, pokes=[(f, mc.flat(shp[f], 1, 0), value)])])[0]
        assert st["errors"] == mc.ERR_TREE and st["move_slot"][1] == -1 and (st["child_visits"][1] == 0).all() and (st["move_action"][1] == 0).all()
