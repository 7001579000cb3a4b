"""node_rule="gumbel" in pcbenv/search.py on the CPU, where no kernel is involved: what the new arguments change and what they
leave alone.  Without node_rule and pending= every function returns the objects it returned; node_rule="gumbel" with one leaf is
full=True bit for bit; c_puct is not read; with several leaves the budget is kept, nothing is pending when a move is made, and a
pending visit moves the next descent of a node; the arguments that are refused; the configuration of the trainer."""
from types import SimpleNamespace

import pytest
import torch

import puct_cases as pc
import puct_leaves_cases as plc
from pcbenv.alphazero import AlphaZeroConfig
from pcbenv.search import (gumbel_node_scores, gumbel_search, gumbel_search_device, gumbel_select_node, puct_reroot, puct_search, puct_selfplay,
                           search_tree)

P, T, K, C, n, Mc = 7, 5, 4, 4, 8, 4
ROOT = SimpleNamespace(num_envs=P, device="cpu", cfg=None)
KW = dict(max_considered=Mc, c_visit=50.0, c_scale=1.0, c_puct=1.25, max_children=C, max_steps=T, seed=77, first_root=3)
FIELDS = ("sim_index", "sim_visits", "move_slot", "move_action", "child_weights", "child_policy", "child_actions", "root_value")
TREE = ("num_nodes", "parent", "depth", "visits", "num_children", "first_child", "node_action", "prior", "value_sum", "value_max", "terminal", "reward_lo",
        "reward_hi", "errors")


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes()


def _assert_same(a, b):
    for f in FIELDS:
        assert _same(getattr(a, f), getattr(b, f)), f
    for f in TREE:
        assert _same(getattr(a.search, f), getattr(b.search, f)), f


def _search(L=1, **kw):
    ev = pc.synthetic_evaluator(P, T, K, 41) if L == 1 else plc.leaves_evaluator(P, T, K, L, 41)
    return gumbel_search(ROOT, n, 100, ev, **dict(KW, **kw), **({} if L == 1 else dict(leaves=L)))


def test_without_the_new_arguments_every_function_returns_what_it_returned():
    for L in (1, 3):
        _assert_same(_search(L), _search(L, node_rule="puct"))
    _assert_same(_search(full=True), _search(full=True, node_rule="puct"))
    tree = search_tree(_search(full=True).search)
    node = tree["first_child"][:, 0].clamp(min=0).long()
    a, b = gumbel_node_scores(tree, node, C, 50.0, 1.0), gumbel_node_scores(tree, node, C, 50.0, 1.0, pending=None)
    assert set(a) == set(b) == {"k", "fc", "ok", "mine", "n", "Nsum", "vhat", "vmix", "logit", "qhat", "sigma", "x", "pi", "t"}
    assert all(_same(a[f], b[f]) for f in a)
    a, b = gumbel_select_node(tree, node, C, 50.0, 1.0), gumbel_select_node(tree, node, C, 50.0, 1.0, pending=None)
    assert set(a) == set(b) == {"child", "ok", "errors"} and all(_same(a[f], b[f]) for f in a)
    # pending all zero: the same child, t with the same bits wherever it is a number
    zero = torch.zeros_like(tree["visits"])
    z = gumbel_node_scores(tree, node, C, 50.0, 1.0, pending=zero)
    plain = gumbel_node_scores(tree, node, C, 50.0, 1.0)
    assert _same(z["t"], plain["t"]) and _same(z["Msum"], plain["Nsum"]) and _same(z["m"], plain["n"]) and all(_same(z[f], plain[f]) for f in plain)
    # a hook of puct_search that says PUCT is no hook, with one leaf and with several
    for L, ev in ((1, pc.synthetic_evaluator(P, T, K, 43)), (3, plc.leaves_evaluator(P, T, K, 3, 43))):
        seen = []
        a = puct_search(ROOT, 5, 5, ev, c_puct=1.25, max_children=C, max_steps=T, leaves=L)
        b = puct_search(ROOT, 5, 5, ev, c_puct=1.25, max_children=C, max_steps=T, leaves=L,
                        pending_select=lambda d, tree, node, stopped, nxt: seen.append(tuple(tree["pending"].shape)) or nxt)
        for f in TREE:
            assert _same(getattr(a, f), getattr(b, f)), f
        assert seen and set(seen) == {tuple(a.visits.shape)}  # the hook is handed pending [P, N]


def test_one_leaf_is_full():
    full, rule = _search(full=True), _search(node_rule="gumbel")
    _assert_same(full, rule)
    _assert_same(full, _search(full=True, node_rule="gumbel"))
    assert not all(_same(getattr(_search().search, f), getattr(rule.search, f)) for f in TREE)  # and another search than PUCT's below the root
    # through the leaf loop with L = 1 (launches given): the same search again
    _assert_same(full, _search(node_rule="gumbel", launches=n + 1))
    # and in a kept tree
    tree, _ = puct_reroot(search_tree(full.search), full.move_slot)
    _assert_same(_search(full=True, tree=tree, gumbel_step_index=101), _search(node_rule="gumbel", tree=tree, gumbel_step_index=101))


@pytest.mark.parametrize("L", [1, 4])
def test_c_puct_is_not_read(L):
    _assert_same(_search(L, node_rule="gumbel"), _search(L, node_rule="gumbel", c_puct=7.5))


@pytest.mark.parametrize("L", [2, 3, 4, 8])
def test_several_leaves_keep_the_budget_and_leave_nothing_pending(L):
    """puct_search's own `pending` is local to it; its hook sees it.  Before the first descent of every iteration -- a move is
    made behind the last one's ABSORB -- nothing is pending; within an iteration the pending visits are those of the leaves so far.
    (Iteration 0 of a fresh tree finds no level to descend: the rule is asked in the E - 1 others.)"""
    shapes, at_first, later = [], [], []

    def watching(paths, path_len, s):
        shapes.append((tuple(paths.shape), tuple(path_len.shape)))
        return plc.leaves_evaluator(P, T, K, L, 41)(paths, path_len, s)
    real = gumbel_select_node

    def spy(tree, node, max_children, c_visit, c_scale, pending=None):
        (at_first if not bool(pending.any()) else later).append(int(pending.sum()))
        return real(tree, node, max_children, c_visit, c_scale, pending)
    import pcbenv.search as search
    search.gumbel_select_node = spy
    try:
        gs = gumbel_search(ROOT, n, 100, watching, leaves=L, node_rule="gumbel", **KW)
    finally:
        search.gumbel_select_node = real
    E = -(-n // L) + 1
    assert shapes == [((T, P * L, 3), (P * L,))] * E and len(at_first) == E - 1 and later and min(later) >= 1
    ps = gs.search
    live = (ps.num_children[:, 0] > 0) & ~ps.terminal[:, 0]
    assert bool(live.any()) and int(ps.errors) == 0
    assert bool((gs.sim_index <= n).all()) and bool((gs.sim_index[live] > 0).all()) and bool((gs.sim_index[~live] == 0).all())
    assert torch.equal(gs.sim_visits.sum(dim=1), gs.sim_index.to(torch.int64)) and torch.equal(ps.child_visits[live], gs.sim_visits[live].to(torch.int64))
    assert torch.equal(ps.visits[live, 0], 1 + gs.sim_index[live].to(torch.int64))  # every pending visit came back as a visit: none is left
    k = ps.num_children[:, 0]
    total = gs.child_weights.to(torch.int64).sum(dim=1)
    assert bool(((total - 2 ** 24).abs() <= k // 2 + 1)[k > 0].all()) and bool((total[k == 0] == 0).all())
    again = gumbel_search(ROOT, n, 100, plc.leaves_evaluator(P, T, K, L, 41), leaves=L, node_rule="gumbel", **KW)
    _assert_same(gs, again)
    tree = puct_reroot(search_tree(ps), gs.move_slot)[0]
    kept = gumbel_search(ROOT, n, 200, plc.leaves_evaluator(P, T, K, L, 43), leaves=L, node_rule="gumbel", tree=tree, gumbel_step_index=101, **KW)
    goes_on = (tree["num_children"][:, 0] > 0) & ~tree["terminal"][:, 0].bool()  # the move's child had been expanded
    assert bool(goes_on.any()) and bool((kept.sim_index[goes_on] > 0).all())


def test_a_pending_visit_moves_the_next_descent():
    """A node with two children of equal priors and no value range: pi = (1/2, 1/2) exactly.  Nothing pending: t = (1/2, 1/2), the
    lower child.  One pending visit on child 0: t = (1/2 - 1/2, 1/2), child 1 -- and nothing else of the scores has moved."""
    f64 = torch.float64
    tree = dict(num_children=torch.tensor([[2, 0, 0]]), first_child=torch.tensor([[1, -1, -1]]), visits=torch.tensor([[1, 0, 0]]),
                prior=torch.tensor([[0.0, 0.5, 0.5]], dtype=f64), value_sum=torch.tensor([[0.5, 0.0, 0.0]], dtype=f64), terminal=torch.zeros((1, 3), dtype=torch.bool),
                reward_lo=torch.tensor([0.5], dtype=f64), reward_hi=torch.tensor([0.5], dtype=f64))
    node = torch.zeros(1, dtype=torch.int64)
    none, one = torch.tensor([[0, 0, 0]]), torch.tensor([[5, 1, 0]])  # pending of the node itself is not read
    a, b = gumbel_node_scores(tree, node, 2, 50.0, 1.0, none), gumbel_node_scores(tree, node, 2, 50.0, 1.0, one)
    assert a["pi"][0].tolist() == [0.5, 0.5] and a["t"][0].tolist() == [0.5, 0.5] and b["t"][0].tolist() == [0.0, 0.5]
    assert b["m"][0].tolist() == [1, 0] and int(b["Msum"][0]) == 1
    assert all(_same(a[f], b[f]) for f in ("n", "Nsum", "vhat", "vmix", "logit", "qhat", "sigma", "x", "pi"))
    assert int(gumbel_select_node(tree, node, 2, 50.0, 1.0, none)["child"][0]) == 0 and int(gumbel_select_node(tree, node, 2, 50.0, 1.0, one)["child"][0]) == 1
    assert int(gumbel_select_node(tree, node, 2, 50.0, 1.0)["child"][0]) == 0


def test_arguments():
    ev = pc.synthetic_evaluator(P, T, K, 41)
    for bad in (dict(node_rule="uct"), dict(node_rule=None), dict(node_rule="gumbel", leaves=0), dict(node_rule="gumbel", leaves=65),
                dict(node_rule="gumbel", leaves=2, launches=0), dict(node_rule="gumbel", full=True, leaves=2)):  # full=True keeps its refusal
        with pytest.raises(ValueError):
            gumbel_search(ROOT, n, 100, ev, **KW, **bad)
        with pytest.raises(ValueError):  # refused before the root is asked for a device
            gumbel_search_device(ROOT, n, 100, ev, max_considered=Mc, max_children=C, max_steps=T, seed=77, **bad)
    root = SimpleNamespace(num_envs=P, device="cpu", cfg=None, run_seed=1)
    for bad in (dict(gumbel_node_rule="gumbel"), dict(gumbel_node_rule="uct", gumbel=(4, 50.0, 1.0)), dict(gumbel_node_rule="gumbel", gumbel=(4, 50.0, 1.0), leaves=2, root_noise=(0.3, 0.25)),
                dict(gumbel_node_rule="gumbel", gumbel_full=True, gumbel=(4, 50.0, 1.0), leaves=2)):
        with pytest.raises(ValueError):
            puct_selfplay(root, ev, 1, 4, max_steps=T, **bad)
    cfg = AlphaZeroConfig(gumbel_considered=4, leaves=4, gumbel_node_rule="gumbel")
    assert (cfg.gumbel_considered, cfg.leaves, cfg.gumbel_node_rule, cfg.gumbel_full) == (4, 4, "gumbel", False) and AlphaZeroConfig().gumbel_node_rule == "puct"
