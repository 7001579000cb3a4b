"""gumbel_search(leaves=L) of pcbenv/search.py on the CPU, where no kernel is involved, on the toy game of
tests/test_gumbel_search.py: that one leaf is today's search, what several leaves spend the budget on, what is chosen when
the launches are too few, the arguments it refuses, and the configuration of the trainer."""
from types import SimpleNamespace

import pytest
import torch

import puct_cases as pc
import puct_leaves_cases as plc
from pcbenv.alphazero import AlphaZeroConfig
from pcbenv.search import gumbel_search, puct_search, puct_selfplay, search_tree

P, T, C, K = 9, 5, 4, 4
ROOT = SimpleNamespace(num_envs=P, device="cpu", cfg=None)
FIELDS = ("visits", "value_sum", "value_max", "prior", "num_children", "first_child", "node_action", "parent", "depth", "terminal", "num_nodes", "reward_lo",
          "reward_hi", "errors")
CHOICE = ("sim_index", "sim_visits", "move_slot", "move_action", "child_weights", "child_policy", "child_actions", "root_value")


def _search(n=8, Mc=4, tree=None, L=None, evaluate=None, **kw):
    if L is not None:
        kw["leaves"] = L
    ev = evaluate or (pc.synthetic_evaluator(P, T, K, 23) if L in (None, 1) else plc.leaves_evaluator(P, T, K, L, 23))
    return gumbel_search(ROOT, n, 100, ev, max_considered=Mc, c_puct=1.25, max_children=C, max_steps=T, tree=tree, seed=5, first_root=0, **kw)


def _bits(t):
    return t.to(torch.float64 if t.is_floating_point() else torch.int64).numpy().tobytes()


def test_one_leaf_is_the_search_of_today():
    calls = []

    def counting(paths, path_len, s):
        calls.append((tuple(paths.shape), int(s)))
        return pc.synthetic_evaluator(P, T, K, 23)(paths, path_len, s)
    a = _search()
    b = _search(L=1, evaluate=counting)
    assert calls == [((T, P, 3), 100 + m * T) for m in range(9)]  # n + 1 launches of P rows
    for f in FIELDS:
        assert _bits(getattr(a.search, f)) == _bits(getattr(b.search, f)), f
    for f in CHOICE:
        assert _bits(getattr(a, f)) == _bits(getattr(b, f)) and getattr(a, f).dtype == getattr(b, f).dtype, f
    # and through the leaf hooks: launches given, the same count
    c = _search(L=1, launches=9)
    for f in CHOICE:
        assert _bits(getattr(a, f)) == _bits(getattr(c, f)), f
    for f in FIELDS:
        assert _bits(getattr(a.search, f)) == _bits(getattr(c.search, f)), f


@pytest.mark.parametrize("L", [2, 3, 4, 8])
def test_several_leaves(L):
    shapes = []

    def watching(paths, path_len, s):
        shapes.append((tuple(paths.shape), tuple(path_len.shape)))
        return plc.leaves_evaluator(P, T, K, L, 23)(paths, path_len, s)
    gs = _search(L=L, evaluate=watching)
    ps = gs.search
    assert shapes == [((T, P * L, 3), (P * L,))] * (-(-8 // L) + 1)  # ceil(n / L) + 1 launches of P * L rows
    live = (ps.num_children[:, 0] > 0) & ~ps.terminal[:, 0]
    assert bool(live.any()) and bool((~live).any()) and int(ps.errors) == 0
    # the budget: never more than n, what was spent went through the root's children, and the counters agree
    assert bool((gs.sim_index <= 8).all()) and bool((gs.sim_index[live] > 0).all()) and bool((gs.sim_index[~live] == 0).all())
    assert torch.equal(gs.sim_visits.sum(dim=1), gs.sim_index.to(torch.int64)) and torch.equal(ps.child_visits[live], gs.sim_visits[live].to(torch.int64))
    assert torch.equal(ps.visits[live, 0], 1 + gs.sim_index[live].to(torch.int64))  # a fresh root: its own evaluation and the simulations
    share = gs.sim_index[live].float().mean().item() / 8
    print(f"L = {L}: share of the budget spent {share:.3f}, roots that finished {(gs.sim_index[live] == 8).float().mean().item():.3f}")
    # the move comes from the children with the most scheduled simulations
    rows = torch.arange(P)[live]
    at = (gs.move_slot[live] - ps.first_child[live, 0]).to(torch.int64)
    assert bool((at >= 0).all()) and bool((gs.sim_visits[rows, at] == gs.sim_visits[live].max(dim=1).values).all())
    assert bool((gs.move_slot[~live] == -1).all()) and not bool(gs.child_weights[~live].any())
    # child_weights sums to 2^24 within the rounding of k entries
    k = ps.num_children[:, 0]
    total = gs.child_weights.to(torch.int64).sum(dim=1)
    assert bool(((total - 2 ** 24).abs() <= k // 2 + 1)[k > 0].all()) and bool((total[k == 0] == 0).all())
    # the same key, the same search; and the search goes on in the kept tree
    again = _search(L=L)
    assert torch.equal(again.sim_visits, gs.sim_visits) and torch.equal(again.child_policy, gs.child_policy)
    kept = _search(L=L, tree=search_tree(ps), gumbel_step_index=101)
    assert bool((kept.sim_index[live] > 0).all()) and bool((kept.search.visits[:, 0] > ps.visits[:, 0])[live].all())


def test_too_few_launches_still_choose():
    gs = _search(L=2, launches=3)  # at most 2 * 2 of the 8 simulations: evaluation 0 expands the root
    ps = gs.search
    live = (ps.num_children[:, 0] > 0) & ~ps.terminal[:, 0]
    assert bool(live.any()) and bool((gs.sim_index[live] <= 4).all()) and bool((gs.sim_index[live] > 0).all())
    at = (gs.move_slot[live] - ps.first_child[live, 0]).to(torch.int64)
    assert bool((gs.sim_visits[torch.arange(P)[live], at] == gs.sim_visits[live].max(dim=1).values).all())
    k = ps.num_children[:, 0]
    assert bool(((gs.child_weights.to(torch.int64).sum(dim=1) - 2 ** 24).abs() <= k // 2 + 1)[k > 0].all())


def test_arguments():
    for bad in (dict(L=0), dict(L=65), dict(L=2, launches=0)):
        with pytest.raises(ValueError):
            _search(**bad)
    ev = pc.synthetic_evaluator(P, T, K, 23)
    with pytest.raises(ValueError):  # a root rule with a budget needs both leaf hooks
        puct_search(ROOT, 4, 0, ev, max_children=C, max_steps=T, leaves=2, root_select=lambda tree, stopped, nxt: nxt, leaf_begin=lambda l, tree, alive: alive)
    # hooks that do nothing leave puct_search(leaves=L) as it is
    lev = lambda: plc.leaves_evaluator(P, T, K, 3, 23)
    a = puct_search(ROOT, 5, 100, lev(), c_puct=1.25, max_children=C, max_steps=T, leaves=3)
    b = puct_search(ROOT, 5, 100, lev(), c_puct=1.25, max_children=C, max_steps=T, leaves=3, root_select=lambda tree, stopped, nxt: nxt,
                    leaf_begin=lambda l, tree, alive: alive, leaf_end=lambda l, alive: None)
    for f in FIELDS:
        assert _bits(getattr(a, f)) == _bits(getattr(b, f)), f
    root = SimpleNamespace(num_envs=P, device="cpu", cfg=None, run_seed=1)
    with pytest.raises(ValueError):
        puct_selfplay(root, None, 1, 4, max_steps=T, gumbel=(4, 50.0, 1.0), leaves=2)  # nothing to call
    with pytest.raises(ValueError):
        puct_selfplay(root, ev, 1, 4, max_steps=T, gumbel=(4, 50.0, 1.0), leaves=2, root_noise=(0.3, 0.25))
    cfg = AlphaZeroConfig(gumbel_considered=4, leaves=4)
    assert (cfg.gumbel_considered, cfg.leaves) == (4, 4)
