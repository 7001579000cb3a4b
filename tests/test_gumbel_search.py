"""The Gumbel search of pcbenv/search.py on the CPU, where no kernel is involved: what gumbel_search spends its evaluations
on, that it leaves puct_search alone, the arguments it refuses, and the configuration of the trainer."""
from types import SimpleNamespace

import pytest
import torch

import puct_cases as pc
from pcbenv.alphazero import AlphaZeroConfig
from pcbenv.search import (GUMBEL_ABSORB, GUMBEL_BEGIN, GUMBEL_CHOOSE, GUMBEL_SELECT, considered_visits, gumbel_scores, gumbel_search, new_gumbel_tensors,
                           new_puct_tree, puct_search, puct_selfplay, search_tree)

P, T, C, K = 9, 5, 4, 4
ROOT = SimpleNamespace(num_envs=P, device="cpu", cfg=None)


def _search(n=8, Mc=4, tree=None, **kw):
    return gumbel_search(ROOT, n, 100, pc.synthetic_evaluator(P, T, K, 23), max_considered=Mc, c_puct=1.25, max_children=C, max_steps=T, tree=tree, seed=5,
                         first_root=0, **kw)


def test_the_budget_of_a_fresh_and_of_a_kept_root():
    gs = _search()
    ps = gs.search
    live = (ps.num_children[:, 0] > 0) & ~ps.terminal[:, 0]
    assert bool(live.any()) and bool((~live).any()) and int(ps.errors) == 0
    # a fresh root: evaluation 0 expands it, then n scheduled simulations, all of them through a child of the root
    assert bool((gs.sim_index[live] == 8).all()) and bool((gs.sim_visits[live].sum(dim=1) == 8).all()) and bool((ps.visits[live, 0] == 9).all())
    assert bool((gs.sim_index[~live] == 0).all()) and bool((gs.sim_visits[~live] == 0).all())
    assert torch.equal(ps.child_visits[live], gs.sim_visits[live].to(torch.int64))  # in a fresh tree the two counters agree
    # Sequential Halving over 4 candidates and 8 simulations: 0 0 0 0 1 1 2 2
    full = live & (ps.num_children[:, 0] == 4)
    assert bool(full.any()) and all(sorted(row) == [1, 1, 3, 3] for row in gs.sim_visits[full].tolist())
    # the move is one of the most-simulated children
    rows = torch.arange(P)[live]
    at = (gs.move_slot[live] - ps.first_child[live, 0]).to(torch.int64)
    assert bool((gs.sim_visits[rows, at] == gs.sim_visits[live].max(dim=1).values).all())
    assert bool((gs.move_slot[~live] == -1).all()) and not bool(gs.child_weights[~live].any())
    # the same key, the same search; another key, another one
    again, other = _search(), _search(gumbel_step_index=101)
    assert torch.equal(again.sim_visits, gs.sim_visits) and torch.equal(again.child_policy, gs.child_policy)
    assert not torch.equal(other.sim_visits, gs.sim_visits)
    # a kept tree: n scheduled simulations and one PUCT descent
    kept = _search(tree=search_tree(ps), gumbel_step_index=101)
    assert bool((kept.sim_index[live] == 8).all()) and bool((kept.search.visits[live, 0] == 9 + 9).all())


def test_puct_search_is_what_it_was():
    ev = lambda: pc.synthetic_evaluator(P, T, K, 23)
    a = puct_search(ROOT, 9, 100, ev(), c_puct=1.25, max_children=C, max_steps=T)
    b = puct_search(ROOT, 9, 100, ev(), c_puct=1.25, max_children=C, max_steps=T, root_select=lambda tree, stopped, nxt: nxt)
    for f in ("visits", "value_sum", "prior", "num_children", "first_child", "node_action", "parent"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert not torch.equal(_search().search.visits, a.visits)  # and the Gumbel rule is another search
    with pytest.raises(ValueError):
        puct_search(ROOT, 4, 0, ev(), max_children=C, max_steps=T, leaves=2, root_select=lambda tree, stopped, nxt: nxt)


def test_arguments():
    assert (GUMBEL_BEGIN, GUMBEL_ABSORB, GUMBEL_SELECT, GUMBEL_CHOOSE) == (1, 2, 4, 8)
    for bad in ((0, 4), (65, 4), (4, 0)):
        with pytest.raises(ValueError):
            considered_visits(*bad)
    with pytest.raises(ValueError):
        _search(n=0)
    with pytest.raises(ValueError):
        _search(Mc=65)
    tree = search_tree(_search().search)
    for bad in (dict(c_visit=-1.0), dict(c_scale=float("nan")), dict(c_visit=float("inf"))):
        with pytest.raises(ValueError):
            gumbel_scores(tree, C, **{**dict(c_visit=50.0, c_scale=1.0, seed=1, step_index=0), **bad})
    with pytest.raises(ValueError):
        gumbel_search(ROOT, 4, 0, None, max_children=C, max_steps=T)  # no run_seed, no seed
    root = SimpleNamespace(num_envs=P, device="cpu", cfg=None, run_seed=1)
    with pytest.raises(ValueError):
        puct_selfplay(root, None, 1, 4, max_steps=T, gumbel=(4, 50.0, 1.0), root_noise=(0.3, 0.25))
    with pytest.raises(ValueError):
        puct_selfplay(root, None, 1, 4, max_steps=T, gumbel=(4, 50.0, 1.0), leaves=2)
    t = new_gumbel_tensors(3, 8, 4, 16, "cpu")
    assert t["considered"].shape == (5, 16) and t["sim_visits"].shape == (3, 8) and t["child_policy"].dtype == torch.float32
    assert t["child_weights"].dtype == t["sim_index"].dtype == torch.int32 and t["root_value"].dtype == torch.float64
    assert "sim_index" not in new_puct_tree(3, 4, 2, "cpu")  # new_puct_tree stays as it is
    cfg = AlphaZeroConfig()
    assert (cfg.gumbel_considered, cfg.gumbel_c_visit, cfg.gumbel_c_scale) == (None, 50.0, 1.0)
