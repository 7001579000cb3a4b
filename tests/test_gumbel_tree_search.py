"""The full Gumbel rule in pcbenv/search.py on the CPU: what the new arguments change and what they leave alone.  Without
full= every function gives the objects it gave; full=True with leaves > 1 or launches= is refused; the per-level hook of
puct_search defaults to PUCT; and a better value of a child raises its pi' at a node below the root."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import puct_cases as pc
from pcbenv.search import (gumbel_choose, gumbel_node_scores, gumbel_search, gumbel_search_device, gumbel_select_node, puct_search,
                           puct_selfplay, search_tree)

P, T, K, C, n, Mc = 7, 5, 4, 4, 8, 4
ROOT = SimpleNamespace(num_envs=P, device="cpu", cfg=None)
KW = dict(max_considered=Mc, c_visit=50.0, c_scale=1.0, c_puct=1.25, max_children=C, max_steps=T, seed=77, first_root=3)
FIELDS = ("sim_index", "sim_visits", "move_slot", "move_action", "child_weights", "child_policy", "child_actions", "root_value")
TREE = ("num_nodes", "parent", "depth", "visits", "num_children", "first_child", "node_action", "prior", "value_sum", "value_max", "terminal")


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes()


def _search(**kw):
    return gumbel_search(ROOT, n, 100, pc.synthetic_evaluator(P, T, K, 41), **KW, **kw)


def test_without_full_every_search_is_what_it_was():
    plain, off, on = _search(), _search(full=False), _search(full=True)
    for f in FIELDS:
        assert _same(getattr(plain, f), getattr(off, f)), f
    for f in TREE:
        assert _same(getattr(plain.search, f), getattr(off.search, f)), f
    assert not all(_same(getattr(plain.search, f), getattr(on.search, f)) for f in TREE)  # the other rule is another search
    # the hook of puct_search that says PUCT is no hook
    ev = pc.synthetic_evaluator(P, T, K, 43)
    a = puct_search(ROOT, 9, 5, ev, c_puct=1.25, max_children=C, max_steps=T)
    b = puct_search(ROOT, 9, 5, ev, c_puct=1.25, max_children=C, max_steps=T, level_select=lambda d, tree, node, stopped, nxt: nxt)
    for f in TREE:
        assert _same(getattr(a, f), getattr(b, f)), f
    seen = []
    puct_search(ROOT, 3, 5, ev, c_puct=1.25, max_children=C, max_steps=T, level_select=lambda d, tree, node, stopped, nxt: seen.append(d) or nxt)
    assert seen == [0, 0, 1]  # iteration m of a fresh tree finds no node deeper than m


def test_full_does_not_go_with_leaves():
    ev = pc.synthetic_evaluator(P, T, K, 41)
    for kw in (dict(leaves=2), dict(launches=3), dict(leaves=4, launches=2)):
        with pytest.raises(ValueError):
            gumbel_search(ROOT, n, 100, ev, full=True, **KW, **kw)
        with pytest.raises(ValueError):  # refused before the root is asked for a device
            gumbel_search_device(ROOT, n, 100, ev, full=True, max_considered=Mc, max_children=C, max_steps=T, seed=77, **kw)
    with pytest.raises(ValueError):
        puct_search(ROOT, 3, 5, ev, max_children=C, max_steps=T, leaves=2, level_select=lambda d, tree, node, stopped, nxt: nxt)
    for kw in (dict(gumbel=None), dict(gumbel=(4, 50.0, 1.0), leaves=2)):
        with pytest.raises(ValueError):
            puct_selfplay(ROOT, ev, 1, n, gumbel_full=True, **kw)


def test_c_puct_is_not_read():
    a, b = _search(full=True), gumbel_search(ROOT, n, 100, pc.synthetic_evaluator(P, T, K, 41), full=True, **dict(KW, c_puct=7.5))
    for f in FIELDS:
        assert _same(getattr(a, f), getattr(b, f)), f
    for f in TREE:
        assert _same(getattr(a.search, f), getattr(b.search, f)), f


def test_a_better_value_raises_the_policy_of_a_node_below_the_root():
    gs = _search(full=True)
    tree = search_tree(gs.search)
    nch, fc, visits = tree["num_children"].long(), tree["first_child"].long(), tree["visits"].long()
    found = 0
    for p in range(P):
        for a in range(1, int(tree["num_nodes"][p])):
            k, f = int(nch[p, a]), int(fc[p, a])
            seen = [j for j in range(k) if visits[p, f + j] > 0]
            if k < 2 or not seen or not float(tree["reward_hi"][p]) > float(tree["reward_lo"][p]):
                continue
            node = torch.zeros(P, dtype=torch.int64)
            node[p] = a
            base = gumbel_node_scores(tree, node, C, 50.0, 1.0)["pi"][p]
            more = dict(tree, value_sum=tree["value_sum"].clone())
            more["value_sum"][p, f + seen[0]] += 0.05
            up = gumbel_node_scores(more, node, C, 50.0, 1.0)["pi"][p]
            # the other children may move either way: the value also enters vmix, which completes those without a visit
            assert up[seen[0]] >= base[seen[0]] and abs(float(up[:k].sum()) - 1.0) < 1e-12, (p, a)
            if float(base[seen[0]]) < 0.99:  # a policy already at 1 has nowhere to rise to
                assert up[seen[0]] > base[seen[0]], (p, a)
                found += 1
    assert found >= 3


def test_the_rule_reads_the_root_through_the_node_scores():
    gs = _search(full=True)
    tree = search_tree(gs.search)
    at_root = gumbel_node_scores(tree, torch.zeros(P, dtype=torch.int64), C, 50.0, 1.0)
    ch = gumbel_choose(tree, gs.sim_visits, C, 50.0, 1.0, 77, 100, 3, full=True)
    assert _same(ch["child_policy"], at_root["pi"].to(torch.float32)) and _same(ch["child_policy"], gs.child_policy)
    sel = gumbel_select_node(tree, torch.zeros(P, dtype=torch.int64), C, 50.0, 1.0)
    ok = at_root["ok"]
    assert bool(ok.any()) and np.array_equal(sel["child"][ok].numpy(), at_root["t"][ok].argmax(dim=1).numpy()) and int(sel["errors"]) == 0
