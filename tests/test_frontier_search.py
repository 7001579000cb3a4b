"""pcbenv.search.frontier_search on the CPU: the beam search over placements on its specification, against searches
written as plain Python loops over the same synthetic evaluator (tests/puct_cases.py:synthetic_evaluator, a function of
(root, path): row p * F + i of a frontier is told what root p is told of that path).

  exhaustive   with W * K >= K^T nothing is ever cut: best_value is the maximum over all finished paths and best_path the
               first such path in the rule's order (by depth, then by slot).
  greedy       W = 1 is the walk along the best-valued child.
  log-prior    a constant value with prior_weight = 1 orders by the cumulative log-prior, in Python floats with ieee_ln
               restated.
And the loop makes no host synchronisation, refuses what it must before it allocates, and leaves the other searches of the
module as they were."""
import math
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gumbel_cases as gc
import puct_cases as pc
import puct_leaves_cases as lc
from pcbenv import search
from pcbenv.search import Evaluation, frontier_search

SEED = 31


def node_of(base, P, T, p, path):
    """What the P-row evaluator `base` says of the node `path` (a tuple of actions) of root p: (value, terminal, count, actions, priors)."""
    paths, path_len = torch.zeros((T, P, 3), dtype=torch.int32), torch.zeros(P, dtype=torch.int32)
    for d, a in enumerate(path):
        paths[d, p] = torch.tensor(a, dtype=torch.int32)
    path_len[p] = len(path)
    ev = base(paths, path_len, 0)
    return float(ev.value[p]), bool(ev.terminal[p]), int(ev.cand_count[p]), [tuple(a) for a in ev.cand_actions[p].tolist()], [float(x) for x in ev.cand_prior[p]]


def walk(base, P, T, K, W, p, score=lambda value, cum: value, ln=None, depths=None):
    """The rule as a loop over lists, one root: -> (best (value, path) or None, the frontiers by depth as lists of (path, cum))."""
    frontier, best, seen = [((), 0.0)], None, []
    for d in range(T + 1 if depths is None else depths):
        seen.append(frontier)
        nodes = [node_of(base, P, T, p, path) for path, _ in frontier]
        for (path, _), (v, over, _, _, _) in zip(frontier, nodes):
            if over and (best is None or v > best[0]):
                best = (v, path)
        rank = sorted((-score(v, cum), i) for i, ((_, cum), (v, over, k, _, _)) in enumerate(zip(frontier, nodes)) if not over and d < T and min(max(k, 0), K) > 0)
        frontier = [(frontier[i][0] + (nodes[i][3][c],), frontier[i][1] + (ln(nodes[i][4][c]) if ln else 0.0)) for _, i in rank[:W] for c in range(min(nodes[i][2], K))]
    return best, seen


def run(P, W, K, T, prior_weight=0.0, base=None, depth=None):
    base = base or pc.synthetic_evaluator(P, T, K, SEED)
    root = SimpleNamespace(num_envs=P, device="cpu", cfg=None)
    return frontier_search(root, lc.per_leaf(base, P, T, K, W * K), W, K, 100, prior_weight=prior_weight, max_steps=T, depth=depth), base


def check_best(fs, p, best):
    if best is None:
        assert fs.best_len[p] == -1 and fs.best_value[p] == float("-inf") and fs.action[p].tolist() == [0, 0, 0]
        return
    v, path = best
    assert float(fs.best_value[p]) == v and int(fs.best_len[p]) == len(path)
    assert [tuple(a) for a in fs.best_path[:len(path), p].tolist()] == list(path)
    assert fs.action[p].tolist() == (list(path[0]) if path else [0, 0, 0])


def test_a_frontier_that_holds_every_path_finds_the_best_one():
    P, W, K, T = 14, 9, 3, 3
    assert W * K >= K ** T
    fs, base = run(P, W, K, T)
    finished = 0
    for p in range(P):
        best, seen = walk(base, P, T, K, 10 ** 6, p)  # no cut at all
        assert all(sum(1 for path, _ in f) <= W * K for f in seen)
        every = [(node_of(base, P, T, p, path)[0], d, i, path) for d, f in enumerate(seen) for i, (path, _) in enumerate(f) if node_of(base, P, T, p, path)[1]]
        finished += len(every)
        if every:
            top = max(v for v, _, _, _ in every)
            first = min((d, i, path) for v, d, i, path in every if v == top)  # the rule's order: by depth, then by slot
            assert best == (top, first[2])
        check_best(fs, p, best)
    assert finished > 3 * P and int(fs.errors) == 0
    assert fs.best_len[6] == 0 and fs.best_len[5] == -1 and (fs.best_len[[0, 1, 2, 3, 4]] >= 1).all()  # terminal at the root; never a candidate
    assert (fs.live == 0).all() and (fs.path_len == -1).all()  # T + 1 depths: nothing is left


def test_width_one_is_the_greedy_walk():
    P, K, T = 14, 4, 5
    fs, base = run(P, 1, K, T)
    for p in range(P):
        children, best = [()], None
        for d in range(T + 1):  # the ten-line loop: the finals among the children are recorded, the walk goes on from the best-valued of the others
            nodes = [node_of(base, P, T, p, path) for path in children]
            for path, (v, over, _, _, _) in zip(children, nodes):
                if over and (best is None or v > best[0]):
                    best = (v, path)
            on = [i for i, (v, over, k, _, _) in enumerate(nodes) if not over and d < T and min(k, K) > 0]
            if not on:
                break
            i = max(on, key=lambda i: (nodes[i][0], -i))  # the first of equals
            children = [children[i] + (a,) for a in nodes[i][3][:min(nodes[i][2], K)]]
        check_best(fs, p, best)
    assert (fs.best_len >= 2).sum() >= 3


def py_ln(x):
    """csrc/pcb_ieee_math.h:ieee_ln in Python floats, operation by operation."""
    m, e = math.frexp(x)
    if m < 7.07106781186547524401e-01:
        m, e = 2.0 * m, e - 1
    t = (m - 1.0) / (m + 1.0)
    t2 = t * t
    p = 1.0 / 27.0
    for n in (25.0, 23.0, 21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0, 1.0):
        p = p * t2 + 1.0 / n
    return e * 6.93147180369123816490e-01 + (e * 1.90821492927058770002e-10 + (2.0 * t) * p)


def test_a_constant_value_and_weight_one_order_by_the_cumulative_log_prior():
    P, W, K, T = 10, 2, 3, 4
    plain = pc.real_evaluator(P, T, K, SEED)  # softmax priors: no two sums of logarithms alike

    def base(paths, path_len, s):
        ev = plain(paths, path_len, s)
        prior = ev.cand_prior.clone()
        prior[prior < 1e-30] = 0.25  # the zero and the denormal of every seventh node: here every prior has a logarithm
        return Evaluation(torch.full_like(ev.value, 0.5), ev.terminal, ev.cand_count, ev.cand_actions, prior)
    depth = 3
    fs, _ = run(P, W, K, T, prior_weight=1.0, base=base, depth=depth)
    rows = 0
    for p in range(P):
        best, seen = walk(base, P, T, K, W, p, score=lambda value, cum: value + 1.0 * cum, ln=py_ln, depths=depth)
        check_best(fs, p, best)
        nodes = [node_of(base, P, T, p, path) for path, _ in seen[depth - 1]]
        rank = sorted((-(v + 1.0 * cum), i) for i, ((_, cum), (v, over, k, _, _)) in enumerate(zip(seen[depth - 1], nodes)) if not over and k > 0)
        want = [(seen[depth - 1][i][0] + (nodes[i][3][c],), seen[depth - 1][i][1] + py_ln(nodes[i][4][c]), w * K + c)
                for w, (_, i) in enumerate(rank[:W]) for c in range(min(nodes[i][2], K))]
        got_len, got_cum = fs.path_len.view(P, W * K)[p], fs.cum_logp.view(P, W * K)[p]
        assert int(fs.live[p]) == len(want) == int((got_len >= 0).sum())
        for path, cum, slot in want:
            assert int(got_len[slot]) == len(path) == depth and float(got_cum[slot]) == cum  # the same bits: the same operations
            assert [tuple(a) for a in fs.paths[:depth, p * W * K + slot].tolist()] == list(path)
            assert abs(cum - sum(math.log(float(np.float32(x))) for x in _priors_along(base, P, T, p, path))) < 1e-12
        rows += len(want)
    assert rows > 2 * P


def _priors_along(base, P, T, p, path):
    out = []
    for d in range(len(path)):
        _, _, _, actions, priors = node_of(base, P, T, p, path[:d])
        out.append(priors[actions.index(path[d])])
    return out


def tensor_evaluator(P, F, K, T):
    """An evaluator in tensor code alone: the value is a hash of the path, a row is final at T, or by its last action."""
    def evaluate(paths, path_len, step_index0):
        R = P * F
        assert tuple(paths.shape) == (T, R, 3) and tuple(path_len.shape) == (R,) and path_len.dtype == torch.int32
        on = torch.arange(T)[:, None] < path_len[None, :]
        h = torch.where(on, paths[:, :, 2].to(torch.int64) * (torch.arange(T)[:, None] + 3) + 1, 0).sum(dim=0) + torch.arange(R) // F
        value = ((h * 7919) % 13).to(torch.float64) / 16.0
        over = (path_len == T) | ((path_len > 1) & (h % 5 == 0))
        actions = torch.zeros((R, K, 3), dtype=torch.int32)
        actions[:, :, 2] = torch.arange(K, dtype=torch.int32)
        prior = torch.full((R, K), 1.0 / K, dtype=torch.float32)
        return Evaluation(value, over.to(torch.uint8), torch.full((R,), K, dtype=torch.int32), actions, prior)
    return evaluate


def test_nothing_synchronises_inside_the_loop(monkeypatch):
    """No .item(), .cpu(), .tolist(), .numpy(), nonzero() or bool(tensor) while the search runs (each would be a host
    synchronisation on a device)."""
    P, W, K, T = 5, 3, 4, 4
    root = SimpleNamespace(num_envs=P, device="cpu", cfg=None)
    want = frontier_search(root, tensor_evaluator(P, W * K, K, T), W, K, 0, prior_weight=0.5, max_steps=T)

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"frontier_search called Tensor.{name}")
        return f
    for name in ("item", "cpu", "tolist", "numpy", "nonzero", "__bool__", "__int__", "__float__", "__index__"):
        monkeypatch.setattr(torch.Tensor, name, refuse(name))
    fs = frontier_search(root, tensor_evaluator(P, W * K, K, T), W, K, 0, prior_weight=0.5, max_steps=T)
    monkeypatch.undo()
    assert (fs.best_len >= 1).all() and torch.equal(fs.best_path, want.best_path) and torch.equal(fs.best_value, want.best_value)
    assert fs.action.tolist() == fs.best_path[0].tolist()


def test_the_calls_it_refuses(monkeypatch):
    root = SimpleNamespace(num_envs=2, device="cpu", cfg=None)
    ev = tensor_evaluator(2, 6, 3, 4)

    def no_tensors(*a, **k):
        raise AssertionError("allocated before the arguments were checked")
    monkeypatch.setattr(search, "new_frontier_tensors", no_tensors)
    for fn in (search.frontier_search, search.frontier_search_device):
        for kw in (dict(width=0), dict(width=65), dict(max_children=0), dict(max_children=65), dict(width=33, max_children=32), dict(prior_weight=float("nan")),
                   dict(prior_weight=float("inf")), dict(max_steps=0), dict(depth=0), dict(depth=6), dict(evaluate=None), dict(evaluate=3)):
            args = dict(dict(evaluate=ev, width=2, max_children=3, step_index=0, max_steps=4), **kw)
            with pytest.raises(ValueError):
                fn(root, **args)
    big = SimpleNamespace(num_envs=2 ** 22, device="cpu", cfg=None)
    with pytest.raises(ValueError):
        search.frontier_search(big, ev, 32, 32, 0, max_steps=4)
    monkeypatch.undo()
    ft = search.new_frontier_tensors(2, 2, 3, 4, "cpu")
    for kw in (dict(phases=3), dict(phases=0), dict(width=0), dict(num_candidates=65), dict(width=64, num_candidates=17)):
        with pytest.raises(ValueError):
            search.frontier_advance(ft, **dict(dict(phases=search.FRONTIER_INIT, width=2, num_candidates=3), **kw))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_other_searches_are_what_they_were():
    """puct_search and gumbel_search against their CPU models, which know nothing of a frontier: the same trees, bit for bit."""
    import test_gumbel_model as tgm
    case = pc.synthetic(14, 5, 3, 3, 14)
    pc.compare_with_search(case.states[-1], case.ps)
    s = tgm.SEARCH
    N = 1 + 2 * (s["n"] + 1) * s["C"]
    gs, calls = gc.record_search(s["P"], s["levels"], s["n"], s["Mc"], s["C"], pc.synthetic_evaluator(s["P"], s["levels"], s["K"], 23), s["rule"], s["key"], capacity=N)
    tgm._replay(gs, calls, gc.init_state(s["P"], N, s["C"], s["levels"]))
