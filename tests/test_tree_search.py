"""pcbenv.search.tree_search on the CPU: a stub backend over a toy game of depth 3 and branching 2 with known rewards.

The game: an action is (0, 0, b), b in {0, 1}; an episode has three transitions, except that b0 = b1 = 1 ends it at the
second.  The final reward is REWARD[b0, b1, b2] (REWARD[1, 1, 0] for the short episode), scaled per root.  Behind its path
a playout "draws" b = (m + t) % 2 at transition t of iteration m -- a function of the step index alone, as the real
draws are -- so every tree below can be worked out by hand, and is: EXPECT_ROOT0 was filled in on paper, and `reference`
is the same search written as a plain loop over dicts, for the roots and iteration counts not done on paper."""
import math
from types import SimpleNamespace

import pytest
import torch

from pcbenv.batched_env import Playout
from pcbenv.search import tree_search

T = 3
REWARD = torch.tensor([[[0.10, 0.90], [0.50, 0.50]], [[0.30, 0.20], [0.70, 0.70]]], dtype=torch.float64)
SCALE = (1.0, -1.0, 4.0)  # root 1 prefers what root 0 avoids; root 2 is root 0 on another scale (the normalisation)


def drawn(step, t):
    m = step // T
    return (m + t) % 2


def backend_for(P, calls=None):
    scale = torch.tensor(SCALE[:P], dtype=torch.float64)

    def backend(paths, path_len, step_index0):
        assert paths.shape == (T, P, 3) and paths.dtype == torch.int32 and path_len.shape == (P,) and path_len.dtype == torch.int32
        if calls is not None:
            calls.append((paths.clone(), path_len.clone(), step_index0))
        acts = torch.zeros((T, P, 3), dtype=torch.int32)
        for t in range(T):
            b = torch.full((P,), drawn(step_index0, t), dtype=torch.int32)
            acts[t, :, 2] = torch.where(t < path_len, paths[t, :, 2], b)
        b0, b1, b2 = (acts[t, :, 2].long() for t in range(T))
        short = (b0 == 1) & (b1 == 1)
        length = torch.where(short, torch.full_like(b0, 2), torch.full_like(b0, 3)).to(torch.int32)
        reward = REWARD[b0, b1, torch.where(short, torch.zeros_like(b2), b2)] * scale
        acts[2] = torch.where(short[:, None], torch.zeros_like(acts[2]), acts[2])
        return Playout(reward, torch.ones(P, dtype=torch.uint8), length, None, acts)
    return backend


def reference(p, iterations, c_uct, max_children):
    """The same search as a plain loop, one root."""
    nodes = [dict(parent=-1, depth=0, b=None, visits=0, vsum=0.0, vmax=-math.inf, terminal=False, children=[])]
    lo, hi = math.inf, -math.inf
    best = (-math.inf, None)
    for m in range(iterations):
        n = 0
        while not nodes[n]["terminal"] and len(nodes[n]["children"]) == max_children:
            def ucb(c):
                q = nodes[c]["vsum"] / nodes[c]["visits"]
                q = (q - lo) / (hi - lo) if hi > lo else 0.0
                return q + c_uct * math.sqrt(math.log(nodes[n]["visits"]) / nodes[c]["visits"])
            scores = [ucb(c) for c in nodes[n]["children"]]
            n = nodes[n]["children"][scores.index(max(scores))]  # the first maximum
        path, k = [], n
        while k > 0:
            path.insert(0, nodes[k]["b"]); k = nodes[k]["parent"]
        bs = path + [drawn(m * T, t) for t in range(len(path), T)]
        short = bs[0] == 1 and bs[1] == 1
        length = 2 if short else 3
        r = float(REWARD[bs[0], bs[1], 0 if short else bs[2]]) * SCALE[p]
        leaf = n
        if not nodes[n]["terminal"] and length > len(path):
            b = bs[len(path)]
            old = [c for c in nodes[n]["children"] if nodes[c]["b"] == b]
            if old:
                leaf = old[0]
            else:
                nodes.append(dict(parent=n, depth=len(path) + 1, b=b, visits=0, vsum=0.0, vmax=-math.inf,
                                  terminal=length <= len(path) + 1, children=[]))
                leaf = len(nodes) - 1
                nodes[n]["children"].append(leaf)
        lo, hi = min(lo, r), max(hi, r)
        k = leaf
        while k >= 0:
            nodes[k]["visits"] += 1; nodes[k]["vsum"] += r; nodes[k]["vmax"] = max(nodes[k]["vmax"], r); k = nodes[k]["parent"]
        if r > best[0]:
            best = (r, bs[:length])
    return nodes, best


def run(P, iterations, c_uct=1.0, max_children=2, **kw):
    root = SimpleNamespace(num_envs=P, device="cpu")
    return tree_search(root, iterations, 0, c_uct=c_uct, max_children=max_children, backend=backend_for(P, **kw), max_steps=T)


# Root 0, c_uct = 1, max_children = 2, worked out on paper.  Iteration m draws b = (m + t) % 2:
#  m=0  root has no child: playout 0,1,0 -> 0.5; node 1 = (root, b=0), visits 1
#  m=1  root has one child (< 2): playout 1,0,1 -> 0.2; node 2 = (root, b=1)
#  m=2  root is full.  lo = 0.2, hi = 0.5: q(1) = 1, q(2) = 0; both visited once, so node 1.  Path [0], draws t=1,2 of
#       m=2: b = 1, 0 -> 0,1,0 -> 0.5; node 3 = (node 1, b=1)
#  m=3  ucb(1) = 1 + sqrt(ln 3 / 2) = 1.741, ucb(2) = 0 + sqrt(ln 3 / 1) = 1.048: node 1 (one child).  draws t=1,2 of m=3:
#       b = 0, 1 -> 0,0,1 -> 0.9; node 4 = (node 1, b=0)
#  m=4  lo = 0.2, hi = 0.9.  q(1) = ((0.5 + 0.5 + 0.9) / 3 - 0.2) / 0.7 = 0.619, ucb(1) = 0.619 + sqrt(ln 4 / 3) = 1.299;
#       ucb(2) = 0 + sqrt(ln 4) = 1.177: node 1, now full.  Children 3 (mean 0.5, q = 0.429) and 4 (0.9, q = 1), one visit
#       each: node 4.  Path [0, 0], draw t=2 of m=4: b = 0 -> 0,0,0 -> 0.1; node 5 = (node 4, b=0), terminal
EXPECT_ROOT0 = dict(
    parent=[-1, 0, 0, 1, 1, 4], depth=[0, 1, 1, 2, 2, 3], b=[0, 0, 1, 1, 0, 0], visits=[5, 4, 1, 1, 2, 1],
    vsum=[0.5 + 0.2 + 0.5 + 0.9 + 0.1, 0.5 + 0.5 + 0.9 + 0.1, 0.2, 0.5, 0.9 + 0.1, 0.1], vmax=[0.9, 0.9, 0.2, 0.5, 0.9, 0.1],
    terminal=[False, False, False, False, False, True], children=[[1, 2], [3, 4], [-1, -1], [-1, -1], [5, -1], [-1, -1]])


def test_five_iterations_by_hand():
    ts = run(1, 5)
    e = EXPECT_ROOT0
    assert ts.num_nodes.tolist() == [6]
    assert ts.parent[0].tolist() == e["parent"] and ts.depth[0].tolist() == e["depth"]
    assert ts.node_action[0, :, 2].tolist() == e["b"] and not ts.node_action[0, :, :2].any()
    assert ts.visits[0].tolist() == e["visits"] and ts.terminal[0].tolist() == e["terminal"]
    assert ts.children[0].tolist() == e["children"]
    # the sums in the order the playouts arrived: bit for bit
    assert ts.value_sum[0].tolist() == e["vsum"] and ts.value_max[0].tolist() == e["vmax"]
    assert ts.child_visits.tolist() == [[4, 1]] and ts.child_actions[0, :, 2].tolist() == [0, 1]
    assert ts.action.tolist() == [[0, 0, 0]]
    assert ts.best_reward.tolist() == [0.9] and ts.best_length.tolist() == [3] and ts.best_actions[:, 0, 2].tolist() == [0, 0, 1]


def check_against_reference(ts, P, iterations, c_uct, max_children):
    for p in range(P):
        nodes, best = reference(p, iterations, c_uct, max_children)
        n = len(nodes)
        assert int(ts.num_nodes[p]) == n
        assert ts.parent[p, :n].tolist() == [k["parent"] for k in nodes] and (ts.parent[p, n:] == -1).all()
        assert ts.depth[p, :n].tolist() == [k["depth"] for k in nodes]
        assert ts.node_action[p, 1:n, 2].tolist() == [k["b"] for k in nodes[1:]]
        assert ts.visits[p, :n].tolist() == [k["visits"] for k in nodes] and not ts.visits[p, n:].any()
        assert ts.value_sum[p, :n].tolist() == [k["vsum"] for k in nodes]
        assert ts.value_max[p, :n].tolist() == [k["vmax"] for k in nodes]
        assert ts.terminal[p, :n].tolist() == [k["terminal"] for k in nodes]
        for k in range(n):
            want = nodes[k]["children"] + [-1] * (max_children - len(nodes[k]["children"]))
            assert ts.children[p, k].tolist() == want, (p, k)
            assert len(nodes[k]["children"]) <= max_children
            assert not (nodes[k]["terminal"] and nodes[k]["children"]), "a terminal node was expanded"
        visits = [nodes[c]["visits"] for c in nodes[0]["children"]]
        assert ts.child_visits[p, :len(visits)].tolist() == visits
        assert int(ts.action[p, 2]) == nodes[nodes[0]["children"][visits.index(max(visits))]]["b"]
        assert float(ts.best_reward[p]) == best[0] and int(ts.best_length[p]) == len(best[1])
        assert ts.best_actions[:len(best[1]), p, 2].tolist() == best[1]


@pytest.mark.parametrize("iterations, c_uct, max_children", [(5, 1.0, 2), (24, 1.0, 2), (24, 0.3, 2), (16, 1.0, 1), (12, 2.0, 3)])
def test_three_roots_in_lock_step(iterations, c_uct, max_children):
    """Roots with different rewards descend differently in one batch.  max_children = 1 makes the tree a chain that ends in
    a terminal node, which is then visited again and again and never expanded; 3 is more than the game's branching."""
    calls = []
    ts = run(3, iterations, c_uct, max_children, calls=calls)
    check_against_reference(ts, 3, iterations, c_uct, max_children)
    assert [c[2] for c in calls] == [m * T for m in range(iterations)]  # step_index0 = step_index + m * max_steps
    if max_children == 3:  # the root never fills: every playout revisits one of its two children, nothing deeper exists
        assert ts.num_nodes.tolist() == [3, 3, 3] and ts.child_visits.sum(dim=1).tolist() == [iterations] * 3
    else:
        assert ts.terminal.any(dim=1).all()
    if max_children == 1:
        assert (ts.children[:, :, 0] >= 0).sum(dim=1).tolist() == [int(n) - 1 for n in ts.num_nodes]
        assert int(ts.num_nodes.max()) <= T + 1 and int(ts.visits[0, 0]) == iterations


def test_ties_go_to_the_lowest_child_slot():
    """Equal rewards everywhere: q is 0 for every child (hi == lo), equal visits tie, and the descent takes the lowest slot;
    the most-visited action of a tie is the lowest slot's too."""
    global REWARD
    saved, REWARD = REWARD, torch.full_like(REWARD, 0.25)
    try:
        ts = run(1, 2)  # two children, one visit each
        assert ts.child_visits.tolist() == [[1, 1]] and ts.action.tolist() == [[0, 0, 0]]  # slot 0 holds b = 0 (m = 0 draws 0)
        ts = run(1, 3)  # the third descent ties between the two: slot 0
        assert ts.child_visits.tolist() == [[2, 1]]
        check_against_reference(run(3, 9), 3, 9, 1.0, 2)
    finally:
        REWARD = saved


def test_nothing_synchronises_inside_the_loop(monkeypatch):
    """No .item(), .cpu(), .tolist(), .numpy(), nonzero() or bool(tensor) while the search runs (each would be a host
    synchronisation on a device)."""
    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"tree_search called Tensor.{name}")
        return f
    backend = backend_for(3)
    root = SimpleNamespace(num_envs=3, device="cpu")
    for name in ("item", "cpu", "tolist", "numpy", "nonzero", "__bool__", "__int__", "__float__", "__index__"):
        monkeypatch.setattr(torch.Tensor, name, refuse(name))
    ts = tree_search(root, 12, 0, c_uct=1.0, max_children=2, backend=backend, max_steps=T)
    monkeypatch.undo()
    check_against_reference(ts, 3, 12, 1.0, 2)


def test_arguments():
    root = SimpleNamespace(num_envs=2, device="cpu")
    with pytest.raises(ValueError):
        tree_search(root, 0, 0, backend=backend_for(2), max_steps=T)
    with pytest.raises(ValueError):
        tree_search(root, 4, 0, max_children=0, backend=backend_for(2), max_steps=T)
