"""pcbenv.search.tree_search_device (the tree on the device: pcbenv_tree_advance + pcbenv_playout_paths per iteration)
against pcbenv.search.tree_search (the tree in torch tensors, some hundred small operations per iteration).
python tools/tree_search_bench.py [--roots 4096] [--configs c3 c4] [--iterations 16 64] [--reps 5]

Per case: both searches interleaved in one process, `reps` repeats each after one warm-up of each, wall time synchronised
at both ends (as item 4 of profiles/path_playouts.txt was taken); that both returned equal trees; then, by HIP events over
the same search, what of a device iteration is the pcbenv_tree_advance launch and what the pcbenv_playout_paths launch --
the rest of the wall time is the host enqueuing them.  One JSON line per case."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rl-environment-for-component-placement_amd"))
import torch  # noqa: E402

from pcbenv import _lib, named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv, default_max_steps  # noqa: E402
from pcbenv.search import new_tree, tree_search, tree_search_device  # noqa: E402

STEP_INDEX, C_UCT, MAX_CHILDREN = 1000, 1.0, 4
FIELDS = ("action", "child_visits", "child_actions", "best_reward", "best_length", "num_nodes", "parent", "depth", "node_action", "visits",
          "value_sum", "value_max", "terminal", "children")


def wall_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def equal_trees(a, b):
    same = all(torch.equal(getattr(a, f), getattr(b, f)) for f in FIELDS)  # floats: equal values, no NaN in a tree
    L = a.best_length
    rows = torch.arange(a.best_actions.shape[0], device=L.device)[:, None] < L[None, :]
    return bool(same and torch.equal(a.best_actions * rows[:, :, None], b.best_actions * rows[:, :, None]))


def launches_ms(root, M, T):
    """The device search again with HIP events around every launch -> (advance ms per iteration, playout ms per iteration)."""
    tree = new_tree(root.num_envs, M + 1, MAX_CHILDREN, T, root.device)
    req = root.tree_request(tree, C_UCT)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(M)]
    root.tree_advance(req, _lib.TREE_INIT | _lib.TREE_SELECT)
    for m in range(M):
        ev[m][0].record()
        po = root.playout(k=1, step_index=STEP_INDEX + m * T, paths=tree["paths"], path_len=tree["path_len"], max_steps=T)
        ev[m][1].record()
        root.tree_advance(req, _lib.TREE_ABSORB | (_lib.TREE_SELECT if m + 1 < M else 0), po.reward, po.length, po.actions)
        ev[m][2].record()
    torch.cuda.synchronize()
    return (sum(e[1].elapsed_time(e[2]) for e in ev) / M, sum(e[0].elapsed_time(e[1]) for e in ev) / M)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--configs", nargs="+", default=["c3", "c4"])
    ap.add_argument("--iterations", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for name in a.configs:
        cfg = named_config(name, reward_type="centroid")
        root = BatchedPlacementEnv(cfg, a.roots, queue_depth=1, run_seed=11)
        root.generate_instances()
        root.reset()
        T = default_max_steps(cfg)
        for M in a.iterations:
            host = lambda: tree_search(root, M, STEP_INDEX, c_uct=C_UCT, max_children=MAX_CHILDREN)
            device = lambda: tree_search_device(root, M, STEP_INDEX, c_uct=C_UCT, max_children=MAX_CHILDREN)
            _, h = wall_ms(host)
            _, d = wall_ms(device)
            equal = equal_trees(h, d)
            th, td = [], []
            for _ in range(a.reps):
                th.append(wall_ms(host)[0])
                td.append(wall_ms(device)[0])
            adv, play = launches_ms(root, M, T)
            med = lambda v: sorted(v)[len(v) // 2]
            per = med(td) / M
            print(json.dumps({
                "config": name, "reward_type": "centroid", "roots": a.roots, "iterations": M, "equal_trees": equal,
                "tree_search_ms": [round(x, 2) for x in th], "tree_search_device_ms": [round(x, 2) for x in td],
                "tree_search_ms_per_iteration": round(med(th) / M, 3), "tree_search_device_ms_per_iteration": round(per, 4),
                "spread_ms_per_iteration": [round((max(th) - min(th)) / M, 4), round((max(td) - min(td)) / M, 4)],
                "advance_launch_ms": round(adv, 4), "playout_launch_ms": round(play, 4),
                "host_enqueue_and_gaps_ms_per_iteration": round(per - adv - play, 4), "speedup": round(med(th) / med(td), 1)}), flush=True)
        root.close()


if __name__ == "__main__":
    main()
