"""pcbenv_playout_paths against the only other way to evaluate tree nodes named by a path: materialise them.
python tools/path_playout_bench.py [--cases c3:centroid,c4:centroid] [--roots 4096] [--k 16] [--depths 1,4,8] [--regions 5] [--reps 3]
                                   [--tree-iterations 16]

A node is (root, the d actions that lead to it).  "paths": one BatchedPlacementEnv.playout(paths=...) launch
(pcbenv_playout_paths) -- nothing is allocated but the outputs.  "planner": gather_ of the roots into a planner handle of
one environment per node with every observation tensor bound, d step launches with the path's actions, then a playout
from the planner.  Both evaluate the same nodes with the same draws and must agree bit for bit (checked before timing).
The paths are the first d actions of each node's own path-less playout, so every path action is legal.  Timed with HIP
events around `reps` back-to-back calls after warm-up; the figure is the median over the regions, the two ways'
regions alternating.  One JSON line per shape and depth: us per evaluation of all nodes, the ratio, and the device memory
each way needs on top of the roots (the planner handle with its tensors, measured as the drop in free device memory; the
paths call's inputs and outputs) and what a planner step launch may write (the bytes of the tensors bound to it).
Then, per case, tree_search next to best_of_k_playouts with the same number of playouts per root (wall time, host
included, synchronised at both ends)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rl-environment-for-component-placement_amd"))
import torch  # noqa: E402

from pcbenv import named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv  # noqa: E402
from pcbenv.search import best_of_k_playouts, child_index, tree_search  # noqa: E402


def region(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def run(name, reward, P, k, depths, regions, reps, warmup):
    cfg = named_config(name, reward)
    T, n = cfg.max_num_components, P * k
    root = BatchedPlacementEnv(cfg, P, queue_depth=1, run_seed=1)
    root.generate_instances()
    root.reset()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    try:
        planner = BatchedPlacementEnv(cfg, n, queue_depth=1, run_seed=1)
        planner.generate_instances()
        planner.reset()
    except (RuntimeError, MemoryError) as e:  # the planner does not fit: say so
        print(json.dumps({"config": name, "roots": P, "k": k, "planner": "does not fit in device memory", "error": str(e)[:120]}), flush=True)
        root.close()
        return
    torch.cuda.synchronize()
    planner_bytes = free0 - torch.cuda.mem_get_info()[0]
    step_bytes = sum(v.numel() * v.element_size() for v in planner.obs.values()) + n * (8 + 1 + 16)
    index, own = child_index(P, k, root.device), torch.arange(n, dtype=torch.int32, device=root.device)
    base = root.playout(k=k, step_index=1000)
    for d in depths:
        paths = base.actions[:d].contiguous()
        new = lambda i: root.playout(k=k, step_index=1000, paths=paths, actions_steps=0)

        def old(i):
            planner.gather_(index, source=root)
            for t in range(d):
                planner.step(paths[t])
            return planner.playout(index=own, step_index=1000 + d, max_steps=T - d, actions_steps=0)
        a, b = new(0), old(0)
        live = base.length > d  # (a node whose episode ended on the path has nothing left to play: the planner would step a finished episode)
        assert torch.equal(a.reward.view(torch.int64)[live], b.reward.view(torch.int64)[live])
        assert torch.equal(a.reward.view(torch.int64), base.reward.view(torch.int64))  # a prefix of the path-less playout reproduces it
        for i in range(warmup):
            new(i), old(i)
        torch.cuda.synchronize()
        t_old, t_new = [], []
        for _ in range(regions):
            t_old.append(region(old, reps))
            t_new.append(region(new, reps))
        us_old, us_new = statistics.median(t_old), statistics.median(t_new)
        print(json.dumps({"config": name, "reward_type": reward, "roots": P, "k": k, "nodes": n, "depth": d,
                          "planner_us": round(us_old, 1), "paths_us": round(us_new, 1), "ratio": round(us_old / us_new, 2),
                          "planner_us_min_max": [round(min(t_old), 1), round(max(t_old), 1)], "paths_us_min_max": [round(min(t_new), 1), round(max(t_new), 1)],
                          "planner_device_bytes": int(planner_bytes), "planner_bound_tensor_bytes_per_launch": int(step_bytes), "planner_launches": d + 2,
                          "paths_device_bytes": int(n * (8 + 1 + 4 + 16) + d * n * 12), "paths_bytes_written": int(n * (8 + 1 + 4 + 16)),
                          "regions": regions, "reps": reps}), flush=True)
    planner.close()
    root.close()


def tree(name, reward, P, iterations):
    cfg = named_config(name, reward)
    root = BatchedPlacementEnv(cfg, P, queue_depth=1, run_seed=1)
    root.generate_instances()
    root.reset()

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out
    ms_tree, ts = wall(lambda: tree_search(root, iterations, 1000))
    ms_flat, bk = wall(lambda: best_of_k_playouts(root, iterations, 1000))
    print(json.dumps({"config": name, "reward_type": reward, "roots": P, "iterations": iterations, "playouts": P * iterations,
                      "tree_search_ms": round(ms_tree, 2), "tree_search_ms_per_iteration": round(ms_tree / iterations, 3),
                      "best_of_k_playouts_ms": round(ms_flat, 2), "tree_mean_best_reward": float(ts.best_reward.mean()),
                      "best_of_k_mean_reward": float(bk.reward.mean()), "tree_mean_nodes": float(ts.num_nodes.double().mean()),
                      "tree_max_depth": int(ts.depth.max())}), flush=True)
    root.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3:centroid,c4:centroid")
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--depths", default="1,4,8")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tree-iterations", type=int, default=16)
    a = ap.parse_args()
    for case in a.cases.split(","):
        name, reward = case.split(":")
        run(name, reward, a.roots, a.k, [int(x) for x in a.depths.split(",")], max(a.regions, 5), a.reps, a.warmup)
        if a.tree_iterations > 0:
            tree(name, reward, a.roots, a.tree_iterations)


if __name__ == "__main__":
    main()
