"""pcbenv_gather_paths against the path it replaces: materialising tree nodes named by a path in a planner handle.
python tools/gather_paths_bench.py [--cases c3:centroid,c4:centroid] [--roots 4096] [--k 16] [--depths 1,4,8] [--regions 7] [--reps 10]

A node is (root, the d actions that lead to it); the planner handle has one environment per node with every observation
tensor bound.  "steps": planner.gather_(index, source=root) and d planner.step launches with the path's actions -- d + 1
launches, each of which writes the observation tensors.  "paths": one planner.gather_(index, source=root, paths=...)
launch (pcbenv_gather_paths), which writes them once.  Both run in this process on the same handles and must leave the
same observations (checked before timing; reward / done / info are compared on the nodes whose episode has not ended
before the path has: the old way steps a finished episode once more).  The paths are the first d actions of each node's
own path-less playout, so every path action is legal.

Timed with HIP events around `reps` back-to-back calls after warm-up, the two ways' regions alternating; the figure is
the median over the regions, and the smallest and largest region are printed with it (the spread).  One JSON line per
shape and depth: us per materialisation of all nodes, the ratio, whether the ratio's worst case -- the old way's fastest
region over the new way's slowest -- is still above 1, and the bytes of the bound tensors one launch may write."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rl-environment-for-component-placement_amd"))
import torch  # noqa: E402

from pcbenv import named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv  # noqa: E402
from pcbenv.search import child_index  # noqa: E402


def region(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def shown(env):
    out = {k: v.clone() for k, v in env.obs.items()}
    out.update(reward=env.reward.clone(), done=env.done.clone(), info=env.info_raw.clone(), mask_bits=env.mask_bits())
    return out


def run(name, reward, P, k, depths, regions, reps, warmup):
    cfg = named_config(name, reward)
    n = P * k
    root = BatchedPlacementEnv(cfg, P, queue_depth=1, run_seed=1)
    root.generate_instances()
    root.reset()
    planner = BatchedPlacementEnv(cfg, n, queue_depth=1, run_seed=1)
    planner.generate_instances()
    planner.reset()
    obs_bytes = sum(v[0].numel() * v.element_size() for v in planner.obs.values())
    index = child_index(P, k, root.device)
    base = root.playout(k=k, step_index=1000)
    for d in depths:
        paths = base.actions[:d].contiguous()

        def old():
            planner.gather_(index, source=root)
            for t in range(d):
                planner.step(paths[t])

        def new():
            planner.gather_(index, source=root, paths=paths)
        old()
        a = shown(planner)
        new()
        b = shown(planner)
        live = base.length >= d  # the episode has not ended before the path has
        for key in a:
            rows = live if key in ("reward", "done", "info") else slice(None)
            x, y = a[key][rows], b[key][rows]
            same = torch.equal(x.nan_to_num(nan=-7.0), y.nan_to_num(nan=-7.0)) if x.is_floating_point() else torch.equal(x, y)
            assert same, (name, d, key, "the two ways disagree")
        assert torch.equal(planner.gather_length.long(), torch.minimum(base.length.long(), torch.full_like(base.length, d).long()))
        for _ in range(warmup):
            old(), new()
        torch.cuda.synchronize()
        t_old, t_new = [], []
        for _ in range(regions):
            t_old.append(region(old, reps))
            t_new.append(region(new, reps))
        us_old, us_new = statistics.median(t_old), statistics.median(t_new)
        print(json.dumps({"config": name, "reward_type": reward, "roots": P, "k": k, "nodes": n, "depth": d,
                          "steps_us": round(us_old, 1), "paths_us": round(us_new, 1), "ratio": round(us_old / us_new, 2),
                          "steps_us_min_max": [round(min(t_old), 1), round(max(t_old), 1)], "paths_us_min_max": [round(min(t_new), 1), round(max(t_new), 1)],
                          "ratio_worst_case": round(min(t_old) / max(t_new), 2), "faster_beyond_the_spread": min(t_old) > max(t_new),
                          "steps_launches": d + 1, "paths_launches": 1, "live_nodes": int(live.sum()),
                          "observation_bytes_per_node": int(obs_bytes), "regions": regions, "reps": reps}), flush=True)
    planner.close()
    root.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3:centroid,c4:centroid")
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--depths", default="1,4,8")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gather_paths_bench.py needs a GPU (there is nothing to time without one)")
    for case in a.cases.split(","):
        name, reward = case.split(":")
        run(name, reward, a.roots, a.k, [int(x) for x in a.depths.split(",")], max(a.regions, 5), a.reps, a.warmup)


if __name__ == "__main__":
    main()
