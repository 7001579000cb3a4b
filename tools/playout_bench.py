"""pcbenv_playout against the path it replaces: k forks of every root played to their end, from the empty board.
python tools/playout_bench.py [--cases c3:centroid,c4:centroid,c3:both] [--roots 256,4096] [--k 16] [--regions 7] [--reps 3]

"planner": pcbenv.search.best_of_k -- gather_ into a planner handle of P * k environments with every observation tensor
bound, then max_num_components rollout_step launches.  "playout": pcbenv.search.best_of_k_playouts -- one pcbenv_playout
launch, no planner.  Both return the same BestOfK (tests/test_playout_gpu.py).  Timed with HIP events around `reps`
back-to-back calls after warm-up; the figure is the median over the regions, the two paths' regions alternating.  One JSON
line per shape: us per search call, playouts/s, the ratio planner / playout and the device memory each path needs on top of
the roots (the planner handle with its tensors, measured as the drop in free device memory; the playout call's outputs)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rl-environment-for-component-placement_amd"))
import torch  # noqa: E402

from pcbenv import named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv  # noqa: E402
from pcbenv.search import best_of_k, best_of_k_playouts  # noqa: E402


def region(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def run(name, reward, P, k, regions, reps, warmup):
    cfg = named_config(name, reward)
    T, n = cfg.max_num_components, P * k
    root = BatchedPlacementEnv(cfg, P, queue_depth=1, run_seed=1)
    root.generate_instances()
    root.reset()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()  # blocks an earlier shape left in torch's cache would hide the planner's allocations
    free0 = torch.cuda.mem_get_info()[0]
    planner = BatchedPlacementEnv(cfg, n, queue_depth=2, run_seed=1)
    planner.enable_device_instances()
    planner.reset()
    torch.cuda.synchronize()
    planner_bytes = free0 - torch.cuda.mem_get_info()[0]
    playout_bytes = n * (8 + 1 + 4 + 16) + T * n * 12  # reward, done, length, info, actions
    old = lambda i: best_of_k(root, planner, k, step_index=1000 + i * T)
    new = lambda i: best_of_k_playouts(root, k, step_index=1000 + i * T)
    a, b = old(0), new(0)  # the same search
    assert torch.equal(a.child_rewards.view(torch.int64), b.child_rewards.view(torch.int64)) and torch.equal(a.length, b.length)
    for i in range(warmup):
        old(i), new(i)
    torch.cuda.synchronize()
    t_old, t_new = [], []
    for _ in range(regions):
        t_old.append(region(old, reps))
        t_new.append(region(new, reps))
    us_old, us_new = statistics.median(t_old), statistics.median(t_new)
    out = {"config": name, "reward_type": reward, "roots": P, "k": k, "playouts": n,
           "planner_us": round(us_old, 1), "playout_us": round(us_new, 1), "ratio": round(us_old / us_new, 2),
           "planner_playouts_per_s": round(n / us_old * 1e6), "playout_playouts_per_s": round(n / us_new * 1e6),
           "planner_us_min_max": [round(min(t_old), 1), round(max(t_old), 1)], "playout_us_min_max": [round(min(t_new), 1), round(max(t_new), 1)],
           "planner_device_bytes": int(planner_bytes), "playout_device_bytes": int(playout_bytes), "regions": regions, "reps": reps}
    planner.close()
    root.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3:centroid,c4:centroid,c3:both")
    ap.add_argument("--roots", default="256,4096")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    for case in a.cases.split(","):
        name, reward = case.split(":")
        for P in (int(x) for x in a.roots.split(",")):
            print(json.dumps(run(name, reward, P, a.k, max(a.regions, 5), a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
