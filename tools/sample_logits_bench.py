#!/usr/bin/env python3
"""pcbenv_sample_logits (BatchedPlacementEnv.sample_logits) against the torch path it replaces.

For c3 x 4096 and c4 x 4096 (fp32 and bf16 logits) and c5 x 8192 (bf16) at three points of an episode -- after reset,
midway, at the last component -- it reports the per-launch time from HIP events (--iters launches after warm-up),
the bytes the draw needs (the 128-byte logits lines that hold a legal action, computed from the mask, plus the mask
words and the outputs) and their fraction of 8 TB/s, and, in the same process and alternating with the kernel, the
torch path on the same tensors: masked_logits + Categorical.sample + log_prob + entropy.  Then an A/B of
PPOTrainer.collect with device_sampler False / True at c4 x 1024.

    python tools/sample_logits_bench.py [--iters 200] [--skip-ppo]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rl-environment-for-component-placement_amd"))

import torch  # noqa: E402

from pcbenv import named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv  # noqa: E402
from pcbenv.rollout import masked_logits  # noqa: E402

HBM = 8.0e12


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters  # us per call


def needed_bytes(env, dtype):
    """Logits lines (128 B) that hold a legal action + the mask words + the outputs (flat action, log_prob, entropy)."""
    B, cfg = env.num_envs, env.cfg
    A = cfg.num_orientations * cfg.height * cfg.width
    esz = 4 if dtype == torch.float32 else 2
    per_line = 128 // esz
    legal = env.action_mask.reshape(B, A).bool()
    assert (A * esz) % 128 == 0
    lines = int(legal.view(B, A // per_line, per_line).any(-1).sum())
    words = B * (1 if cfg.num_orientations == 1 else 2) * cfg.height * ((cfg.width + 63) // 64) * 8
    return lines * 128 + words + B * 12, int(legal.sum()) / B


def point_bench(name, B, dtypes, iters, out):
    cfg = named_config(name)
    env = BatchedPlacementEnv(cfg, B, queue_depth=1, run_seed=1)
    env.generate_instances()
    env.reset()
    A = cfg.num_orientations * cfg.height * cfg.width
    points = {"reset": 0, "midway": cfg.max_num_components // 2, "last": cfg.max_num_components - 1}
    done_steps = 0
    gen = torch.Generator(device=env.device).manual_seed(0)
    for pname, at in points.items():
        while done_steps < at:
            env.rollout_step(done_steps)
            done_steps += 1
        for dtype in dtypes:
            logits = (torch.randn((B, A), generator=gen, device=env.device) * 2).to(dtype)
            mask = env.action_mask

            def kernel():
                env.sample_logits(logits, 7, flat=True)

            def torch_path():
                d = torch.distributions.Categorical(logits=masked_logits(logits.float(), mask), validate_args=False)
                a = d.sample()
                d.log_prob(a)
                d.entropy()
            for f in (kernel, torch_path):
                for _ in range(10):
                    f()
            torch.cuda.synchronize()
            k_us, t_us = [], []
            for _ in range(3):  # alternate, take the best of three rounds each
                k_us.append(timed(kernel, iters))
                t_us.append(timed(torch_path, max(10, iters // 10)))
            nbytes, legal_per_env = needed_bytes(env, dtype)
            k, t = min(k_us), min(t_us)
            row = {"config": name, "B": B, "dtype": str(dtype).replace("torch.", ""), "point": pname,
                   "legal_per_env": round(legal_per_env, 1), "kernel_us": round(k, 2), "torch_us": round(t, 1),
                   "speedup": round(t / k, 1), "needed_MB": round(nbytes / 1e6, 1),
                   "frac_8TBs": round(nbytes / (k * 1e-6) / HBM, 3), "logits_MB": round(B * A * logits.element_size() / 1e6, 1)}
            print(json.dumps(row), flush=True)
            out.append(row)
            del logits
    env.close()
    torch.cuda.empty_cache()


def ppo_ab(rounds=3):
    from pcbenv.policy import SpatialPolicy
    from pcbenv.ppo import PPOConfig, PPOTrainer
    cfg = named_config("c4")
    res = {}
    trainers = {}
    for dev_sampler in (False, True):
        torch.manual_seed(0)
        env = BatchedPlacementEnv(cfg, 1024, queue_depth=4, auto_reset=True, run_seed=2)
        env.generate_instances()
        env.reset()
        trainers[dev_sampler] = PPOTrainer(env, SpatialPolicy(cfg).to(env.device), PPOConfig(rollout_steps=10, device_sampler=dev_sampler))
        trainers[dev_sampler].collect()  # warm-up
        res[dev_sampler] = []
    for _ in range(rounds):
        for dev_sampler, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.collect()
            torch.cuda.synchronize()
            res[dev_sampler].append((time.perf_counter() - t0) * 1e3)
    row = {"ppo_collect_c4_1024_10_steps_ms": {"torch": [round(x, 2) for x in res[False]], "device_sampler": [round(x, 2) for x in res[True]]},
           "best_ms": {"torch": round(min(res[False]), 2), "device_sampler": round(min(res[True]), 2)}}
    print(json.dumps(row), flush=True)
    for tr in trainers.values():
        tr.env.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--skip-ppo", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated subset of c3,c4,c5")
    args = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}  torch {torch.__version__}  iters {args.iters}", flush=True)
    out = []
    runs = [("c3", 4096, (torch.float32, torch.bfloat16)), ("c4", 4096, (torch.float32, torch.bfloat16)), ("c5", 8192, (torch.bfloat16,))]
    for name, B, dtypes in runs:
        if args.only and name not in args.only.split(","):
            continue
        point_bench(name, B, dtypes, args.iters, out)
    if not args.skip_ppo:
        ppo_ab()


if __name__ == "__main__":
    main()
