#!/usr/bin/env python3
"""pcbenv_evaluate_logits / pcbenv_evaluate_logits_backward (pcbenv.masked_categorical.evaluate) against the torch chain
they replace in a PPO update.

Cases: c3 with N = 4 096 and N = 10 240 rows (fp32, bf16), c4 with N = 10 240 (fp32), c5 with N = 8 192 (bf16), masks
taken after reset, midway and at the last component.  Per case, from HIP events after warm-up, the paths alternating in
one process on the same tensors (best of three rounds):
  fwd_us / bwd_us   one pcbenv_evaluate_logits / pcbenv_evaluate_logits_backward launch (preallocated outputs)
  sampler_us        pcbenv_sample_logits on the same logits and masks (the forward does strictly less)
  pair_us           evaluate(...) + backward() through torch.autograd (the two launches, the gradient allocation and the
                    small [N] ops of the loss)
  torch_us          masked_logits + Categorical.log_prob + entropy + backward() on the same tensors
  needed bytes      the 128-byte logits lines that hold a legal action + mask words + outputs; backward adds the
                    N*A*elemsize gradient written; and their share of 8 TB/s
  peak MB           torch.cuda.max_memory_allocated over one forward + backward of each path, above what was allocated
Then an A/B of PPOTrainer.update at c4 x 1 024, T = 10, with device_evaluator off / on.

    python tools/evaluate_logits_bench.py [--iters 100] [--skip-ppo] [--only c3,c4,c5]
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
from pcbenv.masked_categorical import evaluate  # noqa: E402
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
    """(forward, backward) bytes: logits lines (128 B) that hold a legal action + the mask words + the per-row inputs and
    outputs (action, log_prob, entropy, stats / stats, two gradients); backward also writes the whole gradient."""
    N, cfg = env.num_envs, env.cfg
    A = cfg.num_orientations * cfg.height * cfg.width
    esz = 4 if dtype == torch.float32 else 2
    per_line = 128 // esz
    legal = env.action_mask.reshape(N, A).bool()
    assert (A * esz) % 128 == 0
    lines = int(legal.view(N, A // per_line, per_line).any(-1).sum())
    words = N * (1 if cfg.num_orientations == 1 else 2) * cfg.height * ((cfg.width + 63) // 64) * 8
    return lines * 128 + words + N * 28, lines * 128 + words + N * A * esz + N * 28, int(legal.sum()) / N


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def point_bench(name, N, dtypes, iters, out):
    cfg = named_config(name)
    env = BatchedPlacementEnv(cfg, N, queue_depth=1, run_seed=1)
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
        bits, mask = env.mask_bits(), env.action_mask
        for dtype in dtypes:
            logits = (torch.randn((N, A), generator=gen, device=env.device) * 2).to(dtype)
            acts, _, _ = env.sample_logits(logits, 7, flat=True)
            acts64 = acts.long()
            g_lp = torch.randn(N, generator=gen, device=env.device)
            g_h = 0.01 * torch.randn(N, generator=gen, device=env.device)
            stats = torch.empty((N, 4), dtype=torch.float32, device=env.device)
            grad = torch.empty_like(logits)
            x = logits.clone().requires_grad_(True)

            def fwd():
                env.evaluate_logits_forward(logits, bits, acts, stats)

            def bwd():
                env.evaluate_logits_backward(logits, bits, acts, stats, g_lp, g_h, out=grad)

            def sampler():
                env.sample_logits(logits, 7, flat=True)

            def pair():
                x.grad = None
                lp, ent = evaluate(env, x, bits, acts)
                (lp * g_lp + ent * g_h).sum().backward()

            def torch_path():
                x.grad = None
                d = torch.distributions.Categorical(logits=masked_logits(x.float(), mask), validate_args=False)
                (d.log_prob(acts64) * g_lp + d.entropy() * g_h).sum().backward()
            paths = {"fwd": (fwd, iters), "bwd": (bwd, iters), "sampler": (sampler, iters), "pair": (pair, iters),
                     "torch": (torch_path, max(5, iters // 10))}
            for f, _ in paths.values():
                for _ in range(5):
                    f()
            torch.cuda.synchronize()
            us = {k: [] for k in paths}
            for _ in range(3):  # alternate, take the best of three rounds each
                for k, (f, n) in paths.items():
                    us[k].append(timed(f, n))
            best = {k: min(v) for k, v in us.items()}
            mem = {"pair": peak_mb(pair), "torch": peak_mb(torch_path)}
            x.grad = None
            fb, bb, legal_per_row = needed_bytes(env, dtype)
            row = {"config": name, "N": N, "dtype": str(dtype).replace("torch.", ""), "point": pname,
                   "legal_per_row": round(legal_per_row, 1),
                   "fwd_us": round(best["fwd"], 2), "bwd_us": round(best["bwd"], 2), "sampler_us": round(best["sampler"], 2),
                   "pair_us": round(best["pair"], 1), "torch_us": round(best["torch"], 1),
                   "speedup_pair": round(best["torch"] / best["pair"], 1),
                   "speedup_kernels": round(best["torch"] / (best["fwd"] + best["bwd"]), 1),
                   "fwd_needed_MB": round(fb / 1e6, 1), "fwd_frac_8TBs": round(fb / (best["fwd"] * 1e-6) / HBM, 3),
                   "bwd_needed_MB": round(bb / 1e6, 1), "bwd_frac_8TBs": round(bb / (best["bwd"] * 1e-6) / HBM, 3),
                   "peak_MB_pair": round(mem["pair"], 1), "peak_MB_torch": round(mem["torch"], 1),
                   "logits_MB": round(N * A * logits.element_size() / 1e6, 1)}
            print(json.dumps(row), flush=True)
            out.append(row)
            del logits, grad, x
    env.close()
    torch.cuda.empty_cache()


def ppo_ab(rounds=3):
    from pcbenv.policy import SpatialPolicy
    from pcbenv.ppo import PPOConfig, PPOTrainer
    cfg = named_config("c4")
    res, peak, trainers, batches = {}, {}, {}, {}
    for on in (False, True):
        torch.manual_seed(0)
        env = BatchedPlacementEnv(cfg, 1024, queue_depth=4, auto_reset=True, run_seed=2)
        env.generate_instances()
        env.reset()
        trainers[on] = PPOTrainer(env, SpatialPolicy(cfg).to(env.device), PPOConfig(rollout_steps=10, device_evaluator=on))
        batches[on] = trainers[on].collect()
        trainers[on].update(batches[on])  # warm-up
        res[on] = []
    for _ in range(rounds):
        for on, tr in trainers.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            tr.update(batches[on])
            torch.cuda.synchronize()
            res[on].append((time.perf_counter() - t0) * 1e3)
            peak[on] = (torch.cuda.max_memory_allocated() - base) / 1e6
    row = {"ppo_update_c4_1024_T10_ms": {"torch": [round(x, 1) for x in res[False]], "device_evaluator": [round(x, 1) for x in res[True]]},
           "best_ms": {"torch": round(min(res[False]), 1), "device_evaluator": round(min(res[True]), 1)},
           "peak_MB_above_resident": {"torch": round(peak[False], 1), "device_evaluator": round(peak[True], 1)}}
    print(json.dumps(row), flush=True)
    for tr in trainers.values():
        tr.env.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--skip-ppo", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated subset of c3,c4,c5")
    ap.add_argument("--rows", type=int, default=0, help="only the cases with this many rows")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_logits_bench.py needs a GPU")
    print(f"# {torch.cuda.get_device_name(0)}  torch {torch.__version__}  iters {args.iters}", flush=True)
    out = []
    f32, bf16 = torch.float32, torch.bfloat16
    runs = [("c3", 4096, (f32, bf16)), ("c3", 10240, (f32, bf16)), ("c4", 10240, (f32,)), ("c5", 8192, (bf16,))]
    for name, N, dtypes in runs:
        if (args.only and name not in args.only.split(",")) or (args.rows and N != args.rows):
            continue
        point_bench(name, N, dtypes, args.iters, out)
    if not args.skip_ppo:
        ppo_ab()


if __name__ == "__main__":
    main()
