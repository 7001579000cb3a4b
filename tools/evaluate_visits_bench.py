#!/usr/bin/env python3
"""pcbenv_evaluate_visits / pcbenv_evaluate_visits_backward (pcbenv.visit_targets.cross_entropy) against the torch chain
they replace in an AlphaZero update and against their twins pcbenv_evaluate_logits / _backward on the same rows.

Cases: c3 with N = 4 096 rows and c5 with N = 1 024, fp32 and bf16, C = 16 and 64 targets per row, masks taken midway
through an episode.  The targets of a row are C distinct legal actions (the top C of random noise, pcbenv_top_priors) with
random visit counts.  Per case, from HIP events after warm-up, the paths alternating in one process on the same tensors
(best of three rounds):
  fwd_us / bwd_us            one pcbenv_evaluate_visits / pcbenv_evaluate_visits_backward launch (preallocated outputs)
  logits_fwd_us / _bwd_us    pcbenv_evaluate_logits / _backward on the same logits and masks with one stored action: the
                             yardstick -- the same bytes but for the 16 C bytes of targets per row
  bwd_no_target_us           the backward launch on the same rows with every visit count 0 (rows of status ROW_NO_TARGET): its
                             prologue -- the target map zeroed, the scan, four barriers -- with an empty map and no hit, so
                             bwd_no_target_us - logits_bwd_us is what the prologue costs and bwd_us - bwd_no_target_us the hits
  pair_us                    cross_entropy(...) + backward() through torch.autograd (both launches, the gradient
                             allocation and the small [N] ops of the loss)
  torch_us                   cross_entropy_torch(...) + backward(): the bits unpacked, log(mask) added, log_softmax, the
                             visits scattered into a dense target
  needed bytes               as tools/evaluate_logits_bench.py (the 128-byte logits lines that hold a legal action + mask
                             words + outputs; backward adds the gradient written) + 16 C N, and their share of 8 TB/s.
                             The launches loop over the same tensors: where logits (and gradient) fit into the 256 MB
                             Infinity Cache -- the bf16 cases, 134 MB of logits -- that share is no HBM figure

    python tools/evaluate_visits_bench.py [--iters 100] [--only c3,c5]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rl-environment-for-component-placement_amd"))

import torch  # noqa: E402

from pcbenv import named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv  # noqa: E402
from pcbenv.visit_targets import cross_entropy, cross_entropy_torch  # noqa: E402

HBM = 8.0e12


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters  # us per call


def needed_bytes(env, dtype, C):
    """(forward, backward) bytes, legal actions per row."""
    N, cfg = env.num_envs, env.cfg
    A = cfg.num_orientations * cfg.height * cfg.width
    esz = 4 if dtype == torch.float32 else 2
    per_line = 128 // esz
    legal = env.action_mask.reshape(N, A).bool()
    assert (A * esz) % 128 == 0
    lines = int(legal.view(N, A // per_line, per_line).any(-1).sum())
    words = N * (1 if cfg.num_orientations == 1 else 2) * cfg.height * ((cfg.width + 63) // 64) * 8
    fwd = lines * 128 + words + N * 16 * C + N * 24
    return fwd, fwd + N * A * esz, int(legal.sum()) / N


def bench(name, N, iters, out):
    cfg = named_config(name)
    env = BatchedPlacementEnv(cfg, N, queue_depth=1, run_seed=1)
    env.generate_instances()
    env.reset()
    A = cfg.num_orientations * cfg.height * cfg.width
    for t in range(cfg.max_num_components // 2):
        env.rollout_step(t)
    bits = env.mask_bits()
    gen = torch.Generator(device=env.device).manual_seed(0)
    for dtype in (torch.float32, torch.bfloat16):
        logits = (torch.randn((N, A), generator=gen, device=env.device) * 2).to(dtype)
        stored, _, _ = env.sample_logits(logits, 7, flat=False)
        g_ce = torch.randn(N, generator=gen, device=env.device)
        g_h = 0.01 * torch.randn(N, generator=gen, device=env.device)
        stats, stats_l, stats_0 = (torch.empty((N, 4), dtype=torch.float32, device=env.device) for _ in range(3))
        grad = torch.empty_like(logits)
        ce_out = (torch.empty(N, device=env.device), torch.empty(N, device=env.device))
        x = logits.clone().requires_grad_(True)
        for C in (16, 64):
            count, actions, _ = env.top_priors(torch.randn((N, A), generator=gen, device=env.device), C, mask_bits=bits)
            visits = torch.randint(1, 51, (N, C), generator=gen, device=env.device, dtype=torch.int32)
            visits = torch.where(torch.arange(C, device=env.device)[None, :] < count[:, None], visits, torch.zeros_like(visits)).contiguous()

            def fwd():
                env.evaluate_visits_forward(logits, bits, visits, actions, stats, out=ce_out)

            def bwd():
                env.evaluate_visits_backward(logits, bits, visits, actions, stats, g_ce, g_h, out=grad)

            no_visits = torch.zeros_like(visits)
            env.evaluate_visits_forward(logits, bits, no_visits, actions, stats_0, out=ce_out)

            def bwd_no_target():
                env.evaluate_visits_backward(logits, bits, no_visits, actions, stats_0, g_ce, g_h, out=grad)

            def logits_fwd():
                env.evaluate_logits_forward(logits, bits, stored, stats_l)

            def logits_bwd():
                env.evaluate_logits_backward(logits, bits, stored, stats_l, g_ce, g_h, out=grad)

            def pair():
                x.grad = None
                ce, ent = cross_entropy(env, x, bits, visits, actions)
                (ce * g_ce + ent * g_h).sum().backward()

            def torch_path():
                x.grad = None
                ce, ent = cross_entropy_torch(cfg, x, bits, visits, actions)
                (ce * g_ce + ent * g_h).sum().backward()
            paths = {"logits_fwd": (logits_fwd, iters), "logits_bwd": (logits_bwd, iters), "fwd": (fwd, iters), "bwd": (bwd, iters),
                     "bwd_no_target": (bwd_no_target, iters),
                     "pair": (pair, iters), "torch": (torch_path, max(5, iters // 10))}
            for f, _ in paths.values():
                for _ in range(5):
                    f()
            torch.cuda.synchronize()
            us = {k: [] for k in paths}
            for _ in range(3):  # alternate, take the best of three rounds each
                for k, (f, n) in paths.items():
                    us[k].append(timed(f, n))
            best = {k: min(v) for k, v in us.items()}
            x.grad = None
            fb, bb, legal_per_row = needed_bytes(env, dtype, C)
            row = {"config": name, "N": N, "dtype": str(dtype).replace("torch.", ""), "C": C, "legal_per_row": round(legal_per_row, 1),
                   "fwd_us": round(best["fwd"], 2), "bwd_us": round(best["bwd"], 2), "bwd_no_target_us": round(best["bwd_no_target"], 2),
                   "logits_fwd_us": round(best["logits_fwd"], 2), "logits_bwd_us": round(best["logits_bwd"], 2),
                   "fwd_vs_logits": round(best["fwd"] / best["logits_fwd"], 3), "bwd_vs_logits": round(best["bwd"] / best["logits_bwd"], 3),
                   "pair_us": round(best["pair"], 1), "torch_us": round(best["torch"], 1),
                   "speedup_pair": round(best["torch"] / best["pair"], 1),
                   "speedup_kernels": round(best["torch"] / (best["fwd"] + best["bwd"]), 1),
                   "fwd_needed_MB": round(fb / 1e6, 1), "fwd_frac_8TBs": round(fb / (best["fwd"] * 1e-6) / HBM, 3),
                   "bwd_needed_MB": round(bb / 1e6, 1), "bwd_frac_8TBs": round(bb / (best["bwd"] * 1e-6) / HBM, 3),
                   "logits_MB": round(N * A * logits.element_size() / 1e6, 1)}
            print(json.dumps(row), flush=True)
            out.append(row)
        del logits, grad, x
    env.close()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--only", default="", help="comma-separated subset of c3,c5")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_visits_bench.py needs a GPU")
    print(f"# {torch.cuda.get_device_name(0)}  torch {torch.__version__}  iters {args.iters}", flush=True)
    out = []
    for name, N in (("c3", 4096), ("c5", 1024)):
        if args.only and name not in args.only.split(","):
            continue
        bench(name, N, args.iters, out)


if __name__ == "__main__":
    main()
