#!/usr/bin/env python3
"""pcbenv_top_priors (BatchedPlacementEnv.top_priors) against the torch chain it replaces in a PUCT search,
pcbenv.search.top_priors, on the same box, in the same process, on the same logits and masks.
python tools/top_priors_bench.py [--rows 4096] [--configs c3 c4] [--K 16 64] [--reps 5] [--iters 20]

Per case (geometry x K x dtype x logits), one JSON line.  The masks are those of real states at mid-episode.  Logits:
"randn" (spread out: from the second histogram round on nearly every segment is skipped) and "constant" (every round
reads every legal logit, and every count of a round goes to one bin: the worst case of the histogram).
  launch_ms    one pcbenv_top_priors launch (the handle's own bit rows, preallocated outputs) by HIP events around
               `iters` launches; `reps` repeats, interleaved with the chain, after one warm-up of each; median and spread
  chain_ms     pcbenv.search.top_priors on the dense action_mask, by HIP events around one call, the same repeats
  floor_ms     pcbenv_evaluate_logits forward on the same logits and bit rows: one read of the row with the same head
               (pass 1, the legal count, Z) -- what this kernel sits above
  equal        the launch's count and actions are the chain's (constant logits: the priors too, bit for bit; randn: rows
               whose kept float32 probabilities collapse may differ in order and are counted in rows_differ)
and whether the launch beats the chain by more than the chain's spread between repeats."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rl-environment-for-component-placement_amd"))

import torch  # noqa: E402

from pcbenv import named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv  # noqa: E402
from pcbenv.search import top_priors  # noqa: E402


def event_ms(fn, iters=1):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--configs", nargs="+", default=["c3", "c4"])
    ap.add_argument("--K", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    med = lambda v: sorted(v)[len(v) // 2]
    for name in a.configs:
        cfg = named_config(name)
        N, A = a.rows, cfg.num_orientations * cfg.height * cfg.width
        env = BatchedPlacementEnv(cfg, N, queue_depth=1, run_seed=1)
        env.generate_instances()
        env.reset()
        for t in range(cfg.max_num_components // 2):
            env.rollout_step(t)
        mask, bits = env.action_mask, env.mask_bits()
        legal_mean = float((mask != 0).reshape(N, -1).sum(1).float().mean())
        gen = torch.Generator(device=env.device).manual_seed(0)
        acts = torch.zeros((N, 3), dtype=torch.int32, device=env.device)
        for dtype in (torch.float32, torch.bfloat16):
            for kind in ("randn", "constant"):
                logits = (torch.randn((N, A), generator=gen, device=env.device) * 2 if kind == "randn"
                          else torch.full((N, A), 0.5, device=env.device)).to(dtype)
                for K in a.K:
                    out = (torch.empty(N, dtype=torch.int32, device=env.device), torch.empty((N, K, 3), dtype=torch.int32, device=env.device),
                           torch.empty((N, K), dtype=torch.float32, device=env.device))
                    launch = lambda: env.top_priors(logits, K, out=out)
                    chain = lambda: top_priors(logits, mask, K)
                    floor = lambda: env.evaluate_logits_forward(logits, bits, acts)
                    want = chain()          # warm-up of each, and the comparison
                    launch()
                    floor()
                    torch.cuda.synchronize()
                    differ = int(((out[0] != want[0]) | (out[1] != want[1]).any(dim=2).any(dim=1)).sum())
                    same_priors = bool(torch.equal(out[2], want[2]))
                    tl, tc, tf = [], [], []
                    for _ in range(a.reps):
                        tl.append(event_ms(launch, a.iters))
                        tc.append(event_ms(chain))
                        tf.append(event_ms(floor, a.iters))
                    print(json.dumps({
                        "config": name, "rows": N, "A": A, "legal_mean": round(legal_mean, 1), "K": K, "dtype": str(dtype)[6:], "logits": kind,
                        "launch_ms": [round(x, 4) for x in tl], "launch_ms_median": round(med(tl), 4),
                        "chain_ms": [round(x, 3) for x in tc], "chain_ms_median": round(med(tc), 3), "chain_spread_ms": round(max(tc) - min(tc), 3),
                        "floor_ms_median": round(med(tf), 4), "launch_over_floor": round(med(tl) / med(tf), 2),
                        "chain_over_launch": round(med(tc) / med(tl), 1),
                        "beats_chain_by_more_than_its_spread": bool(med(tc) - med(tl) > max(tc) - min(tc)),
                        "rows_differ": differ, "priors_bit_identical": same_priors}), flush=True)
        env.close()


if __name__ == "__main__":
    main()
