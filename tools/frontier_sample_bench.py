"""The stochastic frontier step (pcbenv_frontier_sample) against the deterministic one (pcbenv_frontier_advance) and against
its specification's tensor chain, on the dumped frontiers of tools/frontier_bench.py.
python tools/frontier_sample_bench.py [--roots 4096] [--search-roots 256] [--shapes 4x16 16x16 16x64] [--depths 1 8 15] [--reps 20] [--config c3]

One JSON line per shape and depth.  The frontiers are frontier_bench.dumped_frontiers': a real search of `--search-roots` roots of
`--config` run depth by depth and dumped before the ADVANCE of every depth of `--depths`, tiled to `--roots` roots.  The
rows get a perturbed log-probability of their own (their cum_logp minus an exponential deviate, seeded) and every root an
empty sample set, so the finished rows that win enter it.  On those tensors, alternating in one process, `reps` times each
after a warm-up: the pcbenv_frontier_sample launch, the pcbenv_frontier_advance launch, and
`pcbenv.search.frontier_sample_advance` on the device -- what a user writes without the kernel.  Timed by device events;
best_value, best_len and set_len are put back before every timed call, outside the events, so that every call does the
same work.  Reported: the median and the spread (min, max) of each and the ratios of the medians."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "rl-environment-for-component-placement_amd"))
import torch  # noqa: E402

from frontier_bench import INPUTS, dumped_frontiers, tiled  # noqa: E402
from pcbenv import named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv  # noqa: E402
from pcbenv.search import FRONTIER_ADVANCE, Evaluation, frontier_sample_advance, new_frontier_sample_tensors  # noqa: E402

SEED, STEP_INDEX = 7, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--search-roots", type=int, default=256)
    ap.add_argument("--shapes", nargs="+", default=["4x16", "16x16", "16x64"])
    ap.add_argument("--depths", type=int, nargs="+", default=[1, 8, 15])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--config", default="c3")
    a = ap.parse_args()
    cfg = named_config(a.config)
    handle = BatchedPlacementEnv(cfg, 2, queue_depth=1, run_seed=1)  # the handle gives the device only
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: [round(min(v), 4), round(max(v), 4)]
    for shape in a.shapes:
        W, K = (int(x) for x in shape.split("x"))
        dumps, T = dumped_frontiers(cfg, a.search_roots, W, K, a.depths)
        copies = max(1, a.roots // a.search_roots)
        P = a.search_roots * copies
        for d in a.depths:
            cur, small, ev_small = dumps[d]
            ft = new_frontier_sample_tensors(P, W, K, T, handle.device)
            for n, t in small.items():
                ft[n] = tiled(t, copies, 1 if n.startswith("paths") or n == "best_path" else 0) if n != "errors_dev" else t.clone()
            gen = torch.Generator(device=handle.device).manual_seed(SEED)
            ft[f"gumbel_{cur}"] = ft[f"cum_logp_{cur}"] - torch.empty_like(ft[f"cum_logp_{cur}"]).exponential_(generator=gen)
            ft["set_len"].fill_(-1)
            ev = Evaluation(*(tiled(getattr(ev_small, f), copies, 0) for f in INPUTS))
            keep = {n: ft[n].clone() for n in ("best_value", "best_len", "set_len")}
            sreq = handle.frontier_sample_request(ft, W, K, SEED)
            dreq = handle.frontier_request(ft, W, K, 0.0)
            calls = {"sample": lambda: handle.frontier_sample(sreq, FRONTIER_ADVANCE, STEP_INDEX + d * T, ev, swap=cur == 1),
                     "advance": lambda: handle.frontier_advance(dreq, FRONTIER_ADVANCE, ev, swap=cur == 1),
                     "chain": lambda: frontier_sample_advance(ft, FRONTIER_ADVANCE, W, K, SEED, STEP_INDEX + d * T, 0, ev, swap=cur == 1)}

            def timed(fn):
                for n, t in keep.items():
                    ft[n].copy_(t)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                return t0.elapsed_time(t1)
            for _ in range(3):  # warm-up of all three
                for fn in calls.values():
                    timed(fn)
            ms = {n: [] for n in calls}
            for _ in range(a.reps):  # alternating
                for n, fn in calls.items():
                    ms[n].append(timed(fn))
            timed(calls["sample"])
            length = ft[f"path_len_{cur}"]
            out = {"what": "sample_step", "config": a.config, "roots": P, "copies_of_search_roots": copies, "width": W, "num_candidates": K, "max_steps": T, "depth": d,
                   "live_rows": int(((length >= 0) & (length <= T)).sum()), "children": int((ft[f"path_len_{1 - cur}"] >= 0).sum()), "set_entries": int((ft["set_len"] >= 0).sum())}
            for n in calls:
                out[f"{n}_ms_median"], out[f"{n}_ms_min_max"] = round(med(ms[n]), 4), spread(ms[n])
            out.update(sample_over_advance=round(med(ms["sample"]) / med(ms["advance"]), 2), chain_over_sample=round(med(ms["chain"]) / med(ms["sample"]), 1),
                       reps=a.reps, errors=int(ft["errors_dev"][0]))
            print(json.dumps(out), flush=True)
    handle.close()


if __name__ == "__main__":
    sys.exit(main() or 0)
