"""The frontier step (pcbenv_frontier_advance) against its specification's tensor chain, its bytes against the memory
bandwidth, and a beam search over placements against the Gumbel search end to end.
python tools/frontier_bench.py [--roots 4096] [--search-roots 256] [--shapes 4x16 16x16 16x64] [--depths 1 8 15] [--reps 20] [--config c3]
                               [--end-to-end [--seeds 11 12 13] [--widths 1 4 16] [--simulations 16 64]]

One JSON line each:
  (a) the launch against the chain.  A real search -- `--search-roots` roots of `--config`, network_evaluator(priors="device")
      with constant logits and a uniform rollout for a value, prior_weight 0 -- is run depth by depth, and at every depth of
      `--depths` the frontier it holds is dumped: the in set, the evaluation of its rows and the accumulators.  The dump is
      tiled to `--roots` roots (whole roots, copied: 4096 roots are 16 copies of the frontiers of 256; a planner of 4096 x
      1024 environments is not needed for a measurement of the step).  On those tensors, alternating, `reps` times each
      after a warm-up: the ADVANCE launch, and `pcbenv.search.frontier_advance` on the device -- what a user writes without
      the kernel.  Timed by device events; best_value and best_len are put back before every timed call, outside the
      events, so that every call does the same work.  Reported: the median and the spread (min, max) of each, their ratio.
  (b) the bytes.  What the rule needs for that frontier, counted from its rows and lengths: path_len of every row; value,
      leaf_terminal and cand_count of the live rows; the path prefix of every kept parent once; the candidate action and
      prior of every child; every child's path, length, cum_logp and parent_row written; -1, -1 for the other slots.  Over
      the median launch time, against 8 TB/s.
  (c) --end-to-end: tools/search_demo.py --frontier W --device-priors at `--search-roots` roots for W in `--widths`, K = 16,
      and --puct --device-priors --reuse --gumbel 4 --gumbel-full at k in `--simulations`, per seed, each in a process of
      its own: the mean final reward, the evaluated rows per episode and the time per episode."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "rl-environment-for-component-placement_amd"))
import torch  # noqa: E402

from pcbenv import named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv, default_max_steps  # noqa: E402
from pcbenv.search import FRONTIER_ADVANCE, FRONTIER_INIT, Evaluation, frontier_advance, network_evaluator, new_frontier_tensors  # noqa: E402

PEAK_BYTES_PER_S = 8e12
INPUTS = ("value", "terminal", "cand_count", "cand_actions", "cand_prior")


def dumped_frontiers(cfg, P, W, K, depths, seed=11):
    """The search of frontier_search_device, depth by depth -> {d: (in set index, ft tensors cloned, the evaluation)} before ADVANCE d."""
    def make(n):
        e = BatchedPlacementEnv(cfg, n, queue_depth=1, run_seed=seed)
        e.generate_instances()
        e.reset()
        return e
    root, planner = make(P), make(P * W * K)
    T, dev = default_max_steps(cfg), root.device
    zeros = torch.zeros((P * W * K, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=dev)
    evaluate = network_evaluator(root, planner, lambda obs: zeros, max_children=K, priors="device", leaves=W * K)
    ft = new_frontier_tensors(P, W, K, T, dev)
    req = root.frontier_request(ft, W, K, 0.0)
    root.frontier_advance(req, FRONTIER_INIT, swap=True)
    out = {}
    for d in range(max(depths) + 1):
        cur = d % 2
        ev = evaluate(ft[f"paths_{cur}"], ft[f"path_len_{cur}"], 1000 + d * T)
        if d in depths:
            out[d] = (cur, {n: t.clone() for n, t in ft.items()}, Evaluation(*(getattr(ev, f).clone() for f in INPUTS)))
        root.frontier_advance(req, FRONTIER_ADVANCE, ev, swap=cur == 1)
    torch.cuda.synchronize()
    assert int(ft["errors_dev"][0]) == 0
    root.close()
    planner.close()
    return out, T


def tiled(t, copies, root_dim):
    """A tensor whose dimension `root_dim` is root-major, `copies` times over."""
    reps = [1] * t.dim()
    reps[root_dim] = copies
    return t.repeat(*reps).contiguous()


def needed_bytes(ft, cur, T, K):
    """(b): counted from the frontier read (set `cur`) and the one written (the other set, after an ADVANCE)."""
    length, out_len = ft[f"path_len_{cur}"].to(torch.int64), ft[f"path_len_{1 - cur}"].to(torch.int64)
    rows = length.numel()
    live = int(((length >= 0) & (length <= T)).sum())
    child = out_len >= 0
    children = int(child.sum())
    first = child & (torch.arange(rows, device=length.device) % K == 0)  # child 0 of every kept parent
    prefix_read = int((out_len[first] - 1).sum()) * 12
    written = int(out_len[child].sum()) * 12 + children * (4 + 8 + 4) + (rows - children) * 8
    return dict(rows=rows, live_rows=live, kept_parents=int(first.sum()), children=children,
                bytes=4 * rows + live * (8 + 1 + 4) + prefix_read + children * (12 + 4) + written)


def step(a):
    cfg = named_config(a.config)
    handle = BatchedPlacementEnv(cfg, 2, queue_depth=1, run_seed=1)  # the handle gives the device only
    med = lambda v: sorted(v)[len(v) // 2]
    for shape in a.shapes:
        W, K = (int(x) for x in shape.split("x"))
        dumps, T = dumped_frontiers(cfg, a.search_roots, W, K, a.depths)
        copies = max(1, a.roots // a.search_roots)
        P = a.search_roots * copies
        for d in a.depths:
            cur, small, ev_small = dumps[d]
            ft = {n: tiled(t, copies, 1 if n.startswith("paths") or n == "best_path" else 0) if n != "errors_dev" else t.clone() for n, t in small.items()}
            ev = Evaluation(*(tiled(getattr(ev_small, f), copies, 0) for f in INPUTS))
            keep = {n: ft[n].clone() for n in ("best_value", "best_len")}
            req = handle.frontier_request(ft, W, K, 0.0)
            kernel = lambda: handle.frontier_advance(req, FRONTIER_ADVANCE, ev, swap=cur == 1)
            chain = lambda: frontier_advance(ft, FRONTIER_ADVANCE, W, K, 0.0, ev, swap=cur == 1)

            def timed(fn):
                for n, t in keep.items():
                    ft[n].copy_(t)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                return t0.elapsed_time(t1)
            for _ in range(3):  # warm-up of both
                timed(kernel), timed(chain)
            ms = {"launch": [], "chain": []}
            for _ in range(a.reps):  # alternating
                ms["launch"].append(timed(kernel))
                ms["chain"].append(timed(chain))
            timed(kernel)
            need = needed_bytes(ft, cur, T, K)
            lm, cm = med(ms["launch"]), med(ms["chain"])
            print(json.dumps({"what": "step", "config": a.config, "roots": P, "copies_of_search_roots": copies, "width": W, "num_candidates": K, "max_steps": T,
                              "depth": d, **need, "launch_ms_median": round(lm, 4), "launch_ms_min_max": [round(min(ms["launch"]), 4), round(max(ms["launch"]), 4)],
                              "chain_ms_median": round(cm, 4), "chain_ms_min_max": [round(min(ms["chain"]), 4), round(max(ms["chain"]), 4)],
                              "chain_over_launch": round(cm / lm, 1), "needed_GB_per_s": round(need["bytes"] / (lm * 1e-3) / 1e9, 1),
                              "share_of_8_TB_per_s": round(need["bytes"] / (lm * 1e-3) / PEAK_BYTES_PER_S, 4), "reps": a.reps}), flush=True)
    handle.close()


def end_to_end(a):
    demo = [sys.executable, os.path.join(HERE, "search_demo.py"), "--config", a.config, "--roots", str(a.search_roots), "--device-priors"]
    runs = [("frontier", W, ["--frontier", str(W), "--k", "16"]) for W in a.widths] + \
           [("gumbel", k, ["--puct", "--reuse", "--gumbel", "4", "--gumbel-full", "--k", str(k)]) for k in a.simulations]
    for seed in a.seeds:
        for kind, n, args in runs:
            t0 = time.perf_counter()
            done = subprocess.run(demo + args + ["--seed", str(seed)], capture_output=True, text=True, timeout=a.run_timeout)
            line = [ln for ln in done.stdout.splitlines() if ln.startswith("{")]
            if done.returncode != 0 or not line:
                print(json.dumps({"what": "end_to_end", "search": kind, "budget": n, "seed": seed, "failed": done.returncode, "stderr": done.stderr[-400:]}), flush=True)
                return 1
            r = json.loads(line[-1])
            P = r["roots"]
            rows = r["evaluated_rows_per_episode"] if kind == "frontier" else r["evaluated_leaves"] / P
            print(json.dumps({"what": "end_to_end", "search": kind, "budget": n, "seed": seed, "roots": P,
                              "mean_final_reward": r["frontier_mean_final_reward" if kind == "frontier" else "best_of_k_mean_final_reward"],
                              "random_policy_mean_final_reward": r["random_policy_mean_final_reward"], "evaluated_rows_per_episode": round(rows, 1),
                              "seconds_per_episode": round(r["search_seconds"] / P, 6), "search_seconds": r["search_seconds"],
                              **({"every_plan_reproduced_its_best_value": r["every_plan_reproduced_its_best_value"], "roots_with_a_plan": r["roots_with_a_plan"]}
                                 if kind == "frontier" else {}), "process_seconds": round(time.perf_counter() - t0, 1)}), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--search-roots", type=int, default=256)
    ap.add_argument("--shapes", nargs="+", default=["4x16", "16x16", "16x64"])
    ap.add_argument("--depths", type=int, nargs="+", default=[1, 8, 15])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--config", default="c3")
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--seeds", type=int, nargs="+", default=[11, 12, 13])
    ap.add_argument("--widths", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--simulations", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--run-timeout", type=float, default=240.0)
    a = ap.parse_args()
    return end_to_end(a) if a.end_to_end else step(a)


if __name__ == "__main__":
    sys.exit(main() or 0)
