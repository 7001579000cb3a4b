"""The launches of the full Gumbel rule (pcbenv_gumbel_tree_advance) next to the launches of the root rule they stand in for
(pcbenv_gumbel_advance), on copies of the same trees, in the same run.
python tools/gumbel_tree_bench.py [--roots 4096] [--children 16 64] [--evaluations 64] [--considered 16] [--reps 20] [--config c3]

Per C, one JSON line.  The trees are what a PUCT search of `evaluations` evaluations leaves (tools/gumbel_bench.py's scripted
evaluator on the device: a value by a hash of the path, C candidates with geometric priors, T = 8 levels), copied twice: one
copy goes on under pcbenv_gumbel_tree_advance, one under pcbenv_gumbel_advance, alternating, each launch timed by HIP events
after a warm-up round of its own; the medians over `reps` rounds are reported, and every round's time of the new launch.
  (a) SELECT alone, the counters reset by an untimed BEGIN: one scheduled root level and the descent below it;
  (b) SELECT alone with the budget spent (sim_index = n): the node rule, or PUCT, at every level;
  (c) ABSORB | SELECT with the evaluation of the selection before it; the budget (n = 64) is begun once, so the repetitions
      walk through the schedule as a search does;
  (d) CHOOSE.
levels: the mean path_len of the timed selections of either side -- the two rules descend the same trees to different depths;
per_level_us: the SELECT time of (b) over that side's levels, microseconds per launch and level: a level's softmax next to a
level's PUCT score."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rl-environment-for-component-placement_amd"))
import torch  # noqa: E402

from gumbel_bench import C_PUCT, C_SCALE, C_VISIT, SEED, SIMS, T, event_ms, scripted  # noqa: E402
from pcbenv import _lib, named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv  # noqa: E402
from pcbenv.search import GUMBEL_ABSORB, GUMBEL_BEGIN, GUMBEL_CHOOSE, GUMBEL_SELECT, new_gumbel_tensors, new_puct_tree  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--config", default="c3")
    ap.add_argument("--children", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--evaluations", type=int, default=64)
    ap.add_argument("--considered", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    P, reps = a.roots, a.reps
    if 2 * reps + 4 > SIMS:
        ap.error(f"--reps: at most {(SIMS - 4) // 2}, the budget the repetitions walk through is {SIMS} simulations")
    root = BatchedPlacementEnv(named_config(a.config), P, queue_depth=1, run_seed=11)  # the handle gives the device and the stream only
    dev = root.device
    med = lambda v: sorted(v)[len(v) // 2]
    for C in a.children:
        N = 1 + (a.evaluations + 2 * reps + 8) * C
        evaluate = scripted(P, C, dev)
        grown = new_puct_tree(P, N, T, dev)
        req0 = root.puct_request(grown, C_PUCT, C)
        root.puct_advance(req0, _lib.TREE_INIT | _lib.TREE_SELECT)
        for m in range(a.evaluations):
            ev = evaluate(grown["paths"], grown["path_len"], m)
            root.puct_advance(req0, _lib.TREE_ABSORB | _lib.TREE_SELECT, ev.value, ev.terminal, ev.cand_count, ev.cand_actions, ev.cand_prior)
        sides = {}
        for name, advance in (("tree", root.gumbel_tree_advance), ("root", root.gumbel_advance)):
            t = {k: v.clone() for k, v in grown.items()}
            t.update(new_gumbel_tensors(P, C, min(a.considered, C), SIMS, dev))
            req = root.gumbel_request(t, C_PUCT, C, C_VISIT, C_SCALE)
            launch = lambda phases, ev=None, advance=advance, req=req: advance(
                req, phases, *(() if ev is None else (ev.value, ev.terminal, ev.cand_count, ev.cand_actions, ev.cand_prior)), seed=SEED, step_index=7)
            sides[name] = (t, launch)
        times = {k: {"tree": [], "root": []} for k in ("select", "select_spent", "absorb_select", "choose")}
        levels = {k: {"tree": 0.0, "root": 0.0} for k in ("select", "select_spent")}
        for i in range(reps + 1):  # (a) and (b); the first round is the warm-up
            for name, (t, launch) in sides.items():
                launch(GUMBEL_BEGIN)
                ms = event_ms(lambda: launch(GUMBEL_SELECT))
                if i:
                    times["select"][name].append(ms)
                    levels["select"][name] += float(t["path_len"].double().mean()) / reps
                t["sim_index"].fill_(SIMS)
                ms = event_ms(lambda: launch(GUMBEL_SELECT))
                if i:
                    times["select_spent"][name].append(ms)
                    levels["select_spent"][name] += float(t["path_len"].double().mean()) / reps
        for name, (t, launch) in sides.items():
            launch(GUMBEL_BEGIN | GUMBEL_SELECT)
        for i in range(reps + 1):  # (c)
            for name, (t, launch) in sides.items():
                ev = evaluate(t["paths"], t["path_len"], i)
                ms = event_ms(lambda: launch(GUMBEL_ABSORB | GUMBEL_SELECT, ev))
                if i:
                    times["absorb_select"][name].append(ms)
        for i in range(reps + 1):  # (d)
            for name, (t, launch) in sides.items():
                ms = event_ms(lambda: launch(GUMBEL_CHOOSE))
                if i:
                    times["choose"][name].append(ms)
        out = {"config": a.config, "roots": P, "max_children": C, "considered": min(a.considered, C), "evaluations": a.evaluations, "reps": reps,
               "errors": [int(sides[s][0]["errors_dev"][0]) for s in ("tree", "root")], "mean_nodes": round(float(grown["num_nodes"].double().mean()), 1)}
        for k, v in times.items():
            out[k + "_ms"] = {"tree": round(med(v["tree"]), 4), "root": round(med(v["root"]), 4), "ratio": round(med(v["tree"]) / med(v["root"]), 2),
                              "tree_all": [round(x, 4) for x in v["tree"]]}
        out["levels"] = {k: {s: round(x, 2) for s, x in v.items()} for k, v in levels.items()}
        out["per_level_us"] = {s: round(1e3 * med(times["select_spent"][s]) / max(levels["select_spent"][s], 1e-9), 2) for s in ("tree", "root")}
        print(json.dumps(out), flush=True)
    root.close()


if __name__ == "__main__":
    main()
