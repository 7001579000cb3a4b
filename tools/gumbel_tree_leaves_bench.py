"""The launch of the full Gumbel rule with L leaves (pcbenv_gumbel_tree_advance_leaves) against the two launches it combines,
measured in the same run: the one-leaf launch of the same rule (pcbenv_gumbel_tree_advance: its cost per leaf is its cost per
launch and root) and the root rule's launch of the same L (pcbenv_gumbel_advance_leaves); and next to them the evaluator's step,
pcbenv_top_priors over the P * L rows a launch hands it (L launches over P rows: the handle has P environments).
python tools/gumbel_tree_leaves_bench.py [--roots 4096] [--children 16 64] [--leaves 1 4 8 16] [--evaluations 64] [--considered 16] [--reps 20] [--config c3]

Per C and L, one JSON line.  The trees are what a PUCT search of `evaluations` evaluations leaves (tools/gumbel_bench.py's
scripted evaluator on the device: a value by a hash of root and path, C candidates with geometric priors, T = 8 levels),
copied three times, one copy per launch, the three alternating, each timed by HIP events after a warm-up round of its own.
What is timed is ABSORB | SELECT with the evaluation of the selection before it.  The Gumbel budget is n = 64 simulations:
with L leaves it lasts n / L launches, so behind every n / L - 1 timed launches an untimed ABSORB and BEGIN | SELECT begin
the next move in the tree as it stands.  Reported: the median ms per launch of the three and of the evaluator's step, every
sample, the spread (largest minus smallest sample) of each, the mean rows per launch that were leaves, us per leaf, and the share
of rows that were none (-1: behind a repeat or the end of the budget)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rl-environment-for-component-placement_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from gumbel_bench import C_PUCT, C_SCALE, C_VISIT, SEED, SIMS, T, event_ms  # noqa: E402
from pcbenv import _lib, named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv  # noqa: E402
from pcbenv.search import (GUMBEL_ABSORB, GUMBEL_BEGIN, GUMBEL_SELECT, PUCT_TREE_TENSORS, Evaluation, new_gumbel_tensors, new_puct_tree)  # noqa: E402


def scripted(P, L, C, device):
    """tools/gumbel_bench.py:scripted for P * L rows, row p * L + l told what root p is told of that path."""
    R = P * L
    actions = torch.zeros((R, C, 3), dtype=torch.int32, device=device)
    actions[:, :, 2] = torch.arange(C, dtype=torch.int32, device=device)
    prior = 0.8 ** torch.arange(C, dtype=torch.float64, device=device)
    prior = (prior / prior.sum()).to(torch.float32).expand(R, C).contiguous()
    count = torch.full((R,), C, dtype=torch.int32, device=device)
    weight = (torch.arange(T, dtype=torch.int64, device=device) * 2 + 3)[:, None]
    roots = torch.arange(R, dtype=torch.int64, device=device) // L

    def evaluate(paths, path_len, step_index0):
        on = torch.arange(T, device=device)[:, None] < path_len[None, :]
        h = (torch.where(on, paths[:, :, 2].to(torch.int64) + 1, torch.zeros((), dtype=torch.int64, device=device)) * weight).sum(dim=0) + 7 * roots
        return Evaluation(0.25 + 0.25 * (h % 3).to(torch.float64), (path_len >= T).to(torch.uint8), count, actions, prior)
    return evaluate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--config", default="c3")
    ap.add_argument("--children", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--leaves", type=int, nargs="+", default=[1, 4, 8, 16])
    ap.add_argument("--evaluations", type=int, default=64)
    ap.add_argument("--considered", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    P, reps = a.roots, a.reps
    cfg = named_config(a.config)
    root = BatchedPlacementEnv(cfg, P, queue_depth=1, run_seed=11)  # the handle gives the device and the stream only
    dev = root.device
    med = lambda v: sorted(v)[len(v) // 2]
    key = dict(seed=SEED, step_index=7)
    for C in a.children:
        grow = scripted(P, 1, C, dev)
        for L in a.leaves:
            if L < 1 or SIMS // L < 2:
                ap.error(f"--leaves: {L} leaves leave no launch inside a budget of {SIMS} simulations")
            per_move = SIMS // L - 1  # timed launches of a move: behind them the budget is begun again
            N = 1 + (a.evaluations + (reps + 3 + (reps + 1) // per_move) * L + 8) * C
            grown = new_puct_tree(P, N, T, dev)
            req0 = root.puct_request(grown, C_PUCT, C)
            root.puct_advance(req0, _lib.TREE_INIT | _lib.TREE_SELECT)
            for m in range(a.evaluations):
                ev = grow(grown["paths"], grown["path_len"], m)
                root.puct_advance(req0, _lib.TREE_ABSORB | _lib.TREE_SELECT, ev.value, ev.terminal, ev.cand_count, ev.cand_actions, ev.cand_prior)
            ev = grow(grown["paths"], grown["path_len"], a.evaluations)
            root.puct_advance(req0, _lib.TREE_ABSORB, ev.value, ev.terminal, ev.cand_count, ev.cand_actions, ev.cand_prior)

            def copy(leaves):  # the grown tree under exchange tensors of P * leaves rows, nothing pending
                t = new_puct_tree(P, N, T, dev, leaves)
                for f in PUCT_TREE_TENSORS:
                    t[f].copy_(grown[f])
                return t
            ta, tb, tc = copy(L), copy(1), copy(L)  # a: the full rule with leaves, b: the full rule, one leaf, c: the root rule with leaves
            Mc = min(a.considered, C)
            ta.update(new_gumbel_tensors(P, C, Mc, SIMS, dev))
            tb.update(new_gumbel_tensors(P, C, Mc, SIMS, dev))
            tc.update(new_gumbel_tensors(P, C, Mc, SIMS, dev))
            areq, breq, creq = root.gumbel_leaves_request(ta, C_PUCT, C, C_VISIT, C_SCALE, L), root.gumbel_request(tb, C_PUCT, C, C_VISIT, C_SCALE), \
                root.gumbel_leaves_request(tc, C_PUCT, C, C_VISIT, C_SCALE, L)
            inputs = lambda ev: () if ev is None else (ev.value, ev.terminal, ev.cand_count, ev.cand_actions, ev.cand_prior)
            la = lambda phases, ev=None: root.gumbel_tree_advance_leaves(areq, phases, *inputs(ev), **key)
            lb = lambda phases, ev=None: root.gumbel_tree_advance(breq, phases, *inputs(ev), **key)
            lc = lambda phases, ev=None: root.gumbel_advance_leaves(creq, phases, *inputs(ev), **key)
            many, one = scripted(P, L, C, dev), grow
            la(GUMBEL_BEGIN | GUMBEL_SELECT), lb(GUMBEL_BEGIN | GUMBEL_SELECT), lc(GUMBEL_BEGIN | GUMBEL_SELECT)
            logits = torch.zeros((P, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=dev)  # the evaluator's input, P rows of it
            ms_a, ms_b, ms_c, ms_e, leaves_a, leaves_c = [], [], [], [], [], []
            in_move = 0
            for i in range(reps + 1):
                if in_move == per_move:  # the next move of the leaf search: untimed
                    la(GUMBEL_ABSORB, many(ta["paths"], ta["path_len"], -1))
                    la(GUMBEL_BEGIN | GUMBEL_SELECT)
                    lc(GUMBEL_ABSORB, many(tc["paths"], tc["path_len"], -1))
                    lc(GUMBEL_BEGIN | GUMBEL_SELECT)
                    in_move = 0
                if i and i % (SIMS - 2) == 0:  # and of the one-leaf search
                    lb(GUMBEL_ABSORB, one(tb["paths"], tb["path_len"], -1))
                    lb(GUMBEL_BEGIN | GUMBEL_SELECT)
                eva, evb, evc = many(ta["paths"], ta["path_len"], i), one(tb["paths"], tb["path_len"], i), many(tc["paths"], tc["path_len"], i)
                a_ms = event_ms(lambda: la(GUMBEL_ABSORB | GUMBEL_SELECT, eva))
                b_ms = event_ms(lambda: lb(GUMBEL_ABSORB | GUMBEL_SELECT, evb))
                c_ms = event_ms(lambda: lc(GUMBEL_ABSORB | GUMBEL_SELECT, evc))
                e_ms = event_ms(lambda: [root.top_priors(logits, C) for _ in range(L)])  # P * L rows, as L launches over P rows
                in_move += 1
                if i:  # the first round is the warm-up
                    ms_a.append(a_ms), ms_b.append(b_ms), ms_c.append(c_ms), ms_e.append(e_ms)
                    leaves_a.append(int((ta["path_len"] >= 0).sum())), leaves_c.append(int((tc["path_len"] >= 0).sum()))
            scheduled = float((ta["sim_index"] < SIMS).double().mean())
            mean_a, mean_c = sum(leaves_a) / len(leaves_a), sum(leaves_c) / len(leaves_c)
            r = lambda x: round(x, 4)
            print(json.dumps({
                "config": a.config, "roots": P, "max_children": C, "considered": Mc, "simulations": SIMS, "leaves": L, "evaluations": a.evaluations, "reps": reps,
                "errors": [int(ta["errors_dev"][0]), int(tb["errors_dev"][0]), int(tc["errors_dev"][0])],
                "roots_inside_the_schedule_at_the_end": r(scheduled),
                "absorb_select_ms": {"tree_leaves": r(med(ms_a)), "tree": r(med(ms_b)), "gumbel_leaves": r(med(ms_c)), "evaluator_step": r(med(ms_e))},
                "spread_ms": {"tree_leaves": r(max(ms_a) - min(ms_a)), "tree": r(max(ms_b) - min(ms_b)), "gumbel_leaves": r(max(ms_c) - min(ms_c)),
                              "evaluator_step": r(max(ms_e) - min(ms_e))},
                "leaves_per_launch": {"tree_leaves": round(mean_a, 1), "gumbel_leaves": round(mean_c, 1)},
                "no_leaf_share": {"tree_leaves": r(1.0 - mean_a / (P * L)), "gumbel_leaves": r(1.0 - mean_c / (P * L))},
                "us_per_leaf": {"tree_leaves": r(1e3 * med(ms_a) / max(mean_a, 1.0)), "tree": r(1e3 * med(ms_b) / P), "gumbel_leaves": r(1e3 * med(ms_c) / max(mean_c, 1.0))},
                "us_per_leaf_spread": {"tree_leaves": r(1e3 * (max(ms_a) - min(ms_a)) / max(mean_a, 1.0)), "tree": r(1e3 * (max(ms_b) - min(ms_b)) / P)},
                "every_launch_below_the_evaluator_step": max(ms_a) < min(ms_e),
                "tree_leaves_ms_all": [r(x) for x in ms_a], "tree_ms_all": [r(x) for x in ms_b], "gumbel_leaves_ms_all": [r(x) for x in ms_c],
                "evaluator_step_ms_all": [r(x) for x in ms_e]}), flush=True)
            del ta, tb, tc, grown, logits
    root.close()


if __name__ == "__main__":
    main()
