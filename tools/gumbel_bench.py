"""The launches of a Gumbel root search on the device (pcbenv_gumbel_advance) against the PUCT launches they stand in for
(pcbenv_puct_advance, pcbenv_puct_move) and against the same rule in torch tensors (pcbenv.search.gumbel_select_root and
gumbel_choose, the specification, on the same device).
python tools/gumbel_bench.py [--roots 4096] [--children 16 64] [--evaluations 64] [--considered 16] [--reps 20] [--config c3]

Per C, one JSON line.  The trees are what a PUCT search of `evaluations` evaluations leaves (a scripted evaluator on the
device: a value by a hash of the path, C candidates with geometric priors, T = 8 levels), copied twice: one copy goes on
under the Gumbel launches, one under the PUCT launches, alternating, each timed by HIP events after a warm-up of its own.
  (a) SELECT alone: pcbenv_gumbel_advance(SELECT) -- the counters reset by an untimed BEGIN -- against
      pcbenv_puct_advance(SELECT);
  (b) ABSORB | SELECT with the evaluation of the selection before it, both sides; the Gumbel budget (n = 64) is begun once,
      so the repetitions walk through the schedule as a search does;
  (c) CHOOSE: pcbenv_gumbel_advance(CHOOSE) against pcbenv_puct_move(CHOOSE);
  (d) gumbel_select_root and gumbel_choose on the same tensors, wall time synchronised at both ends, and that they give the
      counters and the six outputs the launches gave, bit for bit."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rl-environment-for-component-placement_amd"))
import torch  # noqa: E402

from pcbenv import _lib, _move_lib, named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv  # noqa: E402
from pcbenv.search import (GUMBEL_ABSORB, GUMBEL_BEGIN, GUMBEL_CHOOSE, GUMBEL_SELECT, PUCT_TREE_TENSORS, Evaluation, gumbel_choose,  # noqa: E402
                           gumbel_select_root, new_gumbel_tensors, new_move_tensors, new_puct_tree)

SEED, T, C_VISIT, C_SCALE, C_PUCT, SIMS = 0x67756D62656C5EED, 8, 50.0, 1.0, 1.25, 64


def scripted(P, C, device):
    """evaluate(paths, path_len, step) on the device: a value in {0.25, 0.5, 0.75} by a hash of (root, path), C candidates
    (0, 0, c) with priors proportional to 0.8^c, terminal at level T."""
    actions = torch.zeros((P, C, 3), dtype=torch.int32, device=device)
    actions[:, :, 2] = torch.arange(C, dtype=torch.int32, device=device)
    prior = 0.8 ** torch.arange(C, dtype=torch.float64, device=device)
    prior = (prior / prior.sum()).to(torch.float32).expand(P, C).contiguous()
    count = torch.full((P,), C, dtype=torch.int32, device=device)
    weight = (torch.arange(T, dtype=torch.int64, device=device) * 2 + 3)[:, None]
    rows = torch.arange(P, dtype=torch.int64, device=device)

    def evaluate(paths, path_len, step_index0):
        on = torch.arange(T, device=device)[:, None] < path_len[None, :]
        h = (torch.where(on, paths[:, :, 2].to(torch.int64) + 1, torch.zeros((), dtype=torch.int64, device=device)) * weight).sum(dim=0) + 7 * rows
        return Evaluation(0.25 + 0.25 * (h % 3).to(torch.float64), (path_len >= T).to(torch.uint8), count, actions, prior)
    return evaluate


def event_ms(launch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


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
        root.puct_advance(root.puct_request(grown, C_PUCT, C), _lib.TREE_INIT | _lib.TREE_SELECT)
        req0 = root.puct_request(grown, C_PUCT, C)
        for m in range(a.evaluations):
            ev = evaluate(grown["paths"], grown["path_len"], m)
            root.puct_advance(req0, _lib.TREE_ABSORB | _lib.TREE_SELECT, ev.value, ev.terminal, ev.cand_count, ev.cand_actions, ev.cand_prior)
        copy = lambda: {k: v.clone() for k, v in grown.items()}
        ta, tb = copy(), copy()  # a: the Gumbel launches, b: the PUCT launches
        ta.update(new_gumbel_tensors(P, C, min(a.considered, C), SIMS, dev))
        tb.update(new_move_tensors(P, N, C, dev))
        greq, preq, mreq = root.gumbel_request(ta, C_PUCT, C, C_VISIT, C_SCALE), root.puct_request(tb, C_PUCT, C), root.puct_move_request(tb, C)
        key = dict(seed=SEED, step_index=7)
        gumbel = lambda phases, ev=None: root.gumbel_advance(greq, phases, *(() if ev is None else (ev.value, ev.terminal, ev.cand_count, ev.cand_actions, ev.cand_prior)), **key)
        puct = lambda phases, ev=None: root.puct_advance(preq, phases, *(() if ev is None else (ev.value, ev.terminal, ev.cand_count, ev.cand_actions, ev.cand_prior)))
        # (a) SELECT alone, and (d) the specification of the root level against it
        sel_g, sel_p, sel_t = [], [], []
        tree_a = {f: ta[f] for f in PUCT_TREE_TENSORS}
        equal = True
        for i in range(reps + 1):
            gumbel(GUMBEL_BEGIN)
            ms_t, spec = wall_ms(lambda: gumbel_select_root(tree_a, ta["sim_index"], ta["sim_visits"], ta["considered"], C, C_VISIT, C_SCALE, SEED, 7,
                                                            root.first_env_index))
            ms_g, ms_p = event_ms(lambda: gumbel(GUMBEL_SELECT)), event_ms(lambda: puct(_lib.TREE_SELECT))
            equal = equal and torch.equal(spec["sim_index"], ta["sim_index"]) and torch.equal(spec["sim_visits"], ta["sim_visits"])
            if i:  # the first round is the warm-up
                sel_g.append(ms_g), sel_p.append(ms_p), sel_t.append(ms_t)
        # (b) ABSORB | SELECT, the budget begun once
        gumbel(GUMBEL_BEGIN | GUMBEL_SELECT)
        puct(_lib.TREE_SELECT)
        abs_g, abs_p = [], []
        for i in range(reps + 1):
            eva, evb = evaluate(ta["paths"], ta["path_len"], i), evaluate(tb["paths"], tb["path_len"], i)
            ms_g, ms_p = event_ms(lambda: gumbel(GUMBEL_ABSORB | GUMBEL_SELECT, eva)), event_ms(lambda: puct(_lib.TREE_ABSORB | _lib.TREE_SELECT, evb))
            if i:
                abs_g.append(ms_g), abs_p.append(ms_p)
        # (c) CHOOSE, and (d) the specification against it
        cho_g, cho_p, cho_t = [], [], []
        for i in range(reps + 1):
            ms_g, ms_p = event_ms(lambda: gumbel(GUMBEL_CHOOSE)), event_ms(lambda: root.puct_move(mreq, _move_lib.MOVE_CHOOSE))
            ms_t, spec = wall_ms(lambda: gumbel_choose(tree_a, ta["sim_visits"], C, C_VISIT, C_SCALE, SEED, 7, root.first_env_index))
            if i:
                cho_g.append(ms_g), cho_p.append(ms_p), cho_t.append(ms_t)
        for f in ("move_slot", "move_action", "child_weights", "child_actions"):
            equal = equal and torch.equal(spec[f], ta[f])
        equal = equal and torch.equal(spec["child_policy"].view(torch.int32), ta["child_policy"].view(torch.int32))
        equal = equal and torch.equal(spec["root_value"].view(torch.int64), ta["root_value"].view(torch.int64))
        r = lambda v: round(med(v), 4)
        print(json.dumps({
            "config": a.config, "roots": P, "max_children": C, "considered": min(a.considered, C), "evaluations": a.evaluations, "reps": reps,
            "equal": bool(equal), "errors": [int(ta["errors_dev"][0]), int(tb["errors_dev"][0])],
            "mean_nodes": round(float(grown["num_nodes"].double().mean()), 1), "scheduled": int(ta["sim_index"].max()),
            "nonzero_target_share": round(float((ta["child_weights"] > 0).double().mean()), 4),
            "select_ms": {"gumbel": r(sel_g), "puct": r(sel_p), "ratio": round(med(sel_g) / med(sel_p), 2), "torch_chain": round(med(sel_t), 2)},
            "absorb_select_ms": {"gumbel": r(abs_g), "puct": r(abs_p), "ratio": round(med(abs_g) / med(abs_p), 2)},
            "choose_ms": {"gumbel": r(cho_g), "puct_move": r(cho_p), "ratio": round(med(cho_g) / med(cho_p), 2), "torch_chain": round(med(cho_t), 2)},
            "select_ms_all": [round(x, 4) for x in sel_g], "absorb_select_ms_all": [round(x, 4) for x in abs_g], "choose_ms_all": [round(x, 4) for x in cho_g]}),
            flush=True)
    root.close()


if __name__ == "__main__":
    main()
