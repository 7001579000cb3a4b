"""The move of a PUCT tree on the device (pcbenv_puct_move: the choice, and the compaction of the chosen subtree in place)
against the same in torch tensors (pcbenv.search.puct_choose + puct_reroot, the specification, on the same device).
python tools/puct_move_bench.py [--roots 4096] [--iterations 64 256] [--reps 5] [--children 16] [--config c3]

Per tree size, one JSON line.  The trees are what a search of that many iterations leaves (tools/puct_search_bench.py's
fixed evaluations, so that only the tree matters); every timed launch works on a fresh copy of them, the copy outside the
timed region.
  (a) the pcbenv_puct_move(CHOOSE | REROOT) launch by HIP events, greedy, `reps` launches after one warm-up; CHOOSE and
      REROOT alone the same way;
  (b) puct_choose + puct_reroot on the same tensors, wall time synchronised at both ends, interleaved with (a), and that both
      left equal trees and remaps;
  (c) the bytes the launch has to move by the algorithm -- per root, with n used slots of N and k of them kept: the parents of
      the n used slots (4 n), a remap row (4 N), 57 bytes of a node across 11 tensors read and written for every kept node
      (114 k) and INIT stores for the slots given up (57 (n - k)) -- over the launch's time, and that as a fraction of the
      8 TB/s the MI355X's HBM is specified at (6.3 TB/s is what a float4 copy reaches)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rl-environment-for-component-placement_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import puct_search_bench as psb  # noqa: E402
from pcbenv import _lib, _move_lib, named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv, default_max_steps  # noqa: E402
from pcbenv.search import PUCT_TREE_TENSORS, new_move_tensors, new_puct_tree, puct_choose, puct_reroot, _puct_iterations  # noqa: E402

NODE_BYTES, HBM_SPEC = 5 * 4 + 12 + 3 * 8 + 1, 8.0e12


def searched_tree(root, M, T, C):
    """The device tree a search of M iterations with the fixed evaluations leaves."""
    P = root.num_envs
    tree = new_puct_tree(P, 1 + M * C, T, root.device)
    fixed = psb.fixed_evaluations(P, M, C, root.device)
    _puct_iterations(root, root.puct_request(tree, psb.C_PUCT, C), tree, M, T, psb.replayed(fixed, T), 0, _lib.TREE_INIT | _lib.TREE_SELECT)
    torch.cuda.synchronize()
    return tree


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--config", default="c3")
    ap.add_argument("--iterations", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--children", type=int, default=16)
    a = ap.parse_args()
    P, C = a.roots, a.children
    cfg = named_config(a.config, reward_type="centroid")
    root = BatchedPlacementEnv(cfg, P, queue_depth=1, run_seed=11)  # the handle gives the device and the stream only
    T = default_max_steps(cfg)
    med = lambda v: sorted(v)[len(v) // 2]
    for M in a.iterations:
        src = searched_tree(root, M, T, C)
        N = src["parent"].shape[1]
        work = {n: src[n].clone() for n in PUCT_TREE_TENSORS}
        work.update(new_move_tensors(P, N, C, root.device), errors_dev=torch.zeros(1, dtype=torch.int32, device=root.device))
        req = root.puct_move_request(work, C)

        def fresh():
            for n in PUCT_TREE_TENSORS:
                work[n].copy_(src[n])

        def launch_ms(phases):
            fresh()
            if phases == _move_lib.MOVE_REROOT:
                root.puct_move(req, _move_lib.MOVE_CHOOSE)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            root.puct_move(req, phases)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        def chain_ms():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ch = puct_choose(src, C)
            new, remap = puct_reroot(src, ch["move_slot"])
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0), ch, new, remap
        both = _move_lib.MOVE_CHOOSE | _move_lib.MOVE_REROOT
        launch_ms(both)
        _, ch, new, remap = chain_ms()
        equal = bool(all(torch.equal(work[n], new[n]) for n in PUCT_TREE_TENSORS if n not in ("value_sum", "prior", "value_max", "reward_lo", "reward_hi"))
                     and all(work[n].view(torch.int64).equal(new[n].view(torch.int64)) for n in ("value_sum", "prior", "value_max", "reward_lo", "reward_hi"))
                     and torch.equal(work["remap"], remap) and torch.equal(work["move_slot"], ch["move_slot"]) and torch.equal(work["child_visits"], ch["child_visits"]))
        n_used, kept = src["num_nodes"].to(torch.int64), work["num_nodes"].to(torch.int64)
        moved = int((4 * n_used + 4 * N + 2 * NODE_BYTES * kept + NODE_BYTES * (n_used - kept)).sum())
        tb, tc, tr, tt = [], [], [], []
        for _ in range(a.reps):
            tb.append(launch_ms(both))
            tc.append(launch_ms(_move_lib.MOVE_CHOOSE))
            tr.append(launch_ms(_move_lib.MOVE_REROOT))
            tt.append(chain_ms()[0])
        rate = moved / (med(tb) * 1e-3)
        print(json.dumps({
            "config": a.config, "roots": P, "iterations": M, "max_children": C, "capacity": N, "equal": equal, "errors": int(work["errors_dev"][0]),
            "nodes_in_use_mean": round(float(n_used.double().mean()), 1), "nodes_kept_mean": round(float(kept.double().mean()), 1),
            "roots_keeping_more_than_1_plus_C": round(float((kept > 1 + C).double().mean()), 3),
            "move_launch_ms": [round(x, 4) for x in tb], "move_launch_ms_median": round(med(tb), 4),
            "choose_launch_ms_median": round(med(tc), 4), "reroot_launch_ms_median": round(med(tr), 4),
            "torch_chain_ms": [round(x, 2) for x in tt], "torch_chain_ms_median": round(med(tt), 2), "chain_over_launch": round(med(tt) / med(tb), 1),
            "algorithmic_bytes": moved, "algorithmic_GB_per_s": round(rate / 1e9, 1), "fraction_of_8_TB_per_s": round(rate / HBM_SPEC, 3)}), flush=True)
        del src, work
    root.close()


if __name__ == "__main__":
    main()
