"""Dirichlet noise on the root priors of a PUCT tree on the device (pcbenv_puct_root_noise) against the same in torch tensors
(pcbenv.search.puct_root_noise, the specification, on the same device) and against CHOOSE on the same trees.
python tools/puct_noise_bench.py [--roots 4096] [--children 16 64] [--alphas 0.3 2.5] [--reps 5] [--config c3]

Per (C, alpha), one JSON line.  Every root has C children in the slots 1 .. C with uniform float32 priors; every timed launch
works on fresh priors and a zeroed `noised`, the reset outside the timed region.
  (a) the pcbenv_puct_root_noise launch by HIP events, `reps` launches after one warm-up;
  (b) puct_root_noise on the same tensors, wall time synchronised at both ends, interleaved with (a), and that both left
      the same priors, bit for bit, and the same `noised`;
  (c) the pcbenv_puct_move(CHOOSE) launch on the same trees by HIP events, interleaved: the other move-level launch."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rl-environment-for-component-placement_amd"))
import torch  # noqa: E402

from pcbenv import _move_lib, named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv  # noqa: E402
from pcbenv.search import new_move_tensors, new_puct_tree, puct_root_noise  # noqa: E402

SEED, EPS = 0x5EED0123456789AB, 0.25


def flat_tree(P, C, device):
    """P roots of N = C + 1 slots whose C children hold uniform priors and one visit each."""
    tree = new_puct_tree(P, C + 1, 1, device)
    for n, v in (("parent", 0), ("depth", 1), ("visits", 1), ("num_children", 0), ("first_child", -1), ("node_action", 0), ("value_sum", 0.5),
                 ("value_max", 0.5), ("terminal", 0), ("reward_lo", 0.0), ("reward_hi", 1.0), ("num_nodes", C + 1)):
        tree[n].fill_(v)
    tree["parent"][:, 0], tree["depth"][:, 0], tree["visits"][:, 0] = -1, 0, C
    tree["num_children"][:, 0], tree["first_child"][:, 0] = C, 1
    tree["prior"].fill_(float(torch.tensor(1.0 / C, dtype=torch.float32)))
    tree["prior"][:, 0] = 0.0
    return tree


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--config", default="c3")
    ap.add_argument("--children", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--alphas", type=float, nargs="+", default=[0.3, 2.5])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    P = a.roots
    root = BatchedPlacementEnv(named_config(a.config), P, queue_depth=1, run_seed=11)  # the handle gives the device and the stream only
    med = lambda v: sorted(v)[len(v) // 2]
    for C in a.children:
        tree = flat_tree(P, C, root.device)
        tree.update(new_move_tensors(P, C + 1, C, root.device))
        src = tree["prior"].clone()
        req, mreq = root.puct_noise_request(tree, C), root.puct_move_request(tree, C)
        for alpha in a.alphas:
            def fresh():
                tree["prior"].copy_(src)
                tree["noised"].zero_()

            def event_ms(launch):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)

            def noise_ms():
                fresh()
                return event_ms(lambda: root.puct_root_noise(req, alpha, EPS, seed=SEED, step_index=7))

            def chain_ms():
                fresh()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                prior, noised = puct_root_noise(tree, tree["noised"], C, alpha, EPS, SEED, 7, root.first_env_index)
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0), prior, noised
            noise_ms()
            got, done = tree["prior"].clone(), tree["noised"].clone()
            _, prior, noised = chain_ms()
            equal = bool(got.view(torch.int64).equal(prior.view(torch.int64)) and torch.equal(done, noised) and bool((done == 1).all()))
            tn, tc, tt = [], [], []
            for _ in range(a.reps):
                tn.append(noise_ms())
                tc.append(event_ms(lambda: root.puct_move(mreq, _move_lib.MOVE_CHOOSE)))
                tt.append(chain_ms()[0])
            print(json.dumps({
                "config": a.config, "roots": P, "max_children": C, "alpha": alpha, "eps": EPS, "equal": equal, "errors": int(tree["errors_dev"][0]),
                "noise_launch_ms": [round(x, 4) for x in tn], "noise_launch_ms_median": round(med(tn), 4),
                "choose_launch_ms_median": round(med(tc), 4), "noise_over_choose": round(med(tn) / med(tc), 2),
                "torch_chain_ms": [round(x, 2) for x in tt], "torch_chain_ms_median": round(med(tt), 2), "chain_over_launch": round(med(tt) / med(tn), 1)}), flush=True)
    root.close()


if __name__ == "__main__":
    main()
