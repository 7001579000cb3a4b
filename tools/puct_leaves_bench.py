"""The leaf-parallel tree step (pcbenv_puct_advance_leaves) against pcbenv_puct_advance, and what a fixed budget of
evaluations costs when it is spent L leaves at a time.
python tools/puct_leaves_bench.py [--roots 4096] [--children 16] [--leaves 1 2 4 8 16] [--launches 8] [--reps 5] [--search-roots 256] [--config c3]

One JSON line each:
  (a) the tree step.  A device search of 64 evaluations (L = 1, evaluations fixed beforehand as tools/puct_search_bench.py
      makes them) leaves P trees; every timed run starts from a copy of them in tensors of one capacity.  Timed by HIP events:
      `launches` consecutive ABSORB | SELECT launches, each absorbing fixed evaluations of the rows the launch before
      selected; the median over launches and `reps` runs, per launch and per real leaf.  The baseline is pcbenv_puct_advance
      on the same trees in the same process, run first, between the L and last: the spread of its medians is the
      run-to-run spread an L = 1 figure is to be read against.
  (b) the search.  `--search-roots` roots of `--config`, network_evaluator(priors="device") with constant logits and a
      uniform rollout for a value, 64 evaluations per move as L x iterations = 1 x 64, 4 x 16, 8 x 8, 16 x 4: wall time of
      puct_search_device, synchronised at both ends, per real leaf (the sum of the roots' visits), and the share of the
      P * L * iterations rows that were no leaf."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rl-environment-for-component-placement_amd"))
import torch  # noqa: E402

from pcbenv import _lib, named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv, default_max_steps  # noqa: E402
from pcbenv.search import PUCT_TREE_TENSORS, Evaluation, network_evaluator, new_puct_tree, puct_search_device  # noqa: E402

C_PUCT, GROWN = 1.25, 64
AS = _lib.TREE_ABSORB | _lib.TREE_SELECT


def fixed_evaluations(rows, M, C, dev, seed=3):
    """M evaluations of `rows` nodes made beforehand (tools/puct_search_bench.py:fixed_evaluations)."""
    g = torch.Generator().manual_seed(seed)
    actions = torch.stack([torch.arange(C) % 2, torch.zeros(C, dtype=torch.int64), torch.arange(C)], dim=1).to(torch.int32)[None].expand(rows, C, 3).contiguous().to(dev)
    out = []
    for _ in range(M):
        value = torch.randint(1, 4, (rows,), generator=g).to(torch.float64) * 0.25
        over = (torch.randint(0, 8, (rows,), generator=g) == 0).to(torch.uint8)
        prior = torch.softmax(torch.randint(0, 4, (rows, C), generator=g).to(torch.float32), dim=1)
        out.append(Evaluation(value.to(dev), over.to(dev), torch.full((rows,), C, dtype=torch.int32, device=dev), actions, prior.to(dev).contiguous()))
    return out


def grown_trees(root, T, C):
    """The trees a search of GROWN evaluations leaves (L = 1)."""
    it = iter(fixed_evaluations(root.num_envs, GROWN, C, root.device))

    def evaluate(paths, path_len, s):
        ev = next(it)
        return Evaluation(ev.value, ev.terminal | (path_len >= T).to(torch.uint8), ev.cand_count, ev.cand_actions, ev.cand_prior)
    ps = puct_search_device(root, GROWN, 0, evaluate, c_puct=C_PUCT, max_children=C, max_steps=T)
    return {n: getattr(ps, n) for n in PUCT_TREE_TENSORS}


def timed_launches(root, grown, N, T, C, L, fixed):
    """One run: the grown trees copied into tensors of capacity N, SELECT, then len(fixed) timed ABSORB | SELECT launches.
    L = 0: pcbenv_puct_advance.  -> (ms of every launch, the real leaves each absorbed on average per root)."""
    P, dev = root.num_envs, root.device
    tree = new_puct_tree(P, N, T, dev, max(L, 1))
    advance = root.puct_advance if L == 0 else root.puct_advance_leaves
    req = root.puct_request(tree, C_PUCT, C) if L == 0 else root.puct_leaves_request(tree, C_PUCT, C, L)
    advance(req, _lib.TREE_INIT)
    n = grown["parent"].shape[1]
    for f in PUCT_TREE_TENSORS:
        (tree[f] if grown[f].dim() == 1 else tree[f][:, :n]).copy_(grown[f].to(tree[f].dtype))
    advance(req, _lib.TREE_SELECT)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in fixed]
    real = torch.zeros((), dtype=torch.float64, device=dev)
    for m, e in enumerate(fixed):
        real += (tree["path_len"] >= 0).to(torch.float64).sum()
        over = e.terminal | (tree["path_len"] >= T).to(torch.uint8)
        ev[m][0].record()
        advance(req, AS, e.value, over, e.cand_count, e.cand_actions, e.cand_prior)
        ev[m][1].record()
    torch.cuda.synchronize()
    assert int(tree["errors_dev"][0]) == 0
    return [a.elapsed_time(b) for a, b in ev], float(real) / len(fixed) / P


def tree_step(a):
    cfg = named_config("c3")
    root = BatchedPlacementEnv(cfg, a.roots, queue_depth=1, run_seed=11)  # the handle gives the device and T only
    T, C, P = default_max_steps(cfg), a.children, a.roots
    grown = grown_trees(root, T, C)
    N = 1 + GROWN * C + (a.launches + 1) * max(a.leaves) * C
    med = lambda v: sorted(v)[len(v) // 2]
    fixed = {L: fixed_evaluations(P * max(L, 1), a.launches, C, root.device, seed=5) for L in [0] + a.leaves}

    def run(L):
        timed_launches(root, grown, N, T, C, L, fixed[L])  # warm-up
        ms, leaves = [], 0.0
        for _ in range(a.reps):
            t, leaves = timed_launches(root, grown, N, T, C, L, fixed[L])
            ms += t
        return med(ms), leaves
    base = [run(0)[0]]
    out = {}
    for L in a.leaves:
        out[L] = run(L)
        base.append(run(0)[0])
    b = med(base)
    print(json.dumps({
        "what": "tree_step", "roots": P, "max_children": C, "max_steps": T, "grown_by_evaluations": GROWN, "nodes_in_use_max": int(grown["num_nodes"].max()),
        "capacity": N, "launches": a.launches, "reps": a.reps,
        "puct_advance_launch_ms": [round(x, 4) for x in base], "puct_advance_launch_ms_median": round(b, 4),
        "puct_advance_spread_ms": round(max(base) - min(base), 4),
        "leaves": {str(L): {"launch_ms": round(ms, 4), "real_leaves_per_root": round(n, 2), "ms_per_leaf": round(ms / max(n, 1e-9), 4),
                            "per_leaf_over_puct_advance": round(ms / max(n, 1e-9) / b, 3)} for L, (ms, n) in out.items()}}), flush=True)
    root.close()


def search(a):
    cfg = named_config(a.config)
    P, T, C = a.search_roots, default_max_steps(cfg), a.children
    for L, M in ((1, 64), (4, 16), (8, 8), (16, 4)):
        def make(n):
            e = BatchedPlacementEnv(cfg, n, queue_depth=1, run_seed=11)
            e.generate_instances()
            e.reset()
            return e
        root, planner = make(P), make(P * L)
        zeros = torch.zeros((P * L, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=root.device)
        evaluate = network_evaluator(root, planner, lambda obs: zeros, max_children=C, priors="device", leaves=L)
        go = lambda: puct_search_device(root, M, 1000, evaluate, c_puct=C_PUCT, max_children=C, max_steps=T, leaves=L)
        go()
        wall, real = [], 0
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ps = go()
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
            real = int(ps.visits[:, 0].sum())
        w = sorted(wall)[len(wall) // 2]
        print(json.dumps({"what": "search", "config": a.config, "roots": P, "max_children": C, "leaves": L, "iterations": M, "rows": P * L * M,
                          "real_leaves": real, "repeat_share": round(1.0 - real / (P * L * M), 4), "search_ms": [round(x, 3) for x in wall],
                          "ms_per_iteration": round(w / M, 4), "us_per_real_leaf": round(1e3 * w / max(real, 1), 4),
                          "tree_errors": int(ps.errors)}), flush=True)
        root.close()
        planner.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--children", type=int, default=16)
    ap.add_argument("--leaves", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--search-roots", type=int, default=256)
    ap.add_argument("--config", default="c3")
    a = ap.parse_args()
    tree_step(a)
    search(a)


if __name__ == "__main__":
    main()
