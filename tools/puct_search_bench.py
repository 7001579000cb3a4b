"""The tree step of the PUCT search on the device (pcbenv_puct_advance) against the same step in torch tensors
(pcbenv.search.puct_search, the specification, on the same device) and against pcbenv_tree_advance, and what of a whole
iteration with pcbenv.search.network_evaluator the tree step is.
python tools/puct_search_bench.py [--roots 4096] [--configs c3 c4] [--iterations 16 64] [--reps 5] [--children 16]

Per case, one JSON line:
  (a) the pcbenv_puct_advance(ABSORB | SELECT) launch by HIP events, averaged over the iterations of a search whose
      evaluations are fixed tensors made beforehand (values from {0.25, 0.5, 0.75}, K = C candidates with seeded priors, a
      leaf terminal at depth T or one time in eight), so that only the tree is timed;
  (b) the same search through puct_search with the same fixed evaluations and the tree on the same device -- wall time
      synchronised at both ends, per iteration: the tensor chain of one tree step -- interleaved with the device search,
      `reps` repeats each after one warm-up of each, and that both grew equal trees; and the pcbenv_tree_advance(ABSORB |
      SELECT) launch at the same P and C, as tools/tree_search_bench.py's launches_ms takes it, in the same process.  The
      two trees differ in shape -- a UCT node is descended through only once it has all its C children, a PUCT node as soon
      as it is expanded -- so each launch comes with the levels its descents took on average, and the PUCT launch is timed
      once more on a search whose nodes below the root are all terminal ("flat": every descent is one level);
  (c) a whole iteration with network_evaluator and constant logits, split by HIP events into the gather
      (pcbenv_gather_paths), top_priors, the playout (pcbenv_playout_paths) and the tree step; and the same iteration with
      the candidates from pcbenv_top_priors (network_evaluator(priors="device")), reported as top_priors_device."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rl-environment-for-component-placement_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import tree_search_bench as tsb  # noqa: E402
from pcbenv import _lib, named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv, default_max_steps  # noqa: E402
from pcbenv.search import Evaluation, new_puct_tree, new_tree, puct_result, puct_search, puct_search_device, top_priors  # noqa: E402

STEP_INDEX, C_PUCT = 1000, 1.25
FIELDS = ("action", "child_visits", "child_actions", "child_priors", "num_nodes", "parent", "depth", "visits", "num_children", "first_child",
          "node_action", "prior", "value_sum", "value_max", "terminal", "reward_lo", "reward_hi")


def fixed_evaluations(P, M, C, dev):
    """M evaluations of P nodes made beforehand: what the tree is fed is the same whichever code keeps it."""
    g = torch.Generator().manual_seed(3)
    out = []
    actions = torch.stack([torch.arange(C) % 2, torch.zeros(C, dtype=torch.int64), torch.arange(C)], dim=1).to(torch.int32)[None].expand(P, C, 3).contiguous()
    for _ in range(M):
        value = (torch.randint(1, 4, (P,), generator=g).to(torch.float64) * 0.25)
        over = (torch.randint(0, 8, (P,), generator=g) == 0).to(torch.uint8)
        prior = torch.softmax(torch.randint(0, 4, (P, C), generator=g).to(torch.float32), dim=1)
        out.append(Evaluation(value.to(dev), over.to(dev), torch.full((P,), C, dtype=torch.int32, device=dev), actions.to(dev), prior.to(dev).contiguous()))
    return out


def replayed(fixed, T):
    """An `evaluate` that hands out the fixed evaluations in order; a node at depth T is terminal whatever the draw said
    (T = 1: the flat search, every node below the root is terminal)."""
    it = iter(fixed)

    def evaluate(paths, path_len, step_index0):
        ev = next(it)
        return Evaluation(ev.value, ev.terminal | (path_len >= T).to(torch.uint8), ev.cand_count, ev.cand_actions, ev.cand_prior)
    return evaluate


def equal_trees(a, b):
    return bool(all(torch.equal(getattr(a, f), getattr(b, f)) for f in FIELDS))  # floats: equal values, no NaN in a tree


def advance_ms(root, fixed, M, T, C, terminal_from=None):
    """The device search with HIP events around every ABSORB | SELECT launch -> (ms per launch, its tree, the levels a
    descent took on average)."""
    P = root.num_envs
    tree = new_puct_tree(P, 1 + M * C, T, root.device)
    req = root.puct_request(tree, C_PUCT, C)
    evaluate = replayed(fixed, T if terminal_from is None else terminal_from)
    levels = torch.zeros((), dtype=torch.float64, device=root.device)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(M)]
    root.puct_advance(req, _lib.TREE_INIT | _lib.TREE_SELECT)
    for m in range(M):
        e = evaluate(tree["paths"], tree["path_len"], 0)
        ev[m][0].record()
        root.puct_advance(req, _lib.TREE_ABSORB | (_lib.TREE_SELECT if m + 1 < M else 0), e.value, e.terminal, e.cand_count, e.cand_actions, e.cand_prior)
        ev[m][1].record()
        levels += tree["path_len"].to(torch.float64).mean() if m + 1 < M else 0.0
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev[:-1]) / max(M - 1, 1), puct_result(tree, C), float(levels) / max(M - 1, 1)


def uct_advance_ms(root, M, T, C):
    """tools/tree_search_bench.py:launches_ms at max_children = C, with the levels a descent took on average ->
    (ms per pcbenv_tree_advance(ABSORB | SELECT) launch, levels)."""
    tree = new_tree(root.num_envs, M + 1, C, T, root.device)
    req = root.tree_request(tree, 1.0)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(M)]
    levels = torch.zeros((), dtype=torch.float64, device=root.device)
    root.tree_advance(req, _lib.TREE_INIT | _lib.TREE_SELECT)
    for m in range(M):
        po = root.playout(k=1, step_index=STEP_INDEX + m * T, paths=tree["paths"], path_len=tree["path_len"], max_steps=T)
        ev[m][0].record()
        root.tree_advance(req, _lib.TREE_ABSORB | (_lib.TREE_SELECT if m + 1 < M else 0), po.reward, po.length, po.actions)
        ev[m][1].record()
        levels += tree["path_len"].to(torch.float64).mean() if m + 1 < M else 0.0
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev[:-1]) / max(M - 1, 1), float(levels) / max(M - 1, 1)


def whole_iteration_ms(root, planner, M, T, C, device_priors=False):
    """puct_search_device with network_evaluator's steps spelled out and HIP events between them -> ms per iteration of
    (gather, top_priors, playout, tree step).  device_priors: the candidates come from planner.top_priors."""
    P, dev = root.num_envs, root.device
    zeros = torch.zeros((P, root.cfg.num_orientations * root.cfg.height * root.cfg.width), dtype=torch.float32, device=dev)
    tree = new_puct_tree(P, 1 + M * C, T, dev)
    req = root.puct_request(tree, C_PUCT, C)
    index = torch.arange(P, dtype=torch.int32, device=dev)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(5)] for _ in range(M)]
    root.puct_advance(req, _lib.TREE_INIT | _lib.TREE_SELECT)
    for m in range(M):
        ev[m][0].record()
        planner.gather_(index, source=root, paths=tree["paths"], path_len=tree["path_len"])
        over = (planner.gather_length > 0) & planner.done.bool()
        ev[m][1].record()
        count, actions, prior = planner.top_priors(zeros, C) if device_priors else top_priors(zeros, planner.obs["action_mask"], C)
        ev[m][2].record()
        leaf = root.playout(k=1, step_index=STEP_INDEX + m * T, paths=tree["paths"], path_len=tree["path_len"], max_steps=T).reward
        value = torch.where(over, planner.reward, leaf)
        ev[m][3].record()
        root.puct_advance(req, _lib.TREE_ABSORB | (_lib.TREE_SELECT if m + 1 < M else 0), value, over.to(torch.uint8), count, actions, prior)
        ev[m][4].record()
    torch.cuda.synchronize()
    return [sum(e[i].elapsed_time(e[i + 1]) for e in ev) / M for i in range(4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--configs", nargs="+", default=["c3", "c4"])
    ap.add_argument("--iterations", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--children", type=int, default=16)
    a = ap.parse_args()
    C = a.children
    med = lambda v: sorted(v)[len(v) // 2]
    for name in a.configs:
        cfg = named_config(name, reward_type="centroid")
        root = BatchedPlacementEnv(cfg, a.roots, queue_depth=1, run_seed=11)
        planner = BatchedPlacementEnv(cfg, a.roots, queue_depth=1, run_seed=11, auto_reset=False)
        for e in (root, planner):
            e.generate_instances()
            e.reset()
        T = default_max_steps(cfg)
        for M in a.iterations:
            fixed = fixed_evaluations(a.roots, M, C, root.device)
            chain = lambda: puct_search(root, M, STEP_INDEX, replayed(fixed, T), c_puct=C_PUCT, max_children=C, max_steps=T)
            device = lambda: puct_search_device(root, M, STEP_INDEX, replayed(fixed, T), c_puct=C_PUCT, max_children=C, max_steps=T)
            _, h = tsb.wall_ms(chain)
            _, d = tsb.wall_ms(device)
            equal = equal_trees(h, d)
            _, ev_tree, levels = advance_ms(root, fixed, M, T, C)
            equal = equal and equal_trees(h, ev_tree)
            _, _, flat_levels = advance_ms(root, fixed, M, T, C, terminal_from=1)
            _, uct_levels = uct_advance_ms(root, M, T, C)
            tc, td, tl, tf, tu = [], [], [], [], []
            for _ in range(a.reps):
                tc.append(tsb.wall_ms(chain)[0])
                td.append(tsb.wall_ms(device)[0])
                tl.append(advance_ms(root, fixed, M, T, C)[0])
                tf.append(advance_ms(root, fixed, M, T, C, terminal_from=1)[0])
                tu.append(uct_advance_ms(root, M, T, C)[0])
            whole_iteration_ms(root, planner, 2, T, C)  # warm-up of its shapes
            parts = whole_iteration_ms(root, planner, M, T, C)
            whole_iteration_ms(root, planner, 2, T, C, device_priors=True)
            parts_dev = whole_iteration_ms(root, planner, M, T, C, device_priors=True)
            print(json.dumps({
                "config": name, "reward_type": "centroid", "roots": a.roots, "iterations": M, "max_children": C, "equal_trees": equal,
                "nodes_in_use_max": int(d.num_nodes.max()), "depth_max": int(d.depth.max()),
                "puct_advance_launch_ms": [round(x, 4) for x in tl], "puct_advance_launch_ms_median": round(med(tl), 4),
                "puct_levels_per_descent": round(levels, 2),
                "puct_advance_flat_launch_ms": [round(x, 4) for x in tf], "puct_advance_flat_launch_ms_median": round(med(tf), 4),
                "puct_flat_levels_per_descent": round(flat_levels, 2),
                "torch_chain_search_ms": [round(x, 2) for x in tc], "torch_chain_ms_per_iteration": round(med(tc) / M, 3),
                "device_search_ms": [round(x, 2) for x in td], "device_search_ms_per_iteration": round(med(td) / M, 4),
                "spread_ms_per_iteration": [round((max(tc) - min(tc)) / M, 4), round((max(td) - min(td)) / M, 4), round(max(tl) - min(tl), 4)],
                "tree_advance_launch_ms": [round(x, 4) for x in tu], "tree_advance_launch_ms_median": round(med(tu), 4),
                "tree_advance_levels_per_descent": round(uct_levels, 2),
                "chain_over_launch": round(med(tc) / M / med(tl), 1),
                "iteration_ms": {"gather": round(parts[0], 4), "top_priors": round(parts[1], 4), "top_priors_device": round(parts_dev[1], 4), "playout": round(parts[2], 4),
                                 "tree_step": round(parts[3], 4)}}), flush=True)
        root.close()
        planner.close()


if __name__ == "__main__":
    main()
