"""Receding-horizon Monte-Carlo lookahead with pcbenv.search.best_of_k against the plain uniform-random policy, c3.
python tools/search_demo.py [--roots 256] [--k 16] [--seed 11] [--playouts | --tree [--device-tree] [--policy] | --puct [--device-priors] [--reuse] [--leaves L] [--noise ALPHA EPS | --gumbel M [--leaves L] [--gumbel-full]] [--capacity N] [--train N [--moves M] [--torch-loss]] | --frontier W [--prior-weight X | --stochastic] [--device-priors]]

Both play the same instances (one episode per root environment).  The search forks every root k times into a planner
batch (one device-side gather), plays every child to its end with the on-device sampler, and applies the best child's
first action to the root, then searches again.  --playouts: the same search through pcbenv.search.best_of_k_playouts --
one pcbenv_playout launch per search step instead of a planner batch and a launch per planner step.  Reports mean final reward of both policies and the search rate in
planner env-steps/s (wall time of the best_of_k calls).  --tree: pcbenv.search.tree_search with k iterations per move -- the
same number of playouts as best-of-k, spent by UCT on a tree of paths (one pcbenv_playout_paths launch per iteration) -- and
the most-visited first action is applied.  --tree --device-tree: the same search through pcbenv.search.tree_search_device, the
tree kept by the device (pcbenv_tree_advance): two launches per iteration.  --tree --policy (a spatial configuration:
--config c4): the rollout behind every path is played by a policy instead of the uniform draw -- pcbenv.search.policy_backend
materialises the nodes in a planner batch (pcbenv_gather_paths) and draws from the logits of pcbenv/policy.py's model with
its initial weights (seeded, untrained: the demo shows the plumbing, not a trained policy's strength).  --puct:
pcbenv.search.puct_search_device with k iterations per move -- the tree kept by the device (pcbenv_puct_advance), a node
expanded with the 16 most probable legal actions of pcbenv.search.network_evaluator (constant logits: uniform priors) and
scored by one uniform rollout from it; the most-visited first action is applied.  --puct --reuse: the same search through
pcbenv.search.puct_selfplay -- the tree stays on the device from move to move: pcbenv_puct_move picks the most-visited
action and makes its subtree the next move's tree, so the k iterations of a move add to the visits already spent below it;
the line then also reports the mean visits a move's root started with.  --puct --leaves L: every iteration selects L leaves
per root (pcbenv_puct_advance_leaves) and the evaluator sees roots x L nodes at once; k stays the iterations per move, so a
move costs k x L evaluations.  --puct --noise ALPHA EPS: exploration noise on the root's priors, once per root and move
(pcbenv_puct_root_noise: a draw from Dir(ALPHA) mixed in with weight EPS); with --reuse the line also reports the share of
the 16 child entries of a move's root that got no visit (entries behind the root's children included).  --puct --gumbel M:
the root level of every search is a Gumbel search (pcbenv_gumbel_advance): k simulations per move, k + 1 evaluations, spent by
Sequential Halving over M candidates, c_visit 50 and c_scale 1; the move is the best of the most-simulated children, and with
--reuse the policy target is softmax(logit + sigma(completed q)), whose entries without weight zero_visit_share then counts.
--puct --gumbel M --leaves L: up to L simulations of a root per launch (pcbenv_gumbel_advance_leaves): a move is k simulations in
ceil(k / L) + 1 evaluations of roots x L rows; the line then also reports the rows that were leaves, their cost, the share of
rows that were none (-1: behind a repeat or the end of the budget) and, with --reuse, the share of searched roots that finished
their schedule (sim_index == k).
--puct --gumbel M --gumbel-full: the full Gumbel rule (pcbenv_gumbel_tree_advance): below the root the search goes to the argmax of
pi' - n / (1 + sum n) in the place of PUCT, and a child without a visit is completed with v_mix.  With --leaves L the launches
are pcbenv_gumbel_tree_advance_leaves' (node_rule="gumbel"): the same rule with a pending visit counted as a visit.
--puct --capacity N: node slots per root in the place of the search's default; tree_errors (with --reuse) has bit 0 set if some
expansion found no room (ERR_FULL), so 0 says that no root met it.
--puct --train N (a spatial configuration: --config
c4): N rounds of pcbenv.alphazero.AlphaZeroTrainer -- collect() plays --moves moves of every root with puct_selfplay, k
iterations each, pcbenv/policy.py's model behind network_evaluator(priors="device"); update() trains the model on the visit
counts with pcbenv_evaluate_visits (--torch-loss: the torch chain instead) -- and one line per round: the mean final reward
of the episodes that ended in the round and the mean cross entropy of the update.
--frontier W: a beam search over placements (pcbenv.search.frontier_search_device: one pcbenv_frontier_advance launch per depth next
to the evaluation), ONE search per episode: a frontier of W partial placements per root, each expanded by the k most probable
legal actions of network_evaluator (constant logits; --device-priors: pcbenv_top_priors) and scored by one uniform rollout from
it, plus --prior-weight X times its cumulative log-prior.  The plan found, best_path, is then played with `step`.  The line
reports the mean final reward, the rows evaluated and the time per episode, and that every played plan ended with the
best_value the search reported for it.
--frontier W --stochastic: the same search with the rows ordered by Gumbel-perturbed log-probabilities
(pcbenv.search.frontier_sample_search_device, one pcbenv_frontier_sample launch per depth): W complete placements per root
sampled without replacement from the evaluator's priors under --seed.  The entry with the largest value is played; the line
reports its mean reward, the mean reward over all entries and the distinct plans per root.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rl-environment-for-component-placement_amd"))
import torch  # noqa: E402

from pcbenv import named_config  # noqa: E402
from pcbenv.batched_env import BatchedPlacementEnv  # noqa: E402
from pcbenv.config import KIND_SPATIAL  # noqa: E402
from pcbenv.search import (best_of_k, best_of_k_playouts, frontier_sample_search_device, frontier_search_device, gumbel_search_device, network_evaluator, policy_backend, puct_search_device, puct_selfplay, tree_search,  # noqa: E402
                           tree_search_device)


def final_rewards(env, act, T):
    """Steps every root until its first done; `act(t)` issues step t and returns (reward, done)."""
    final = torch.zeros(env.num_envs, dtype=torch.float64, device=env.device)
    finished = torch.zeros(env.num_envs, dtype=torch.bool, device=env.device)
    for t in range(T):
        r, d = act(t)
        first = d.bool() & ~finished
        final = torch.where(first, r, final)
        finished |= first
    assert bool(finished.all())
    return final


def train(a, cfg):
    """--puct --train N: one JSON line per collect/update round."""
    from pcbenv.alphazero import AlphaZeroConfig, AlphaZeroTrainer
    from pcbenv.policy import SpatialPolicy
    moves = a.moves or cfg.max_num_components
    episodes = -(-a.train * moves // cfg.max_num_components) + 1  # per root: one instance record each
    root = BatchedPlacementEnv(cfg, a.roots, queue_depth=episodes, run_seed=11, auto_reset=True)
    root.generate_instances()
    root.reset()
    planner = BatchedPlacementEnv(cfg, a.roots * a.leaves, queue_depth=1, run_seed=11)
    planner.generate_instances()
    planner.reset()
    torch.manual_seed(0)
    trainer = AlphaZeroTrainer(root, planner, SpatialPolicy(cfg).to(root.device),
                               AlphaZeroConfig(moves=moves, iterations=a.k, max_children=16, capacity=1 + moves * (a.k + 1) * a.leaves * 16, device_loss=not a.torch_loss,
                                               leaves=a.leaves, noise_alpha=a.noise[0] if a.noise else None, noise_eps=a.noise[1] if a.noise else 0.25,
                                               gumbel_considered=a.gumbel, gumbel_node_rule="gumbel" if a.gumbel_full else "puct"))
    for it in range(a.train):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch = trainer.collect()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        stats = trainer.update(batch)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        over = batch["done"].bool()
        print(json.dumps({"round": it, "episodes_ended": int(over.sum()),
                          "mean_final_reward": float(batch["reward"][over].mean()) if bool(over.any()) else None,
                          "mean_cross_entropy": round(stats["policy"], 4), "value_loss": round(stats["value"], 4),
                          "policy_entropy": round(stats["entropy"], 4), "tree_errors": int(batch["errors"]),
                          "collect_s": round(t1 - t0, 3), "update_s": round(t2 - t1, 3)}), flush=True)
    root.close()
    planner.close()


def stochastic_frontier(a, root, fs, rows, spent, random_final, no_action, envs):
    """--frontier W --stochastic: the entry of a root's sample with the largest value is played; one JSON line."""
    P, W, T = a.roots, a.frontier, fs.set_path.shape[0]
    n, value = fs.set_len.view(P, W), fs.set_value.view(P, W)
    held = n >= 1
    ninf = torch.full_like(value, float("-inf"))
    best = torch.where(held, value, ninf).argmax(dim=1)                                  # [P]: the slot played
    at = torch.arange(P, device=n.device)
    plan_len, plan = n[at, best], fs.set_path.view(T, P, W, 3)[:, at, best]              # [P], [T, P, 3]

    def play(t):
        _, r, d, _ = root.step(torch.where((plan_len <= t)[:, None], no_action, plan[t]))
        return r, d
    final = final_rewards(root, play, T)
    planned = plan_len >= 1
    paths = fs.set_path.view(T, P, W, 3).permute(1, 2, 0, 3).cpu().numpy()
    lens = n.cpu().numpy()
    distinct = [len({paths[p, j, :lens[p, j]].tobytes() for j in range(W) if lens[p, j] >= 1}) for p in range(P)]
    entries = int(held.sum())
    out = {"config": a.config, "roots": P, "frontier": W, "k": a.k, "stochastic": True, "seed": a.seed,
           "search": "frontier_sample_search_device+network_evaluator" + ("(priors=device)" if a.device_priors else ""),
           "random_policy_mean_final_reward": float(random_final.mean()), "frontier_mean_final_reward": float(final.mean()),
           "mean_best_reward": float(torch.where(held, value, ninf).max(dim=1).values[planned].mean()) if bool(planned.any()) else None,
           "mean_set_reward": float(value[held].mean()) if entries else None, "set_entries_per_root": round(entries / P, 3),
           "distinct_plans_per_root": round(sum(distinct) / P, 3), "every_entry_is_a_distinct_plan": sum(distinct) == entries,
           "roots_with_a_plan": int(planned.sum()), "every_plan_reproduced_its_value": bool((final[planned] == value[at, best][planned]).all()),
           "evaluated_rows_per_episode": round(int(rows) / P, 2), "us_per_evaluated_row": round(1e6 * spent / max(int(rows), 1), 3),
           "search_seconds": round(spent, 3), "seconds_per_episode": round(spent / P, 6), "frontier_errors": int(fs.errors)}
    print(json.dumps(out), flush=True)
    for e in envs:
        e.close()


def frontier(a, cfg):
    """--frontier W: one search per episode and its plan played; one JSON line."""
    P, W, K, T = a.roots, a.frontier, a.k, cfg.max_num_components

    def make(n):
        e = BatchedPlacementEnv(cfg, n, queue_depth=1, run_seed=a.seed)
        e.generate_instances()
        e.reset()
        return e
    rand_root, root, planner = make(P), make(P), make(P * W * K)
    dev = root.device
    zeros = torch.zeros((P * W * K, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=dev)
    scored = network_evaluator(root, planner, lambda obs: zeros, max_children=K, priors="device" if a.device_priors else "torch", leaves=W * K)
    rows = torch.zeros((), dtype=torch.int64, device=dev)

    def evaluate(paths, path_len, step_index0):
        rows.add_((path_len >= 0).sum())
        return scored(paths, path_len, step_index0)
    random_final = final_rewards(rand_root, lambda t: rand_root.rollout_step(t)[1:3], T)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if a.stochastic:
        fs = frontier_sample_search_device(root, evaluate, W, K, 1000, seed=a.seed)
    else:
        fs = frontier_search_device(root, evaluate, W, K, 1000, prior_weight=a.prior_weight)
    torch.cuda.synchronize()
    spent = time.perf_counter() - t0
    no_action = torch.full((P, 3), -1, dtype=torch.int32, device=dev)
    if a.stochastic:
        return stochastic_frontier(a, root, fs, rows, spent, random_final, no_action, (rand_root, root, planner))

    def play(t):  # past its plan, or without one: an action that is no action ends the episode as it stands
        _, r, d, _ = root.step(torch.where((fs.best_len <= t)[:, None], no_action, fs.best_path[t]))
        return r, d
    final = final_rewards(root, play, T)
    planned = fs.best_len >= 1
    out = {"config": a.config, "roots": P, "frontier": W, "k": K, "prior_weight": a.prior_weight,
           "search": "frontier_search_device+network_evaluator" + ("(priors=device)" if a.device_priors else ""),
           "random_policy_mean_final_reward": float(random_final.mean()), "frontier_mean_final_reward": float(final.mean()),
           "roots_with_a_plan": int(planned.sum()), "every_plan_reproduced_its_best_value": bool((final[planned] == fs.best_value[planned]).all()),
           "evaluated_rows_per_episode": round(int(rows) / P, 2), "us_per_evaluated_row": round(1e6 * spent / max(int(rows), 1), 3),
           "search_seconds": round(spent, 3), "seconds_per_episode": round(spent / P, 6), "frontier_errors": int(fs.errors)}
    if a.seed != 11:
        out["seed"] = a.seed
    print(json.dumps(out), flush=True)
    for e in (rand_root, root, planner):
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=256)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--config", default="c3")
    ap.add_argument("--seed", type=int, default=11, help="the run seed of the root environments: other instances, other draws")
    ap.add_argument("--playouts", action="store_true", help="search with best_of_k_playouts (no planner batch)")
    ap.add_argument("--tree", action="store_true", help="search with tree_search, k iterations per move (no planner batch)")
    ap.add_argument("--device-tree", action="store_true", help="with --tree: tree_search_device (the tree on the device)")
    ap.add_argument("--policy", action="store_true", help="with --tree: rollouts by pcbenv/policy.py's model (initial weights) through policy_backend")
    ap.add_argument("--puct", action="store_true", help="search with puct_search_device, k iterations per move, network_evaluator with constant logits")
    ap.add_argument("--device-priors", action="store_true", help="with --puct: the candidates from pcbenv_top_priors (network_evaluator(priors=\"device\"))")
    ap.add_argument("--reuse", action="store_true", help="with --puct: puct_selfplay, the subtree of the move played is kept (pcbenv_puct_move)")
    ap.add_argument("--leaves", type=int, default=1, metavar="L", help="with --puct: L leaves per root and iteration (pcbenv_puct_advance_leaves); k stays the iterations per move")
    ap.add_argument("--noise", type=float, nargs=2, default=None, metavar=("ALPHA", "EPS"), help="with --puct: Dir(ALPHA) noise of weight EPS on the root's priors (pcbenv_puct_root_noise)")
    ap.add_argument("--gumbel", type=int, default=None, metavar="M", help="with --puct: Gumbel root search, Sequential Halving over M candidates (pcbenv_gumbel_advance)")
    ap.add_argument("--gumbel-full", action="store_true", help="with --gumbel: the non-root rule and v_mix of the paper as well (pcbenv_gumbel_tree_advance; with --leaves pcbenv_gumbel_tree_advance_leaves)")
    ap.add_argument("--capacity", type=int, default=None, metavar="N", help="with --puct: node slots per root (default: the search's own)")
    ap.add_argument("--train", type=int, default=0, metavar="N", help="with --puct: N collect/update rounds of pcbenv.alphazero.AlphaZeroTrainer")
    ap.add_argument("--moves", type=int, default=0, help="with --train: moves of every root per round (default: one episode)")
    ap.add_argument("--torch-loss", action="store_true", help="with --train: the policy loss through the torch chain (device_loss off)")
    ap.add_argument("--frontier", type=int, default=None, metavar="W", help="a beam search over placements, W rows per root and k candidates per row, one search per episode (frontier_search_device)")
    ap.add_argument("--prior-weight", type=float, default=0.0, metavar="X", help="with --frontier: the weight of a row's cumulative log-prior in its score")
    ap.add_argument("--stochastic", action="store_true", help="with --frontier: a stochastic beam search (frontier_sample_search_device), W plans per root sampled without replacement under --seed; the best of them is played")
    a = ap.parse_args()
    if a.stochastic and (a.frontier is None or a.prior_weight != 0.0):
        ap.error("--stochastic goes with --frontier and without --prior-weight")
    if a.train and not a.puct:
        ap.error("--train goes with --puct")
    if a.frontier is not None and (a.puct or a.tree or a.playouts or a.train):
        ap.error("--frontier goes alone")
    if a.prior_weight != 0.0 and a.frontier is None:
        ap.error("--prior-weight goes with --frontier")
    if a.device_priors and not a.puct and a.frontier is None:
        ap.error("--device-priors goes with --puct or --frontier")
    if a.reuse and not a.puct:
        ap.error("--reuse goes with --puct")
    if a.leaves != 1 and not a.puct:
        ap.error("--leaves goes with --puct")
    if a.noise and not a.puct:
        ap.error("--noise goes with --puct")
    if a.gumbel_full and a.gumbel is None:
        ap.error("--gumbel-full goes with --gumbel")
    if a.capacity is not None and not a.puct:
        ap.error("--capacity goes with --puct")
    if a.gumbel is not None and (not a.puct or a.noise):
        ap.error("--gumbel goes with --puct, without --noise")
    if a.puct and (a.tree or a.playouts):
        ap.error("--puct goes alone")
    if a.device_tree and not a.tree:
        ap.error("--device-tree goes with --tree")
    if a.policy and not a.tree:
        ap.error("--policy goes with --tree")
    cfg = named_config(a.config)
    if a.policy and cfg.kind != KIND_SPATIAL:
        ap.error("--policy needs a spatial configuration, the one pcbenv/policy.py's model reads (--config c4)")
    P, k, T = a.roots, a.k, cfg.max_num_components
    if a.frontier is not None:
        return frontier(a, cfg)
    if a.train:
        if cfg.kind != KIND_SPATIAL:
            ap.error("--train needs a spatial configuration, the one pcbenv/policy.py's model reads (--config c4)")
        return train(a, cfg)

    def make(n, seed):
        e = BatchedPlacementEnv(cfg, n, queue_depth=1, run_seed=seed)
        e.generate_instances()
        e.reset()
        return e
    rand_root, search_root = make(P, a.seed), make(P, a.seed)
    planner = make(P * a.leaves, a.seed) if a.puct else make(P, a.seed) if a.policy else None if a.playouts or a.tree else make(P * k, a.seed + 1)  # (policy_backend, network_evaluator: the root's run seed)
    backend = None
    if a.puct:
        zeros = torch.zeros((P * a.leaves, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=search_root.device)
        evaluate = network_evaluator(search_root, planner, lambda obs: zeros, max_children=16, priors="device" if a.device_priors else "torch", leaves=a.leaves)
        leaf_rows, all_rows = torch.zeros((), dtype=torch.int64, device=search_root.device), [0]  # rows evaluated that were leaves, rows in all
        counted = evaluate

        def evaluate(paths, path_len, step_index0):
            all_rows[0] += path_len.numel()
            if a.leaves != 1:  # with one leaf every row is one: nothing is counted on the device
                leaf_rows.add_((path_len >= 0).sum())
            return counted(paths, path_len, step_index0)
    if a.policy:
        from pcbenv.policy import SpatialPolicy
        torch.manual_seed(0)
        model = SpatialPolicy(cfg).to(search_root.device).eval()

        def logits_fn(obs):
            with torch.no_grad():
                return model(obs, mask=False)[0].contiguous()
        backend = policy_backend(search_root, planner, logits_fn)

    random_final = final_rewards(rand_root, lambda t: rand_root.rollout_step(t)[1:3], T)
    torch.cuda.synchronize()
    spent, planner_steps = 0.0, 0

    def search_step(t):
        nonlocal spent, planner_steps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if a.puct and a.gumbel is not None:
            first = gumbel_search_device(search_root, k, 1000 + t * T * (-(-k // a.leaves) + 1), evaluate, max_considered=a.gumbel, max_children=16,
                                         gumbel_step_index=1000 + t, leaves=a.leaves, node_rule="gumbel" if a.gumbel_full else "puct", capacity=a.capacity).move_action
        elif a.puct:
            first = puct_search_device(search_root, k, 1000 + t * T * k, evaluate, max_children=16, leaves=a.leaves, root_noise=a.noise, capacity=a.capacity).action
        elif a.tree:
            first = (tree_search_device if a.device_tree else tree_search)(search_root, k, step_index=1000 + t * T * k, backend=backend).action
        elif a.playouts:
            res = best_of_k_playouts(search_root, k, step_index=1000 + t * T)
        else:
            res = best_of_k(search_root, planner, k, step_index=1000 + t * T)
        torch.cuda.synchronize()
        spent += time.perf_counter() - t0
        planner_steps += P * k * a.leaves * T
        _, r, d, _ = search_root.step(first if a.tree or a.puct else res.actions[0])
        return r, d
    kept = None
    if a.reuse:
        finished = torch.zeros(2, dtype=torch.int64, device=search_root.device)  # searched roots that finished their schedule, searched roots

        def on_move(j, tree):
            if a.gumbel is not None:
                finished[0] += (tree["sim_index"] == k).sum()
                finished[1] += (tree["sim_index"] > 0).sum()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sp = puct_selfplay(search_root, evaluate, T, k, step_index=1000, max_children=16, leaves=a.leaves, root_noise=a.noise,
                           gumbel=None if a.gumbel is None else (a.gumbel, 50.0, 1.0), on_move=on_move, gumbel_node_rule="gumbel" if a.gumbel_full else "puct", capacity=a.capacity)
        torch.cuda.synchronize()
        spent, planner_steps = time.perf_counter() - t0, P * k * a.leaves * T * T
        search_final = final_rewards(search_root, lambda t: (sp.reward[t], sp.done[t]), T)
        kept = {"mean_visits_kept_per_move": round(float(sp.kept_visits[:-1].double().mean()), 2), "tree_errors": int(sp.errors)}
        searched = sp.child_visits.sum(dim=2) > 0
        kept["zero_visit_share"] = round(float((sp.child_visits[searched] == 0).double().mean()), 4)
        if a.gumbel is not None:
            kept["finished_schedule_share"] = round(int(finished[0]) / max(int(finished[1]), 1), 4)
    else:
        search_final = final_rewards(search_root, search_step, T)
    out = {"config": a.config, "roots": P, "k": k, "search": ("puct_selfplay" if a.reuse else "puct_search_device") + "+network_evaluator" + ("(priors=device)" if a.device_priors else "") if a.puct else ("tree_search_device" if a.device_tree else "tree_search") + ("+policy_backend" if a.policy else "") if a.tree else "best_of_k_playouts" if a.playouts else "best_of_k",
           "random_policy_mean_final_reward": float(random_final.mean()),
           "best_of_k_mean_final_reward": float(search_final.mean()),
           "search_env_steps_per_sec": round(planner_steps / spent), "search_seconds": round(spent, 3)}
    out.update(kept or {})
    if a.leaves != 1:
        out["leaves"] = a.leaves
    if a.noise:
        out["noise"] = a.noise
    if a.gumbel is not None:
        out["gumbel"] = a.gumbel
    if a.gumbel_full:
        out["gumbel_full"] = True
    if a.seed != 11:
        out["seed"] = a.seed
    if a.capacity is not None:
        out["capacity"] = a.capacity
    if a.puct:
        total = all_rows[0]
        leaves = int(leaf_rows) if a.leaves != 1 else total
        out.update(evaluated_leaves=leaves, us_per_evaluated_leaf=round(1e6 * spent / max(leaves, 1), 3), no_leaf_share=round(1.0 - leaves / max(total, 1), 4))
    out["seconds_per_move"] = round(spent / T, 4)
    print(json.dumps(out), flush=True)
    for e in (rand_root, search_root, planner):
        if e is not None:
            e.close()


if __name__ == "__main__":
    main()
