"""Monte-Carlo lookahead over forked episodes: the first consumer of `BatchedPlacementEnv.gather_`.

A caller of the reference forks an episode with `copy.deepcopy(env)`, plays it out and keeps the best try.  Here
`best_of_k` forks every root environment into k children of a planner batch with one device-side gather, plays every
child to the end of its episode with the on-device uniform sampler (one `rollout_step` launch per step) and picks, per
root, the child with the highest terminal reward -- with tensor ops only, no host round trip.  The caller then applies
the best child's first action to the root and searches again from the next state (receding-horizon lookahead).

`best_of_k_playouts` gives the same result without the planner batch: `BatchedPlacementEnv.playout` plays the k forks of
every root in one kernel launch that writes no observation (pcbenv_playout).  `action_values` scores candidate first
actions the same way: k playouts behind each candidate, the forced first action of the playout call.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch


@dataclass
class BestOfK:
    reward: torch.Tensor   # [P] float64: terminal reward of the best child of every root
    child: torch.Tensor    # [P] int64: its index in the planner batch (root p's children are p * k .. p * k + k - 1)
    actions: torch.Tensor  # [T, P, 3] int32: the actions it took, T = max_num_components (rows behind its end: don't care)
    length: torch.Tensor   # [P] int64: steps up to and including its terminal transition
    child_rewards: torch.Tensor  # [P, k] float64: the terminal reward of every child


def child_index(P: int, k: int, device="cpu") -> torch.Tensor:
    """Planner environment i plays root i // k: the gather index arange(P).repeat_interleave(k), int32 [P * k]."""
    return torch.arange(P, dtype=torch.int32, device=device).repeat_interleave(k)


def pick_best(final_reward: torch.Tensor, k: int):
    """Per root, the child with the highest terminal reward (the first such child on ties): (reward [P], planner index [P])."""
    r = final_reward.view(-1, k)
    best = r.argmax(dim=1)
    P = r.shape[0]
    return r.gather(1, best[:, None])[:, 0], torch.arange(P, device=r.device) * k + best


def best_of_k(root, planner, k: int, step_index: int) -> BestOfK:
    """root: P environments; planner: P * k environments of the same definition with auto_reset=False.  Forks every
    root episode k times into the planner (`gather_`), plays every child to its first `done` with the fused sampler
    (draws for steps step_index, step_index + 1, ... -- the children of one root differ by their global environment
    index), and returns the best child per root.  At most max_num_components launches: every transition places a
    component or ends the episode."""
    P = root.num_envs
    if planner.num_envs != P * k:
        raise ValueError(f"the planner needs {P} x {k} = {P * k} environments, it has {planner.num_envs}")
    if planner.auto_reset:
        raise ValueError("the planner must be created with auto_reset=False (a child's episode ends at its first done)")
    dev, n = planner.device, planner.num_envs
    planner.gather_(child_index(P, k, dev), source=root)
    T = root.cfg.max_num_components
    actions = torch.zeros((T, n, 3), dtype=torch.int32, device=dev)
    final = torch.zeros(n, dtype=torch.float64, device=dev)
    length = torch.zeros(n, dtype=torch.int64, device=dev)
    finished = torch.zeros(n, dtype=torch.bool, device=dev)
    for t in range(T):
        _, r, d, _, _ = planner.rollout_step(step_index + t, out=actions[t])
        first = d.bool() & ~finished
        final = torch.where(first, r, final)
        length = torch.where(first, torch.full_like(length, t + 1), length)
        finished |= first
    reward, child = pick_best(final, k)
    return BestOfK(reward, child, actions[:, child], length[child], final.view(P, k))


def select_best(final_reward: torch.Tensor, length: torch.Tensor, actions: torch.Tensor, k: int) -> BestOfK:
    """The tensor half of a best-of-k search (any device): per-child terminal rewards [P * k], lengths [P * k] and actions
    [T, P * k, 3] -> the best child per root, its actions and length, and every child's reward as [P, k]."""
    reward, child = pick_best(final_reward, k)
    return BestOfK(reward, child, actions[:, child], length.to(torch.int64)[child], final_reward.view(-1, k))


def best_of_k_playouts(root, k: int, step_index: int) -> BestOfK:
    """`best_of_k(root, planner, k, step_index)` for a planner with the root's run_seed and first_env_index = 0, without the
    planner: one `root.playout` launch plays the k forks of every root to their end (the same draws, the same
    transitions), and the selection is the same.  Same fields, same values; `actions` rows behind a child's end are zero."""
    po = root.playout(k=k, step_index=step_index, max_steps=root.cfg.max_num_components)
    return select_best(po.reward, po.length, po.actions, k)


@dataclass
class ActionValues:
    mean: torch.Tensor       # [P, A] float64: mean playout reward behind every candidate
    max: torch.Tensor        # [P, A] float64: the best playout reward behind every candidate
    cut_share: torch.Tensor  # 0-dim float64: the share of playouts that were cut before their episode ended


def aggregate_values(reward: torch.Tensor, done: torch.Tensor, P: int, A: int, k: int) -> ActionValues:
    """The tensor half of `action_values` (any device): playout rewards and done flags [P * A * k], playout
    (p * A + a) * k + j being try j of candidate a of root p."""
    r = reward.view(P, A, k)
    return ActionValues(r.mean(dim=2), r.max(dim=2).values, (done == 0).to(torch.float64).mean())


def action_values(root, candidates: torch.Tensor, k: int, step_index: int, max_steps=None) -> ActionValues:
    """Monte-Carlo values of candidate first actions: candidates int32 [P, A, 3]; behind candidate a of root p run k playouts
    that take it as their first action and draw uniformly afterwards (one `root.playout` launch of P * A * k playouts).
    The value is the playouts' final reward (pin kinds: the terminal routing reward; an illegal candidate gives the
    worst-case reward).  Returns the mean and the max per candidate and the share of playouts cut at max_steps."""
    P = root.num_envs
    if candidates.dim() != 3 or candidates.shape[0] != P or candidates.shape[2] != 3:
        raise ValueError(f"candidates must have shape [{P}, A, 3], got {list(candidates.shape)}")
    A = candidates.shape[1]
    first = candidates.to(device=root.device, dtype=torch.int32).repeat_interleave(k, dim=1).reshape(P * A * k, 3)
    po = root.playout(k=A * k, step_index=step_index, first_actions=first, max_steps=max_steps, actions_steps=0)
    return aggregate_values(po.reward, po.done, P, A, k)
