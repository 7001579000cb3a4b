"""Monte-Carlo lookahead over forked episodes: the first consumer of `BatchedPlacementEnv.gather_`.

A caller of the reference forks an episode with `copy.deepcopy(env)`, plays it out and keeps the best try.  Here
`best_of_k` forks every root environment into k children of a planner batch with one device-side gather, plays every
child to the end of its episode with the on-device uniform sampler (one `rollout_step` launch per step) and picks, per
root, the child with the highest terminal reward -- with tensor ops only, no host round trip.  The caller then applies
the best child's first action to the root and searches again from the next state (receding-horizon lookahead).
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
