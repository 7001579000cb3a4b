"""A compact AlphaZero loop around the device-resident search: self-play with `puct_selfplay` -- the tree on the device,
the network behind `network_evaluator(priors="device")` -- collects the training targets `pcbenv_puct_move` writes, and the
update trains the network on them: the cross entropy of its masked policy against the visit counts of every move's root
(`visit_targets.cross_entropy`: one kernel launch forward, one backward, with `device_loss`), the squared error of its
value against the final reward of the move's episode, and an entropy bonus.

Everything stays on the GPU and `collect` makes no host synchronisation: the root observations and bit-packed legal sets
are copied per move, the targets are `SelfPlay`'s rows, the value targets a reverse scan over `done`.  The reference has
no search: this is judged on plumbing and on learning-curve sanity only (tools/search_demo.py --puct --train N).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch

from .distributed import allreduce_mean_, broadcast_module
from .search import MOVE_PROPORTIONAL, network_evaluator, puct_selfplay
from .visit_targets import cross_entropy, cross_entropy_torch


@dataclass
class AlphaZeroConfig:
    moves: int = 4            # moves of every root per collect()
    iterations: int = 16      # search iterations per move
    max_children: int = 16    # C: candidates per node, and entries of a policy target
    c_puct: float = 1.0
    capacity: Optional[int] = None  # node slots per root (puct_selfplay's default: 1 + 2 * iterations * leaves * max_children)
    leaves: int = 1           # L: leaves selected per root and iteration; the planner then has P * L environments
    mode: int = MOVE_PROPORTIONAL  # how the move is picked from the root's visits (MOVE_GREEDY: the most visited)
    epochs: int = 1
    minibatches: int = 1
    policy_coef: float = 1.0
    value_coef: float = 0.5
    entropy_coef: float = 0.0
    lr: float = 3e-4
    # update() evaluates the policy loss with visit_targets.cross_entropy on the raw logits (pcbenv_evaluate_visits and its
    # backward) instead of the torch chain cross_entropy_torch.  Both read the same stored mask_bits and targets.
    device_loss: bool = False
    # Exploration noise on the root's priors, once per root and move (puct_selfplay's root_noise): a draw from
    # Dir(noise_alpha) mixed in with weight noise_eps.  None: no noise.
    noise_alpha: Optional[float] = None
    noise_eps: float = 0.25
    # Gumbel root search (puct_selfplay's gumbel): every move is a search of `iterations` simulations spent by Sequential
    # Halving over gumbel_considered candidates, and the policy target is softmax(logit + sigma(completed q)) in the place of
    # the visit counts; sigma(q) = (gumbel_c_visit + the most visits of a root child) * gumbel_c_scale * q.  `mode` is then not
    # read.  None: PUCT at the root.  Not together with noise_alpha; with leaves = L > 1 a move is ceil(iterations / L) + 1 evaluations
    # of P * L rows (pcbenv_gumbel_advance_leaves).
    gumbel_considered: Optional[int] = None
    gumbel_c_visit: float = 50.0
    gumbel_c_scale: float = 1.0
    # the full Gumbel rule (puct_selfplay's gumbel_full, pcbenv_gumbel_tree_advance): below the root the search goes to the
    # argmax of pi' - n / (1 + sum n) and a child without a visit is completed with v_mix; needs gumbel_considered and leaves = 1
    gumbel_full: bool = False
    # "gumbel": the full Gumbel rule with any leaves (puct_selfplay's gumbel_node_rule): gumbel_full's launches with leaves = 1,
    # pcbenv_gumbel_tree_advance_leaves' with more, where a pending visit counts as a visit of the child; needs gumbel_considered
    gumbel_node_rule: str = "puct"


def value_targets(reward: torch.Tensor, done: torch.Tensor):
    """(z, weight), both like `reward` [M, P]: z[j, p] is the reward of the transition that ended the episode move j of
    root p belongs to -- carried backwards over the moves of that episode by a reverse scan over `done` -- and weight 1;
    moves whose episode did not end inside the batch have weight 0 (and z 0)."""
    z, weight = torch.zeros_like(reward), torch.zeros_like(reward)
    cur_z, cur_w = torch.zeros_like(reward[0]), torch.zeros_like(reward[0])
    for j in reversed(range(reward.shape[0])):
        over = done[j].bool()
        cur_z = torch.where(over, reward[j], cur_z)
        cur_w = torch.where(over, torch.ones_like(cur_w), cur_w)
        z[j], weight[j] = cur_z, cur_w
    return z, weight


def alphazero_loss(ce, entropy, value, z, weight, cfg: AlphaZeroConfig):
    """policy_coef mean(ce) + value_coef weighted mse(value, z) - entropy_coef mean(entropy) -> (loss, the three terms)."""
    policy = ce.mean()
    vf = (weight * (value - z).pow(2)).sum() / weight.sum().clamp(min=1.0)
    ent = entropy.mean()
    return cfg.policy_coef * policy + cfg.value_coef * vf - cfg.entropy_coef * ent, policy, vf, ent


class AlphaZeroTrainer:
    """root: the self-play environments (auto_reset=True: an episode that ends is followed by the next).  planner: as many
    environments (cfg.leaves times as many with leaf-parallel search) of the root's definition with auto_reset=False, the root's run_seed and first_env_index 0
    (`network_evaluator`).  policy: `(obs, mask=False) -> (raw logits [B, A], value [B])`, e.g. pcbenv/policy.py's."""

    def __init__(self, root, planner, policy, cfg: AlphaZeroConfig = AlphaZeroConfig(),
                 obs_keys=("grid", "pin_grid", "component_grid", "placement_mask", "action_mask")):
        assert root.auto_reset, "create the root environments with auto_reset=True"
        self.root, self.planner, self.policy, self.cfg, self.obs_keys = root, planner, policy, cfg, obs_keys
        broadcast_module(policy)
        self.opt = torch.optim.Adam(policy.parameters(), lr=cfg.lr)
        self.step_index = 0  # of the next collect(): every search and every proportional draw has a key of its own
        cache = {}

        def logits_fn(obs):  # one forward per evaluated node: the value rides along
            with torch.no_grad():
                logits, cache["value"] = self.policy(obs, mask=False)
            return logits.contiguous()
        self.evaluate = network_evaluator(root, planner, logits_fn, lambda obs: cache["value"], max_children=cfg.max_children, priors="device",
                                          leaves=cfg.leaves)

    @torch.no_grad()
    def collect(self) -> Dict[str, torch.Tensor]:
        """`cfg.moves` searched moves of every root -> the batch, every field [M, P, ...]: obs and mask_bits of each move's
        root, child_visits / child_actions (the policy target), z / weight (the value target), reward and done.  No host
        synchronisation."""
        root, M, P = self.root, self.cfg.moves, self.root.num_envs
        dev = root.device
        obs = {k: torch.empty((M,) + tuple(root.obs[k].shape), dtype=root.obs[k].dtype, device=dev) for k in self.obs_keys}
        bits = torch.empty((M, P, 2, root.cfg.height, (root.cfg.width + 63) // 64), dtype=torch.int64, device=dev)

        def keep_root(j):  # the search never changes the root: the state after move j - 1 is move j's root
            for k in self.obs_keys:
                obs[k][j].copy_(root.obs[k])
            root.mask_bits(out=bits[j])
        keep_root(0)
        self.policy.eval()
        sp = puct_selfplay(root, self.evaluate, M, self.cfg.iterations, step_index=self.step_index, c_puct=self.cfg.c_puct,
                           max_children=self.cfg.max_children, capacity=self.cfg.capacity, mode=self.cfg.mode,
                           on_move=lambda j, tree: keep_root(j + 1) if j + 1 < M else None, leaves=self.cfg.leaves,
                           root_noise=None if self.cfg.noise_alpha is None else (self.cfg.noise_alpha, self.cfg.noise_eps),
                           gumbel=None if self.cfg.gumbel_considered is None else (self.cfg.gumbel_considered, self.cfg.gumbel_c_visit, self.cfg.gumbel_c_scale),
                           gumbel_full=self.cfg.gumbel_full, gumbel_node_rule=self.cfg.gumbel_node_rule)
        from .batched_env import default_max_steps
        evaluations = self.cfg.iterations + (self.cfg.gumbel_considered is not None)
        if self.cfg.gumbel_considered is not None and self.cfg.leaves != 1:
            evaluations = -(-self.cfg.iterations // self.cfg.leaves) + 1
        self.step_index += M * evaluations * default_max_steps(root.cfg)
        z, weight = value_targets(sp.reward.float(), sp.done)
        return {"obs": obs, "mask_bits": bits, "child_visits": sp.child_visits, "child_actions": sp.child_actions, "z": z, "weight": weight,
                "reward": sp.reward, "done": sp.done, "errors": sp.errors}

    def update(self, batch) -> Dict[str, float]:
        cfg = self.cfg
        M, P = batch["z"].shape
        N = M * P
        flat = lambda t: t.reshape((N,) + tuple(t.shape[2:]))
        flat_obs = {k: flat(v) for k, v in batch["obs"].items()}
        bits, visits, actions = flat(batch["mask_bits"]), flat(batch["child_visits"]), flat(batch["child_actions"])
        z, weight = flat(batch["z"]), flat(batch["weight"])
        # BatchNorm as in PPOTrainer.update: the statistics are refreshed once from a random minibatch in training mode,
        # the loss is evaluated with the running statistics the search used
        with torch.no_grad():
            self.policy.train()
            ridx = torch.randperm(N, device=z.device)[:max(1, N // cfg.minibatches)]
            self.policy({k: o[ridx] for k, o in flat_obs.items()}, mask=False)
            allreduce_mean_([b for b in self.policy.buffers() if b.is_floating_point()])
        self.policy.eval()
        stats = {}
        for _ in range(cfg.epochs):
            perm = torch.randperm(N, device=z.device)
            for idx in perm.chunk(cfg.minibatches):
                logits, value = self.policy({k: o[idx] for k, o in flat_obs.items()}, mask=False)
                if cfg.device_loss:
                    ce, entropy = cross_entropy(self.root, logits, bits[idx], visits[idx], actions[idx])
                else:
                    ce, entropy = cross_entropy_torch(self.root.cfg, logits, bits[idx], visits[idx], actions[idx])
                loss, policy, vf, ent = alphazero_loss(ce, entropy, value, z[idx], weight[idx], cfg)
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                allreduce_mean_([p.grad for p in self.policy.parameters() if p.grad is not None])
                torch.nn.utils.clip_grad_norm_(self.policy.parameters(), 1.0)
                self.opt.step()
                stats = {"loss": float(loss.detach()), "policy": float(policy.detach()), "value": float(vf.detach()), "entropy": float(ent.detach())}
        return stats
