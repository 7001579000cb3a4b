"""The AlphaZero policy loss: the cross entropy of the policy's masked categorical against the visit counts of a searched
move, and the entropy, differentiable with respect to the logits (`pcbenv_evaluate_visits` /
`pcbenv_evaluate_visits_backward`, include/pcbenv_train.h).

The targets are what `pcbenv_puct_move` CHOOSE writes per move and `puct_selfplay` stacks into `SelfPlay`: `child_visits`
[.., C] and `child_actions` [.., C, 3].  The legal set of a stored root is its bit-packed `mask_bits` row, as for
`masked_categorical.evaluate`.  The forward is one kernel launch that reads only legal logits and the <= 64 target
entries of a row, the backward one launch that writes the whole gradient.

`cross_entropy_torch` states the same thing with torch ops -- the bits unpacked, the reference's masked-logits chain,
`log_softmax`, the visits scattered into a dense target; it is the specification, and `cross_entropy` uses it for tensors
that are not on a HIP device.
"""
from __future__ import annotations

import torch

from .masked_categorical import unpack_mask_bits
from .rollout import masked_logits


class VisitCrossEntropy(torch.autograd.Function):
    """(cross_entropy, entropy) = f(logits); saves logits, mask_bits, the targets and the [N, 4] row statistics only."""

    @staticmethod
    def forward(ctx, env, logits, mask_bits, visits, target_actions):
        stats = torch.empty((logits.shape[0], 4), dtype=torch.float32, device=logits.device)
        ce, entropy = env.evaluate_visits_forward(logits, mask_bits, visits, target_actions, stats)
        ctx.env = env
        ctx.save_for_backward(logits, mask_bits, visits, target_actions, stats)
        return ce, entropy

    @staticmethod
    def backward(ctx, grad_ce, grad_entropy):
        logits, mask_bits, visits, target_actions, stats = ctx.saved_tensors
        gce = None if grad_ce is None else grad_ce.contiguous().float()
        gh = None if grad_entropy is None else grad_entropy.contiguous().float()
        grad = ctx.env.evaluate_visits_backward(logits, mask_bits, visits, target_actions, stats, gce, gh)
        return None, grad, None, None, None


def dense_targets(cfg, legal: torch.Tensor, visits: torch.Tensor, target_actions: torch.Tensor, dtype=torch.float32):
    """(pi [N, A], T int64 [N]): the visits of the valid entries -- visits > 0, the action in range and legal -- scattered
    into a dense target and divided by their total T (rows with T == 0 stay zero); entries with the same action add up."""
    O, H, W = cfg.num_orientations, cfg.height, cfg.width
    N, A = legal.shape
    a = target_actions.long()
    if a.dim() == 3:
        in_range = (a[..., 0] >= 0) & (a[..., 0] < O) & (a[..., 1] >= 0) & (a[..., 1] < H) & (a[..., 2] >= 0) & (a[..., 2] < W)
        a = a[..., 0] * (H * W) + a[..., 1] * W + a[..., 2]
    else:
        in_range = (a >= 0) & (a < A)
    a = torch.where(in_range, a, torch.zeros_like(a))
    valid = (visits > 0) & in_range & legal.gather(1, a)
    v = torch.where(valid, visits, torch.zeros_like(visits)).long()
    T = v.sum(dim=1)
    pi = torch.zeros((N, A), dtype=dtype, device=legal.device).scatter_add_(1, a, v.to(dtype) / T.clamp(min=1).to(dtype)[:, None])
    return pi, T


def cross_entropy_torch(cfg, logits: torch.Tensor, mask_bits: torch.Tensor, visits: torch.Tensor, target_actions: torch.Tensor):
    """The specification, with torch ops: `masked_logits` + `log_softmax` against the dense scattered target, and
    `Categorical.entropy`, computed in float32 (float64 logits stay float64).  Illegal logits are replaced by 0 before the
    mask is added, as in `evaluate_torch`.  Rows without a legal action or with T == 0 give cross entropy 0; rows without
    a legal action entropy 0.  Returns (cross_entropy [N], entropy [N])."""
    legal = unpack_mask_bits(cfg, mask_bits)
    l = logits if logits.dtype == torch.float64 else logits.float()
    masked = masked_logits(torch.where(legal, l, torch.zeros_like(l)), legal)
    logp = torch.log_softmax(masked, dim=1)
    pi, T = dense_targets(cfg, legal, visits, target_actions, l.dtype)
    ce = -torch.where(pi > 0, pi * logp, torch.zeros_like(logp)).sum(dim=1)
    entropy = torch.distributions.Categorical(logits=masked, validate_args=False).entropy()
    has = legal.any(dim=1)
    zero = torch.zeros((), dtype=l.dtype, device=l.device)
    return torch.where(has & (T > 0), ce, zero), torch.where(has, entropy, zero)


def cross_entropy(env, logits: torch.Tensor, mask_bits: torch.Tensor, visits: torch.Tensor, target_actions: torch.Tensor):
    """(cross_entropy, entropy) float32 [N] of the masked categorical of `logits` ([N, A] float32 / bfloat16) with the
    legal sets `mask_bits` (int64 [N, 2, H, WW]) against the visit distribution `visits` (int32 [N, C]) over
    `target_actions` (int32 [N, C, 3] or [N, C] flat); differentiable with respect to `logits`.  On a HIP device: the
    kernels.  Elsewhere: `cross_entropy_torch(env.cfg, ...)`."""
    if logits.device.type != "cuda":
        return cross_entropy_torch(env.cfg, logits, mask_bits, visits, target_actions)
    return VisitCrossEntropy.apply(env, logits.contiguous(), mask_bits, visits, target_actions)
