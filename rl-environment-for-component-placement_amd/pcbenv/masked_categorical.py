"""The update half of the policy's masked categorical: log-probability and entropy of stored actions, differentiable
with respect to the logits (`pcbenv_evaluate_logits` / `pcbenv_evaluate_logits_backward`).

The reference's models mask their logits (`logits += max(log(action_mask), float32.min)`,
`agent/models/square_model.py:137-139`) and RLlib's `Categorical.logp` / `entropy`
(`utils/agent/factorized_action_distributions.py:21-91`) are evaluated on them in every PPO minibatch.  Here the legal
set of a stored step is its bit-packed `mask_bits` row (2 KB at 64x64 against 16 KB of uint8 `action_mask`), the forward
is one kernel launch that reads only legal logits, and the backward one launch that writes the whole gradient.

`evaluate_torch` states the same thing with torch ops (the bits unpacked, the reference's masked-logits chain); `evaluate`
uses it for tensors that are not on a HIP device, so that CPU tests and A/B measurements share one definition.
"""
from __future__ import annotations

import torch

from .rollout import masked_logits


class MaskedCategoricalEval(torch.autograd.Function):
    """(log_prob, entropy) = f(logits); saves logits, mask_bits, actions and the [N, 4] row statistics only."""

    @staticmethod
    def forward(ctx, env, logits, mask_bits, actions):
        stats = torch.empty((logits.shape[0], 4), dtype=torch.float32, device=logits.device)
        log_prob, entropy = env.evaluate_logits_forward(logits, mask_bits, actions, stats)
        ctx.env = env
        ctx.save_for_backward(logits, mask_bits, actions, stats)
        return log_prob, entropy

    @staticmethod
    def backward(ctx, grad_log_prob, grad_entropy):
        logits, mask_bits, actions, stats = ctx.saved_tensors
        glp = None if grad_log_prob is None else grad_log_prob.contiguous().float()
        gh = None if grad_entropy is None else grad_entropy.contiguous().float()
        grad = ctx.env.evaluate_logits_backward(logits, mask_bits, actions, stats, glp, gh)
        return None, grad, None, None


def unpack_mask_bits(cfg, mask_bits: torch.Tensor) -> torch.Tensor:
    """int64 [N, 2, H, WW] -> bool [N, O*H*W] in flat action order (orientation o reads plane o & 1; square: plane 0)."""
    N, H, W, O = mask_bits.shape[0], cfg.height, cfg.width, cfg.num_orientations
    cols = torch.arange(W, device=mask_bits.device)
    words = mask_bits[:, :, :, cols // 64]                  # [N, 2, H, W]
    planes = ((words >> (cols % 64)) & 1).bool()            # arithmetic shift: the sign fill is masked off
    return torch.stack([planes[:, o & 1] for o in range(O)], dim=1).reshape(N, O * H * W)


def _flat_actions(cfg, actions: torch.Tensor) -> torch.Tensor:
    a = actions.long()
    if a.dim() == 2:
        a = a[:, 0] * (cfg.height * cfg.width) + a[:, 1] * cfg.width + a[:, 2]
    return a


def evaluate_torch(cfg, logits: torch.Tensor, mask_bits: torch.Tensor, actions: torch.Tensor):
    """The reference's chain with torch ops: `masked_logits` + `Categorical.log_prob` / `entropy`, computed in float32
    (float64 logits stay float64).  Illegal logits are replaced by 0 before the mask is added, so that whatever they
    hold (NaN included) changes nothing, as for the kernels.  Rows without a legal action give 0 / 0, as the ABI states."""
    legal = unpack_mask_bits(cfg, mask_bits)
    l = logits if logits.dtype == torch.float64 else logits.float()
    masked = masked_logits(torch.where(legal, l, torch.zeros_like(l)), legal)
    d = torch.distributions.Categorical(logits=masked, validate_args=False)
    a = _flat_actions(cfg, actions)
    has = legal.any(dim=1)
    zero = torch.zeros((), dtype=l.dtype, device=l.device)
    return torch.where(has, d.log_prob(a), zero), torch.where(has, d.entropy(), zero)


def evaluate(env, logits: torch.Tensor, mask_bits: torch.Tensor, actions: torch.Tensor):
    """(log_prob, entropy) float32 [N] of the stored `actions` (int32 [N] flat or [N, 3]) under the masked categorical of
    `logits` ([N, A] float32 / bfloat16) with the legal sets `mask_bits` (int64 [N, 2, H, WW]); differentiable with
    respect to `logits`.  On a HIP device: the kernels.  Elsewhere: `evaluate_torch(env.cfg, ...)`."""
    if logits.device.type != "cuda":
        return evaluate_torch(env.cfg, logits, mask_bits, actions)
    return MaskedCategoricalEval.apply(env, logits.contiguous(), mask_bits, actions)
