"""Factorised policies: the action (orientation, x, y) drawn one coordinate at a time, each from a masked categorical over
O, H or W logits instead of one over O*H*W (`utils/agent/factorized_action_distributions.py:107-818`, used by
`agent/models/rectangle_model_factorized.py`, `rectangle_pin_factorized_model.py` and
`rectangle_pin_all_attn_factorized.py`).

The reference ships two orders, stated here as data: "orientation" = p(o) p(x|o) p(y|o,x) and "coordinates" =
p(x) p(y|x) p(o|x,y).  A stage is `(axis, given)` with axis 0 = orientation, 1 = x, 2 = y and `given` the axes already
drawn.  Its mask is a reduce_max / gather of `action_mask` in the reference; here the device derives it from the
bit-packed legal set (`pcbenv_sample_axis` for the draw, `pcbenv_evaluate_axis` / `_backward` for the update), so a
stored step keeps `mask_bits` (1 KB at 64x64) and nothing reads `action_mask`.

`evaluate_axis_torch` states the same thing with torch ops on the unpacked mask (the reference's chain); `evaluate_axis`
uses it for tensors that are not on a HIP device, so that CPU tests and A/B measurements share one definition.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch
import torch.nn as nn

from .masked_categorical import unpack_mask_bits
from .rollout import masked_logits

AXIS_ORIENTATION, AXIS_X, AXIS_Y = 0, 1, 2
# order name -> its three stages (axis, given axes)
ORDERS = {
    "orientation": ((AXIS_ORIENTATION, ()), (AXIS_X, (AXIS_ORIENTATION,)), (AXIS_Y, (AXIS_ORIENTATION, AXIS_X))),
    "coordinates": ((AXIS_X, ()), (AXIS_Y, (AXIS_X,)), (AXIS_ORIENTATION, (AXIS_X, AXIS_Y))),
}


def axis_sizes(cfg) -> Tuple[int, int, int]:
    return cfg.num_orientations, cfg.height, cfg.width


class FactorisedHeads(nn.Module):
    """The reference's three action models, one `Dense` each (`rectangle_pin_factorized_model.py:166-303`): the head of a
    stage reads the encoding concatenated, in the order the coordinates were drawn, with the one-hot orientation as
    float32 (O inputs), x / H and y / W as float32 (one input each; `factorized_action_distributions.py:438, :751,
    :794-795`), and emits O, H or W logits."""

    def __init__(self, enc_dim: int, cfg, order: str = "orientation"):
        super().__init__()
        if order not in ORDERS:
            raise ValueError(f"order must be one of {sorted(ORDERS)}, got {order!r}")
        self.cfg, self.order, self.stages, self.enc_dim = cfg, order, ORDERS[order], int(enc_dim)
        sizes = axis_sizes(cfg)
        width = {AXIS_ORIENTATION: sizes[AXIS_ORIENTATION], AXIS_X: 1, AXIS_Y: 1}  # inputs a drawn coordinate adds
        self.heads = nn.ModuleList(nn.Linear(self.enc_dim + sum(width[a] for a in given), sizes[axis])
                                   for axis, given in self.stages)

    def head_input(self, stage: int, enc: torch.Tensor, actions: torch.Tensor) -> torch.Tensor:
        O, H, W = axis_sizes(self.cfg)
        parts = [enc]
        for a in self.stages[stage][1]:
            col = actions[:, a].long()
            if a == AXIS_ORIENTATION:
                parts.append(torch.nn.functional.one_hot(col.clamp(0, O - 1), O).to(enc.dtype))
            else:
                parts.append((col.to(torch.float32) / (H if a == AXIS_X else W)).to(enc.dtype).unsqueeze(1))
        return torch.cat(parts, dim=1)

    def logits(self, stage: int, enc: torch.Tensor, actions: torch.Tensor) -> torch.Tensor:
        """Raw logits [N, n] of stage `stage`, its head fed the columns of `actions` (int [N, 3]) its stage is given."""
        return self.heads[stage](self.head_input(stage, enc, actions))


def axis_legal_torch(cfg, axis: int, given: Sequence[int], mask_bits: torch.Tensor, actions: torch.Tensor) -> torch.Tensor:
    """The stage's mask as the reference computes it on the unpacked `action_mask` [N, O, H, W]: a gather along every given
    axis, a reduce_max over the remaining ones (`:358, :398-401, :445-448, :717, :757-758, :803-808`) -> bool [N, n].  A
    given value outside its axis leaves the row empty."""
    sizes = axis_sizes(cfg)
    N = mask_bits.shape[0]
    m = unpack_mask_bits(cfg, mask_bits).reshape(N, *sizes)
    ok = torch.ones(N, dtype=torch.bool, device=m.device)
    for a in (AXIS_ORIENTATION, AXIS_X, AXIS_Y):
        if a == axis:
            continue
        if a in given:
            v = actions[:, a].long()
            ok &= (v >= 0) & (v < sizes[a])
            shape = list(m.shape)
            shape[a + 1] = 1
            m = m.gather(a + 1, v.clamp(0, sizes[a] - 1).reshape(N, 1, 1, 1).expand(shape))
        else:
            m = m.any(dim=a + 1, keepdim=True)  # reduce_max of a 0 / 1 mask
    return m.reshape(N, sizes[axis]) & ok[:, None]


def evaluate_axis_torch(cfg, axis: int, given: Sequence[int], logits: torch.Tensor, mask_bits: torch.Tensor, actions: torch.Tensor):
    """The reference's chain with torch ops: the stage's mask, `masked_logits`, `Categorical.log_prob` / `entropy`, in
    float32 (float64 logits stay float64).  Logits outside the mask are replaced by 0 before the mask is added, so that
    whatever they hold changes nothing, as for the kernels.  Rows with an empty mask give 0 / 0, and a stored value that is
    not in the mask log_prob 0 and a gradient without the one-hot term, as the ABI states."""
    legal = axis_legal_torch(cfg, axis, tuple(given), mask_bits, actions)
    l = logits if logits.dtype == torch.float64 else logits.float()
    masked = masked_logits(torch.where(legal, l, torch.zeros_like(l)), legal)
    d = torch.distributions.Categorical(logits=masked, validate_args=False)
    a = actions[:, axis].long()
    n = legal.shape[1]
    a_in = (a >= 0) & (a < n) & legal.gather(1, a.clamp(0, n - 1)[:, None])[:, 0]
    has = legal.any(dim=1)
    zero = torch.zeros((), dtype=l.dtype, device=l.device)
    lse = torch.logsumexp(masked, dim=1)
    dropped = lse.detach() - lse  # the value 0 with the gradient -p_v: log_prob without its one-hot term
    return torch.where(has, torch.where(a_in, d.log_prob(a.clamp(0, n - 1)), dropped), zero), torch.where(has, d.entropy(), zero)


class MaskedAxisEval(torch.autograd.Function):
    """(log_prob, entropy) = f(logits) of one stage; saves logits, mask_bits and actions only (the backward kernel
    recomputes the row statistics)."""

    @staticmethod
    def forward(ctx, env, axis, given, logits, mask_bits, actions):
        log_prob, entropy = env.evaluate_axis_forward(axis, given, logits, mask_bits, actions)
        ctx.env, ctx.axis, ctx.given = env, axis, given
        ctx.save_for_backward(logits, mask_bits, actions)
        return log_prob, entropy

    @staticmethod
    def backward(ctx, grad_log_prob, grad_entropy):
        logits, mask_bits, actions = ctx.saved_tensors
        glp = None if grad_log_prob is None else grad_log_prob.contiguous().float()
        gh = None if grad_entropy is None else grad_entropy.contiguous().float()
        grad = ctx.env.evaluate_axis_backward(ctx.axis, ctx.given, logits, mask_bits, actions, glp, gh)
        return None, None, None, grad, None, None


def evaluate_axis(env, axis: int, given: Sequence[int], logits: torch.Tensor, mask_bits: torch.Tensor, actions: torch.Tensor):
    """(log_prob, entropy) float32 [N] of the values stored in column `axis` of `actions` (int32 [N, 3]) under the stage's
    masked categorical of `logits` ([N, n] float32 / bfloat16), the legal sets derived from `mask_bits` (int64
    [N, 2, H, WW]) and the given columns of `actions`; differentiable with respect to `logits`.  On a HIP device: the
    kernels.  Elsewhere: `evaluate_axis_torch(env.cfg, ...)`."""
    if logits.device.type != "cuda":
        return evaluate_axis_torch(env.cfg, axis, given, logits, mask_bits, actions)
    return MaskedAxisEval.apply(env, axis, tuple(given), logits.contiguous(), mask_bits, actions)


class FactorisedPolicy(nn.Module):
    """An encoder with `.encode(obs)` (the encoding, or a tuple whose first element it is) and `.enc_dim` -- `SpatialPolicy`
    has both -- the three heads of an order and a `Dense(1)` value."""

    def __init__(self, encoder: nn.Module, cfg, order: str = "orientation"):
        super().__init__()
        self.cfg, self.encoder = cfg, encoder
        self.heads = FactorisedHeads(encoder.enc_dim, cfg, order)
        self.value = nn.Linear(encoder.enc_dim, 1)

    def encoding(self, obs) -> torch.Tensor:
        enc = self.encoder.encode(obs)
        return enc[0] if isinstance(enc, tuple) else enc

    @torch.no_grad()
    def act(self, env, obs, step_index: int, greedy: bool = False, out: torch.Tensor = None):
        """Three `env.sample_axis` launches, each head fed the values just drawn -> (actions int32 [B, 3], log_prob,
        entropy), the latter two summed over the stages as the reference's `logp` / `entropy` do."""
        enc = self.encoding(obs)
        actions = torch.zeros((env.num_envs, 3), dtype=torch.int32, device=env.device) if out is None else out
        log_prob = entropy = None
        for i, (axis, given) in enumerate(self.heads.stages):
            logits = self.heads.logits(i, enc, actions)
            if logits.dtype != torch.bfloat16:
                logits = logits.float()
            lp, ent = env.sample_axis(axis, logits.contiguous(), step_index, actions, given, greedy=greedy)
            log_prob, entropy = (lp, ent) if log_prob is None else (log_prob + lp, entropy + ent)
        return actions, log_prob, entropy

    def evaluate(self, env, obs, mask_bits: torch.Tensor, actions: torch.Tensor):
        """(log_prob, entropy, value) [N] of stored steps: three `evaluate_axis` calls on the stored `mask_bits` and
        `actions`, summed; differentiable with respect to the heads and the encoder."""
        enc = self.encoding(obs)
        log_prob = entropy = None
        for i, (axis, given) in enumerate(self.heads.stages):
            logits = self.heads.logits(i, enc, actions)
            if logits.dtype != torch.bfloat16:
                logits = logits.float()
            lp, ent = evaluate_axis(env, axis, given, logits, mask_bits, actions)
            log_prob, entropy = (lp, ent) if log_prob is None else (log_prob + lp, entropy + ent)
        return log_prob, entropy, self.value(enc).squeeze(-1)
