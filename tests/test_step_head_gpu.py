"""The head of a step launch in the geometry-fixed builds of k_step (part 4 of pcb_layout::step_build_part): what a launch
takes over from the one before it -- the action presampled into the state block's header -- against every call that
must make it stale, and both paths of the grid plane's emission (written out, and the loop PCBENV_FLAG_INCREMENTAL_OBS
keeps).

The fixed builds exist only on the 64 x 64 grid of a pin kind, so the grid is that one; the batch is small -- 8, 9 (not a
multiple of 8: the other arm of xcd_contiguous_env) and 64 -- and an episode has two or three components, so that a few
dozen launches hold a dozen episodes with their in-launch resets.  Every call goes through tests/handle_model.py's
Driver: after it every bound tensor, reward, done, info and mask_bits() are compared with the oracle bit for bit, and a
fused launch must have taken the action `sample_actions` draws from the mask alone -- a stale presampled action would
differ.

What makes a presampled action stale, each followed by a fused launch whose (seed, step index, environment) is the very
tag the stale action carries wherever the call leaves that possible, so that only the call's own invalidation protects it:
  other     pcbenv_step with an external action that differs from the presampled one (another legal cell), then the
            fused launch at the SAME step index (the repeated index: the tag matches, the mask does not);
  reset     pcbenv_reset of half of the environments, then the fused launch at the next index (the tag matches);
  gather    pcbenv_gather by a rotation (every row moves), then the fused launch at the next index;
  seed      another draw seed from here on (the tag's seed no longer matches);
  again     the fused launch repeated at the index of the last one (the tag's step index is the next one).
"""
import numpy as np
import pytest
import torch

from pcbenv import EnvConfig

from handle_model import Driver, Setup

pytestmark = pytest.mark.gpu

BATCHES = (8, 9, 64)
# two or three components of 2..4 x 2..4 cells, two nets of two or three pins: the smallest episodes the kinds allow
SMALL = dict(pin=lambda: EnvConfig.pin(64, 64, 9, 9, 2, 4, 2, 4, 3, 2, 2, 2, 3, 2, "centroid", 2, 0.5),
             spatial=lambda: EnvConfig.spatial(64, 64, 9, 9, 2, 4, 2, 4, 3, 2, 2, 2, 3, 2, "centroid", 2, 0.5))
CASES = {"pin": ("pin", {}), "spatial": ("spatial", {}), "pin_incremental": ("pin", {"incremental_obs": True}),
         "spatial_incremental": ("spatial", {"incremental_obs": True})}
ONE_WAVEFRONT = dict(threads_per_env=64)  # (with the in-place layout and the centroid reward: what pcb_layout::fixed_geometry_applies asks)
BLOCK = ("fused", "fused", "other", "fused", "reset", "fused", "fused", "gather", "fused", "seed", "fused", "again", "fused")
ROUNDS = 2


def other_legal_actions(drv, presampled):
    """Per row a legal action that is not `presampled[i]`: the last legal cell of the oracle's mask, or the first."""
    a = presampled.copy()
    differ = 0
    for i in range(drv.B):
        legal = np.argwhere(drv.model.ob.env(i).obs()["action_mask"] != 0)
        for cand in (legal[-1:], legal[:1]):
            if len(cand) and not np.array_equal(cand[0], presampled[i]):
                a[i] = cand[0]
                differ += 1
                break
    return a.astype(np.int32), differ


def run_case(kind, B, kw):
    setup = Setup(f"head_{kind}", SMALL[kind], B, (0,), 0, auto_reset=True, queue_depth=3, replay=False, **ONE_WAVEFRONT, **kw)
    drv = Driver(setup, run_seed=3, B=B)
    e = drv.env
    terminal = 0
    try:
        for rnd in range(ROUNDS):
            for k, op in enumerate(BLOCK):
                tag = (rnd, k, op)
                if op == "fused":
                    drv.op_fused(0, 0, tag)
                elif op == "other":
                    pre = e.sample_actions(drv.t).cpu().numpy()  # the action the last fused launch presampled for this index
                    a, differ = other_legal_actions(drv, pre)
                    assert differ >= B // 2, (tag, "too few rows with a second legal action", differ)
                    e.step(torch.from_numpy(a))
                    drv.stepped(a, tag)
                    drv.t -= 1  # the next fused launch carries the index the stale action was drawn for
                elif op == "reset":
                    drv.op_reset_mask(0.5, 17 + rnd, tag)
                elif op == "gather":
                    idx = (np.arange(B) + 1 + rnd) % B
                    e.gather_(torch.from_numpy(idx).to(e.device))
                    drv.model.gather(idx)
                    drv.compare(tag)
                elif op == "seed":
                    e.run_seed += 101  # the draws' seed (the instance streams were seeded at construction)
                elif op == "again":
                    drv.t -= 1
                if op in ("fused", "other"):
                    terminal += int(drv.model.last_done().any())
    finally:
        drv.close()
    assert terminal >= 2 * ROUNDS, terminal  # launches that ended episodes and reset them in the launch


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_presampled_action_against_every_call_that_stales_it(case, B):
    kind, kw = CASES[case]
    run_case(kind, B, kw)
