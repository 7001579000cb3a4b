"""The geometry-fixed build of the step kernel (PCBENV_OPT_FIXED_GEOMETRY, csrc/pcb_layout.h fixed_geometry_applies)
against the build that reads the grid at run time: the same seeded call sequence on two handles of c3 / c4 (64 x 64,
centroid reward), one with the option at 1 and one at 0; after every call every bound tensor, reward, done, info, the
actions taken and `mask_bits()` must be equal bit for bit.  The fused sequence also runs against the host model of
tests/handle_model.py.  B = 40 is no multiple of 8 (one arm of xcd_contiguous_env), B = 64 is (the other)."""
import numpy as np
import pytest
import torch

from pcbenv import named_config
from pcbenv.batched_env import BatchedPlacementEnv

from handle_model import Run

pytestmark = pytest.mark.gpu

STEPS = 40
CASES = [(name, B) for name in ("c3", "c4") for B in (40, 64)]


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


class Pair:
    """Two handles of one definition, seed and queue: `fix` runs the fixed build where it applies, `run` never does."""

    def __init__(self, cfg, B, fix=None, options=None, **kw):
        kw = dict(queue_depth=3, run_seed=3, mask_marginals=True, **kw)
        self.B = B
        self.fix = fix or BatchedPlacementEnv(cfg, B, options=dict(options or {}, fixed_geometry=1), **kw)
        self.run = BatchedPlacementEnv(cfg, B, options=dict(options or {}, fixed_geometry=0), **kw)
        for e in (self.run,) if fix else (self.fix, self.run):
            e.generate_instances()
            e.reset()
        self.compare("first reset")

    def both(self, f):
        return f(self.fix), f(self.run)

    def compare(self, tag):
        a, b = self.fix, self.run
        for k in a.traj:
            assert _same(a.traj[k], b.traj[k]), (tag, k)
        for k in a.traj_marginals:
            assert _same(a.traj_marginals[k], b.traj_marginals[k]), (tag, "marginal", k)
        assert _same(a.traj_reward, b.traj_reward), (tag, "reward")
        assert _same(a.traj_done, b.traj_done), (tag, "done")
        assert _same(a.traj_info, b.traj_info), (tag, "info")
        assert _same(a.mask_bits(), b.mask_bits()), (tag, "mask_bits")

    def fused(self, t):
        x, y = self.both(lambda e: e.rollout_step(t)[-1])
        assert _same(x, y), (("fused", t), "actions")
        self.compare(("fused", t))
        return int(self.fix.done.sum().item())

    def close(self):
        self.fix.close()
        self.run.close()


@pytest.mark.parametrize("name,B", CASES)
def test_fused_auto_reset_against_model_and_runtime_build(name, B):
    """40 fused steps with in-launch resets: the fixed build against the host model, the run-time build against the fixed one."""
    cfg = named_config(name)
    run = Run(cfg, B, auto_reset=True, mask_marginals=True, options={"fixed_geometry": 1})
    pair = Pair(cfg, B, fix=run.env, auto_reset=True)
    terminal_launches = 0
    taken, fused_launch = [], run.env.rollout_step
    run.env.rollout_step = lambda t: taken.append(fused_launch(t)) or taken[-1]  # (Run.step keeps the actions to itself)
    try:
        for t in range(STEPS):
            dd = run.step(t, fused=True)  # the model's comparison, after the fixed build's launch
            x = pair.run.rollout_step(t)[-1]
            assert _same(taken[-1][-1], x), (("fused", t), "actions")
            pair.compare(("fused", t))
            terminal_launches += bool(dd.any())
    finally:
        pair.run.close()
        run.close()
    assert terminal_launches >= 2, terminal_launches


@pytest.mark.parametrize("name,B", CASES)
def test_external_actions_with_reset_done(name, B):
    """40 explicit steps, tuple and flat actions in turn, a tenth of them out of range or illegal, reset_done() after each."""
    cfg = named_config(name)
    pair = Pair(cfg, B)
    rng = np.random.RandomState(7)
    HW, A = cfg.height * cfg.width, cfg.num_orientations * cfg.height * cfg.width
    try:
        for t in range(STEPS):
            a = pair.fix.sample_actions(t).cpu().numpy()
            assert np.array_equal(a, pair.run.sample_actions(t).cpu().numpy()), t
            bad = rng.rand(B) < 0.1
            if t % 2:
                f = (a[:, 0] * HW + a[:, 1] * cfg.width + a[:, 2]).astype(np.int64)
                f[bad] = rng.randint(-5, A + 5, size=int(bad.sum()))  # anywhere: mostly illegal cells, some out of range
                if bad.any():
                    f[np.flatnonzero(bad)[0]] = (-1, A, A + 4, 2 ** 31 - 1)[(t // 2) % 4]
                acts = torch.from_numpy(f.astype(np.int32))
            else:
                a[bad] = rng.randint(-1, 70, size=(int(bad.sum()), 3))
                acts = torch.from_numpy(a)
            pair.both(lambda e: e.step(acts))
            pair.compare(("step", t))
            pair.both(lambda e: e.reset_done())
            pair.compare(("reset_done", t))
    finally:
        pair.close()


@pytest.mark.parametrize("name,B", CASES)
def test_staggered_phases_with_helpers(name, B):
    """Episode phases spread over the batch: a sixteenth of it ends an episode in every launch, so the terminal list is
    kept and the launches start helpers -- the delegated environment team, the reward helpers and the feature helper."""
    cfg = named_config(name)
    L = cfg.max_num_components
    pair = Pair(cfg, B, auto_reset=True)
    terminal_launches = 0
    try:
        for t in range(STEPS):
            terminal_launches += pair.fused(t) > 0
            if t < L:
                m = torch.from_numpy((np.arange(B) % L == t).astype(np.uint8))
                pair.both(lambda e: e.reset(m))
                pair.compare(("spread", t))
    finally:
        pair.close()
    assert terminal_launches >= STEPS - L, terminal_launches


@pytest.mark.parametrize("name,B", CASES)
def test_fused_with_streaming_stores(name, B):
    """stream_threshold_bytes = 0: the streaming-store twins of both builds."""
    cfg = named_config(name)
    pair = Pair(cfg, B, auto_reset=True, options={"stream_threshold_bytes": 0})
    terminal_launches = 0
    try:
        for t in range(STEPS):
            terminal_launches += pair.fused(t) > 0
    finally:
        pair.close()
    assert terminal_launches >= 2, terminal_launches


def test_option_values():
    """0 and 1 are the option's values; the escape hatch can be flipped between launches."""
    from pcbenv import _lib
    cfg = named_config("c3")
    pair = Pair(cfg, 8, auto_reset=True)
    try:
        assert pair.fix._L.pcbenv_set_option(pair.fix._h, _lib.OPT_FIXED_GEOMETRY, 2) == _lib.PCBENV_EINVAL
        assert pair.fix._L.pcbenv_set_option(pair.fix._h, _lib.OPT_FIXED_GEOMETRY, -1) == _lib.PCBENV_EINVAL
        for t in range(6):
            pair.fix.set_option("fixed_geometry", t % 2)
            pair.fused(t)
    finally:
        pair.close()
