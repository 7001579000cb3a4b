"""The persistent rollout (pcbenv_rollout_sampled: k_step's STEP_BUILD_ROLLOUT) at the shapes, team sizes and queue
bounds of tests/rollout_cases.py, against the plan of each case and the host model of tests/handle_model.py.

After every call of a case's script every tensor of every slot, reward, done, info, `_last_done`, the marginals and
`mask_bits()` are compared with the oracle (Driver.compare), and the actions the device recorded with the plan's, byte
for byte; after a rollout launch every step whose slot survived the launch is checked on its own.  Further: a rollout
against its single steps on a twin handle, the ABI's own arguments (flat format, another seed, first_env_index,
a step index that crosses 2^32) and the calls it refuses."""
import numpy as np
import pytest
import torch

import rollout_cases as rc
from handle_model import Driver, _bytes_equal, _same_info
from pcbenv import _lib
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.config import KIND_SQUARE

pytestmark = pytest.mark.gpu


def _driver(case):
    return Driver(case.setup(), run_seed=case.seed)


def _advance(drv):
    """Trajectory layout: the next transition goes to the slot behind the one the last transition wrote."""
    if drv.model.S > 1:
        s = drv.model.slot + 1
        drv.env.select_slot(s)
        drv.model.select(s)


def _explicit_step(drv, want, tag):
    a = drv.env.sample_actions(drv.t).cpu().numpy()
    assert _bytes_equal(a, want), (tag, "sample_actions draws other actions than the plan")
    drv.env.step(torch.from_numpy(a))
    drv.stepped(a, tag)


def _run_call(drv, c, tag):
    """One call of a plan on the device, compared with the model after it (Driver) and with the plan."""
    if c["op"] == "reset_mask":
        drv.op_reset_mask(c["arg"], c["seed"], tag)
        return
    _advance(drv)
    assert (drv.t, drv.model.slot) == (c["t0"], c["slot0"]), (tag, "the driver is not where the plan is")
    if c["op"] == "rollout":
        got = drv.op_rollout(c["arg"], c["seed"], tag, expect=lambda k: c["actions"][k])
        assert _bytes_equal(got, c["actions"]), (tag, "recorded actions")
    elif c["op"] == "fused":
        drv.op_fused(0, c["seed"], tag)
        assert _bytes_equal(drv.last_actions, c["actions"][0]), (tag, "recorded actions")
    else:
        _explicit_step(drv, c["actions"][0], tag)
    rr, dd, _ = c["steps"][-1]  # (the model took the plan's actions: its last transition is the plan's)
    assert _bytes_equal(drv.model.R[drv.model.slot], rr) and np.array_equal(drv.model.D[drv.model.slot], dd), (tag, "plan")


@pytest.mark.parametrize("name", list(rc.CASES))
def test_case(name):
    case, plan = rc.CASES[name], rc.plan(name)
    print(f"ROLLOUT-MIX {name} seed {case.seed}: {plan.mix()}")
    drv = _driver(case)
    try:
        for j, c in enumerate(plan.calls):
            _run_call(drv, c, (name, j, c["op"], c["arg"]))
        if case.device_instances:
            assert drv.env.device_instance_errors() == 0
    finally:
        drv.close()


# ---- a rollout equals its single steps --------------------------------------------------------------------------
def _bare(case):
    cfg = case.cfg()
    kw = dict(case.kw, num_slots=case.S) if case.S > 1 else dict(case.kw)
    env = BatchedPlacementEnv(cfg, case.B, queue_depth=case.Q, run_seed=case.seed, auto_reset=True, **kw)
    if case.device_instances:
        env.enable_device_instances()
    elif cfg.kind != KIND_SQUARE:
        env.generate_instances()
    env.reset()
    return env


def _assert_twins_equal(a, b, tag):
    for k in a.traj:
        assert torch.equal(a.traj[k], b.traj[k]), (tag, k)
    for k in a.traj_marginals:
        assert torch.equal(a.traj_marginals[k], b.traj_marginals[k]), (tag, "marginal", k)
    assert torch.equal(a.traj_reward.view(torch.int64), b.traj_reward.view(torch.int64)), (tag, "reward")
    assert torch.equal(a.traj_done, b.traj_done), (tag, "done")
    assert _same_info(a.traj_info.cpu().numpy(), b.traj_info.cpu().numpy()), (tag, "info")
    assert torch.equal(a.mask_bits(), b.mask_bits()), (tag, "mask_bits")


@pytest.mark.parametrize("name", ["spatial_7x100_t256", "pin_40x48_k4_t256", "crowded_pin_inplace"])
def test_rollout_equals_its_single_steps(name):
    """include/pcbenv.h: "num_steps consecutive pcbenv_step_sampled transitions".  Handle `a` runs the script of the
    case, its twin `b` takes rollout_step n times where `a` takes rollout_steps(n); every other call is the same."""
    case, plan = rc.CASES[name], rc.plan(name)
    a, b = _bare(case), _bare(case)
    S, B = case.S, case.B
    try:
        slot = 0
        for j, c in enumerate(plan.calls):
            tag = (name, j, c["op"], c["arg"])
            if c["op"] == "reset_mask":
                for e in (a, b):
                    e.reset(torch.from_numpy(c["mask"]))
            else:
                slot, t0, n = c["slot0"], c["t0"], len(c["steps"])
                a.select_slot(slot)
                b.select_slot(slot)
                if c["op"] == "rollout":
                    acts_a = a.rollout_steps(t0, n)
                    acts_b = torch.full_like(acts_a, -7)
                    for k in range(n):
                        b.select_slot(slot + k)
                        b.rollout_step(t0 + k, out=acts_b[k])
                    slot = (slot + n - 1) % S
                    a.select_slot(slot)
                elif c["op"] == "fused":
                    acts_a, acts_b = (e.rollout_step(t0)[-1][None] for e in (a, b))
                else:
                    acts_a = acts_b = a.sample_actions(t0)[None]
                    a.step(acts_a[0])
                    b.step(acts_a[0])
                assert torch.equal(acts_a, acts_b), (tag, "actions")
                assert _bytes_equal(acts_a.cpu().numpy(), c["actions"]), (tag, "actions against the plan")
            _assert_twins_equal(a, b, tag)
    finally:
        a.close()
        b.close()


# ---- the ABI's own arguments -----------------------------------------------------------------------------------
OTHER_SEED = 0x5EED0123456789AB


@pytest.mark.parametrize("name", ["pin_100x9", "rect_33x65"])
def test_abi_arguments(name):
    """pcbenv_rollout_sampled itself: the flat format, a seed other than the run seed, first_env_index = 1000 (the
    instances stay the handle's, only the draws move) and step_index0 = 2^32 - 2 with five steps.  A fused step comes
    first: what it has presampled (run seed, step 1, environment i) is not what this launch asks for at t = 0."""
    case = rc.CASES[name]
    cfg, B = case.cfg(), case.B
    drv = _driver(case)
    try:
        _advance(drv)
        drv.op_fused(0, 0, (name, "fused"))
        _advance(drv)
        t0, n, drawn = 2 ** 32 - 2, 5, []

        def expect(k):
            drawn.append(rc.draws(cfg, drv.model, OTHER_SEED, 1000, t0 + k))
            return drawn[-1]
        rec = drv.op_rollout(n, 0, (name, "abi"), flat=True, draw_seed=OTHER_SEED, first_env_index=1000, t0=t0, expect=expect)
        d = np.stack(drawn).astype(np.int64)
        want = (d[..., 0] * cfg.height * cfg.width + d[..., 1] * cfg.width + d[..., 2]).astype(np.int32)
        assert rec.shape == (n, B) and _bytes_equal(rec, want)
        assert drv.t == t0 + n
        # the handle goes on from there with its own numbers
        _advance(drv)
        drv.op_rollout(2, 0, (name, "after"), expect=lambda k: rc.draws(cfg, drv.model, case.seed, 0, t0 + n + k))
        # Only first_env_index moves, directly behind a fused call at the step before: the presampled action carries the
        # run seed and this launch's step index, but environment i's number, not 1000 + i's -- it must not be taken.
        _advance(drv)
        drv.op_fused(0, 0, (name, "fused again"))
        _advance(drv)
        t1 = drv.t
        assert t1 == t0 + n + 3
        drv.op_rollout(2, 0, (name, "first_env_index alone"), first_env_index=1000,
                       expect=lambda k: rc.draws(cfg, drv.model, case.seed, 1000, t1 + k))
    finally:
        drv.close()


# ---- the calls it refuses --------------------------------------------------------------------------------------
def _snapshot(env):
    snap = {"traj/" + k: v for k, v in env.traj.items()}
    snap.update({"marginal/" + k: v for k, v in env.traj_marginals.items()})
    snap.update(reward=env.traj_reward, done=env.traj_done, info=env.traj_info, last_done=env._last_done, mask_bits=env.mask_bits())
    snap = {k: v.cpu().numpy().copy() for k, v in snap.items()}
    snap["cursors"] = np.array(env.queue_cursors(), np.int64)
    return snap


@pytest.mark.parametrize("name", ["pin_100x9", "rect_4x4_generator"])
def test_refused_calls_change_nothing(name):
    """num_steps = -1 and a null actions_out: PCBENV_EINVAL; num_steps = 0: PCBENV_OK; on the generator handle (queue_depth
    4) num_steps = 5: PCBENV_ELIMIT.  Each leaves every tensor, the queue cursors and mask_bits() as they were, and the
    rollout_steps(4) behind them is the plan's."""
    case = rc.CASES[name]
    plan = rc.Plan(case, script=(("fused",), ("rollout", 4)))
    drv = _driver(case)
    env, L = drv.env, drv.env._L
    try:
        _run_call(drv, plan.calls[0], (name, "fused"))
        before = _snapshot(env)
        out = torch.full((5, case.B, 3), -7, dtype=torch.int32, device=env.device)
        calls = [("num_steps = -1", out.data_ptr(), -1, _lib.PCBENV_EINVAL), ("null actions_out", None, 2, _lib.PCBENV_EINVAL),
                 ("num_steps = 0", out.data_ptr(), 0, _lib.PCBENV_OK)]
        if case.device_instances:
            assert case.Q == 4
            calls.append(("num_steps = 5 > queue_depth", out.data_ptr(), 5, _lib.PCBENV_ELIMIT))
        for what, ptr, n, want in calls:
            got = L.pcbenv_rollout_sampled(env._h, ptr, _lib.ACTION_TUPLE, n, env.run_seed, env.first_env_index, drv.t, env._stream())
            assert got == want, (what, got)
            after = _snapshot(env)
            for k, v in before.items():
                assert _bytes_equal(after[k], v), (what, "changed", k)
            assert bool((out == -7).all()), (what, "actions were written")
        _run_call(drv, plan.calls[1], (name, "rollout 4"))
        if case.device_instances:
            assert env.device_instance_errors() == 0
    finally:
        drv.close()
