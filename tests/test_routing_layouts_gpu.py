"""The routing reward on the device at the pin layouts of tests/routing_layouts.py: every environment of a handle gets one
layout (hand-built records through load_instances), the episode is the layout's placement list, and reward, done and info
are compared bit for bit with OracleBatch at every step, every observation tensor at the terminal step and at the step
behind it.  The oracle itself is pinned to the reference at these layouts by tests/test_routing_layouts.py; the fixture's
terminal rows are asserted here as well, so a failure names the layout.

A handle plays three episodes (queue slot 0, slot 1 = the table rotated by one environment, slot 0 again), each with
another capacity of the terminal list: 0 (the terminal transition on the environment's own team), at least B (every
terminal has helper teams) and 16 (one entry per shard: one launch holds listed and unlisted terminals; all B episodes
end in the same launch because every layout is padded to 64 components).  Before the last placement of every episode a
playout from each root with that placement as first action must give the step's reward and info.  Every configuration
-- both pin kinds, `beam` and `both` at every beam width the kind accepts -- runs four handles: 64 and 256 threads, in
place and the slot build, auto_reset on and off; `centroid` runs two, and once more on the 64 x 64 grid, where the
fixed-geometry build scores the layouts."""
import time

import numpy as np
import pytest
import torch

import routing_layouts as rl
from handle_model import _bytes_equal
from oracle import oracle as orc
from pcbenv.batched_env import BatchedPlacementEnv

pytestmark = pytest.mark.gpu

# The handles of one (kind, reward type, beam width): (handle keywords, terminal-list capacities of the three episodes; "B" = 16 * B)
VARIANTS = (
    (dict(threads_per_env=64), (0, "B", 16)),
    (dict(threads_per_env=256, auto_reset=True), ("B", 16, 0)),
    (dict(threads_per_env=64, num_slots=3, auto_reset=True), (16, 0, "B")),
    (dict(threads_per_env=256, num_slots=2), (0, 16, "B")),
)
# name -> (kind, reward type, beam width, grid side, handles).  A handle takes under 0.1 s on an MI355X, so every routed
# configuration runs all four; `centroid` has no helpers to share a reward with and runs the first two, and once more on
# the 64 x 64 grid with one wavefront, in place: the fixed-geometry build.
CONFIGS = {f"{kind}_{rt}_k{k}": (kind, rt, k, 24, VARIANTS) for kind in rl.KINDS for rt in ("beam", "both") for k in rl.BEAM_WIDTHS[kind]}
CONFIGS.update({f"{kind}_centroid": (kind, "centroid", 2, 24, VARIANTS[:2]) for kind in rl.KINDS})
CONFIGS["pin_centroid_64x64_fixed"] = ("pin", "centroid", 2, 64, ((dict(threads_per_env=64, options={"fixed_geometry": 1}), (0, 0, 0)),))


def test_the_table_of_handles():
    """Every (kind, reward type, beam width) the device accepts has its handles; over them 64 and 256 threads, auto_reset on
    and off, the in-place and the slot build each meet every capacity of the terminal list."""
    assert len(CONFIGS) == 2 * (4 + 3) + 3
    seen = set()
    for kw, teams in VARIANTS:
        assert set(teams) == {0, "B", 16}
        seen |= {(kw["threads_per_env"], bool(kw.get("auto_reset")), kw.get("num_slots", 1) > 1)}
    assert {s[0] for s in seen} == {64, 256} and {s[1] for s in seen} == {False, True} and {s[2] for s in seen} == {False, True}
    assert {(t, sl) for t, _, sl in seen} == {(64, False), (256, False), (64, True), (256, True)}


def _compare_obs(env, ob, tag):
    for key, v in env.obs_f64().items():
        bad = ob.first_mismatch(key, v.cpu().numpy())
        assert bad < 0, (tag, key, "first environment", bad)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_handles(name):
    kind, rt, k, side, variants = CONFIGS[name]
    for kw, teams in variants:
        _run_handle(f"{name} {kw}", kind, rt, k, side, kw, teams)


def _run_handle(name, kind, rt, k, side, kw, teams):
    t_start = time.time()
    cfg = rl.config(kind, rt, k, side)
    _, rows = rl.fixture()
    slots = [rl.batch(kind, 0, side), rl.batch(kind, 1, side)]  # (names, packed, placements) of queue slot 0 and 1
    B, T = len(slots[0][0]), rl.T
    auto, S = bool(kw.get("auto_reset")), kw.get("num_slots", 1)
    assert B > 16, "a capacity of 16 must leave terminals unlisted"
    env = BatchedPlacementEnv(cfg, B, queue_depth=2, run_seed=5, **kw)
    ob = orc.OracleBatch(cfg, B)
    everyone = torch.arange(B, dtype=torch.int32, device=env.device)
    try:
        for q in (0, 1):
            env.load_packed(slots[q][1], slot=q)
        env.reset()
        ob.reset_packed(slots[0][1])
        _compare_obs(env, ob, (name, "first reset"))
        step = 0
        for episode, cap in enumerate(teams):
            names, _, acts = slots[episode % 2]
            env.set_option("terminal_teams", 16 * B if cap == "B" else cap)
            for t in range(T):
                tag = (name, "episode", episode, "teams", cap, "step", t)
                a = torch.from_numpy(acts[t]).to(env.device)
                po = env.playout(index=everyone, first_actions=a, step_index=step) if t == T - 1 else None
                if S > 1:
                    env.select_slot(step + 1)
                _, r, d, _ = env.step(a)
                step += 1
                rr, dd, ii = ob.step(acts[t])
                r, d, inf = r.cpu().numpy(), d.cpu().numpy(), env.info_raw.cpu().numpy()
                assert np.array_equal(d, dd) and bool(dd.all()) == (t == T - 1), (tag, "done")
                bad = np.flatnonzero(r.view(np.uint64) != rr.view(np.uint64))
                assert bad.size == 0, (tag, "reward", [names[i] for i in bad[:6]])
                has = ~np.isnan(inf[:, 0])
                assert _bytes_equal(inf[has], ii[has]) and bool(has.all()) == (t == T - 1), (tag, "info", [names[i] for i in np.flatnonzero(has)[:6]])
                if auto and episode > 0 and t == 0:  # with auto_reset the step behind a terminal one is the next episode's first
                    _compare_obs(env, ob, (tag, "behind the end"))
            # the terminal transition: the fixture's rows, the playout, every observation tensor
            for i, layout in enumerate(names):
                want = rows[(layout, kind, rt, k, side)]
                got = tuple(int(b) for b in np.array([r[i], inf[i, 0], inf[i, 1]]).view(np.uint64))
                assert got == want, (tag, "the reference's reward and info", layout)
            assert _bytes_equal(po.reward.cpu().numpy(), rr) and _bytes_equal(po.info.cpu().numpy(), ii), (tag, "playout")
            assert bool((po.done == 1).all()) and bool((po.length == 1).all()), (tag, "playout done / length")
            nxt = slots[(episode + 1) % 2][1]
            if auto:
                ob.reset_packed(nxt)  # the terminal launch has taken the next record
                _compare_obs(env, ob, tag)
            else:
                _compare_obs(env, ob, tag)
                # the step behind the terminal one (the reference keeps no done latch)
                if S > 1:
                    env.select_slot(step + 1)
                zero = np.zeros((B, 3), np.int32)
                _, r, d, _ = env.step(torch.from_numpy(zero).to(env.device))
                step += 1
                rr, dd, ii = ob.step(zero)
                inf = env.info_raw.cpu().numpy()
                has = ~np.isnan(inf[:, 0])
                assert np.array_equal(d.cpu().numpy(), dd) and _bytes_equal(r.cpu().numpy(), rr) and _bytes_equal(inf[has], ii[has]), (tag, "behind the end")
                _compare_obs(env, ob, (tag, "behind the end"))
                env.reset()
                ob.reset_packed(nxt)
    finally:
        env.close()
    print(f"ROUTING-LAYOUTS {name}: B={B} {len(teams)} episodes of {T} steps, {time.time() - t_start:.2f} s")
