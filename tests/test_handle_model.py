"""The call-sequence schedules and the host model of tests/handle_model.py, without a GPU.

The schedules must reach every op and every ordered pair of ops (the product of "what was called before" and "what is
called now" is what tests/test_call_sequences_gpu.py is there to explore); the model's snapshot / restore and its
gather-by-replay must leave the oracle rows where a twin OracleBatch gets by stepping directly."""
from collections import Counter

import numpy as np
import pytest

from handle_model import NEAR_REPLAY, OPS, PAIR_OPS, SETUPS, HandleModel, schedule
from pcbenv import named_config


def _all_schedules():
    return {(name, seed): schedule(s, seed) for name, s in SETUPS.items() for seed in s.seeds}


def test_schedule_is_a_pure_function_of_setup_and_seed():
    for name, s in SETUPS.items():
        for seed in s.seeds:
            a, b = schedule(s, seed), schedule(name, seed)
            assert a == b and len(a) == s.length
        assert schedule(s, s.seeds[0]) != schedule(s, s.seeds[-1]) or len(s.seeds) == 1


def test_only_allowed_ops_are_scheduled():
    for (name, seed), ops in _all_schedules().items():
        s = SETUPS[name]
        allowed = set(s.alphabet()) | ({"capture"} if s.replay else set())
        saves = 0
        for op, arg, _ in ops:
            assert op in allowed, (name, seed, op)
            if op == "load":
                assert 0 <= arg < saves, (name, seed, "restores a snapshot that has not been taken")
            saves += op == "save"
        assert [o[0] for o in ops].count("capture") == (1 if s.replay else 0)


def test_every_op_occurs_five_times_in_every_setup_that_allows_it():
    sched = _all_schedules()
    for name, s in SETUPS.items():
        n = Counter(op for seed in s.seeds for op, _, _ in sched[(name, seed)])
        for op in s.alphabet():
            assert n[op] >= 5, (name, op, n[op])
    assert set(OPS) == {op for s in SETUPS.values() for op in s.alphabet()}


def _pairs(sched):
    return Counter((a[0], b[0]) for ops in sched.values() for a, b in zip(ops, ops[1:]))


def test_every_ordered_pair_of_ops_occurs():
    """Every (op, next op) of ops 1-13 that some setup allows together, directly adjacent in some sequence."""
    seen = _pairs(_all_schedules())
    possible = {(a, b) for s in SETUPS.values() for a in s.alphabet() for b in s.alphabet() if a in PAIR_OPS and b in PAIR_OPS}
    # never on one handle: rollout (auto-reset) with reset_done (none), slot (trajectory layout) with replay (in place)
    assert len(possible) == len(PAIR_OPS) ** 2 - 4
    missing = sorted(p for p in possible if seen[p] == 0)
    assert not missing, missing


def test_ops_next_to_a_replay():
    seen = _pairs(_all_schedules())
    for op in NEAR_REPLAY:
        assert seen[(op, "replay")] >= 1, ("never directly before a replay", op)
        assert seen[("replay", op)] >= 1, ("never directly after a replay", op)


def test_the_table_reaches_what_it_must():
    from pcbenv.config import KIND_PIN, KIND_RECT, KIND_SPATIAL, KIND_SQUARE
    S = list(SETUPS.values())
    assert {s.config().kind for s in S} == {KIND_SQUARE, KIND_RECT, KIND_PIN, KIND_SPATIAL}
    assert any(s.config().width == 100 for s in S)                                  # a ragged grid
    assert any(s.config().reward_type == "both" and s.config().kind == KIND_PIN for s in S)
    assert {s.kw.get("threads_per_env") for s in S} >= {64, 256}
    assert {s.auto_reset for s in S} == {True, False}
    assert any(s.S == 5 and s.kw.get("mask_marginals") for s in S) and any(s.kw.get("compact_features") for s in S)
    assert any(s.kw.get("incremental_obs") for s in S)
    assert any(s.device_instances and "replay" not in s.alphabet() for s in S)
    assert any(s.B == 1024 and s.config().kind == KIND_PIN for s in S)
    assert 10 <= len(S) <= 12


# ---- the model itself -------------------------------------------------------------------------------------------
def _legal_actions(model, rng):
    """A random legal action per row from the oracle's own mask (0, 0, 0 where there is none)."""
    a = np.zeros((model.B, 3), np.int32)
    for i in range(model.B):
        cells = np.argwhere(model.ob.env(i).obs()["action_mask"].reshape(-1, model.cfg.height, model.cfg.width) != 0)
        if len(cells):
            a[i] = cells[rng.randint(len(cells))]
    return a


def _assert_rows_equal(model, twin, rows, tag):
    want = twin.obs_rows()
    got = model.obs_rows()
    for k in want:
        for i, j in rows:
            assert np.array_equal(got[k][i], want[k][j]), (tag, k, i, j)


@pytest.mark.parametrize("name,auto_reset", [("c1", False), ("c2", True), ("c3", True), ("c3", False), ("c4", True)])
def test_model_snapshot_restore_equals_stepping_directly(name, auto_reset):
    cfg, B = named_config(name), 6
    rng = np.random.RandomState(4)
    model, twin = (HandleModel(cfg, B, auto_reset=auto_reset, run_seed=5) for _ in range(2))
    model.reset(); twin.reset()
    n = cfg.max_num_components + 3 if name != "c1" else 5
    for t in range(n):
        a = _legal_actions(model, rng)
        if t % 4 == 3:
            a[t % B] = (-1, 0, 0)  # an action that is not one
        out = model.step(a)
        want = twin.step(a)
        assert all(np.array_equal(x, y) for x, y in zip(out, want))
    snap = model.snapshot()
    for t in range(4):  # the model wanders off ...
        model.step(_legal_actions(model, rng))
        if t == 1:
            model.reset(np.arange(B) % 2)
    model.restore(snap)  # ... and comes back by replay to where the twin went step by step
    _assert_rows_equal(model, twin, [(i, i) for i in range(B)], "restore")
    assert np.array_equal(model.cursor, twin.cursor) and np.array_equal(model.last_done(), twin.last_done())
    a = _legal_actions(twin, rng)
    out, want = model.step(a), twin.step(a)  # and goes on as the twin does, resets from the queue included
    assert all(np.array_equal(x, y) for x, y in zip(out, want))
    _assert_rows_equal(model, twin, [(i, i) for i in range(B)], "step after restore")


@pytest.mark.parametrize("name", ["c1", "c2", "c3", "c4"])
def test_model_gather_by_replay_equals_stepping_directly(name):
    cfg, B = named_config(name), 6
    rng = np.random.RandomState(7)
    model, twin = (HandleModel(cfg, B, auto_reset=False, run_seed=2) for _ in range(2))
    model.reset(); twin.reset()
    for t in range(3):
        a = _legal_actions(model, rng)
        model.step(a); twin.step(a)
    idx = np.array([3, -1, 0, 3, 9, 1])  # repeats, keep, out of range
    cursor = model.cursor.copy()
    take = model.gather(idx)
    assert take.tolist() == [True, False, True, True, False, True]
    _assert_rows_equal(model, twin, [(i, int(idx[i]) if take[i] else i) for i in range(B)], "gather")
    assert np.array_equal(model.cursor, cursor), "the queue cursors stay the destination's"
    # the forked rows go on as their sources do: the same action on both sides
    a = _legal_actions(twin, rng)
    want = twin.step(a)
    src = np.where(take, idx, np.arange(B))
    out = model.step(a[src])
    assert all(np.array_equal(x, y[src]) for x, y in zip(out, want))
    _assert_rows_equal(model, twin, [(i, int(src[i])) for i in range(B)], "step after gather")
    # across two models: rows of another batch, with its records
    other = HandleModel(cfg, 4, auto_reset=False, run_seed=9)
    other.reset()
    b = _legal_actions(other, rng)
    other.step(b)
    model.gather(np.array([0, 1, 2, 3, -1, 0]), other)
    _assert_rows_equal(model, other, [(0, 0), (1, 1), (2, 2), (3, 3), (5, 0)], "gather from another batch")


def test_model_queue_and_refill():
    """Reset k of row i takes queue slot (resets so far) % depth as it is filled at that moment."""
    cfg, B = named_config("c3"), 4
    model = HandleModel(cfg, B, queue_depth=2, run_seed=1)
    first = [q.copy() for q in model.queue]
    model.reset()
    assert all(np.array_equal(model.inst[i], first[0][i]) for i in range(B))
    snap = model.snapshot()
    model.reset(np.array([1, 0, 0, 0]))
    assert np.array_equal(model.inst[0], first[1][0]) and model.cursor.tolist() == [2, 1, 1, 1]
    new = model.refill(1).copy()
    assert not np.array_equal(new, first[1])
    model.restore(snap)  # an older cursor resolves to what the slot holds now
    model.reset(np.array([1, 1, 0, 0]))
    assert np.array_equal(model.inst[0], new[0]) and np.array_equal(model.inst[1], new[1])
