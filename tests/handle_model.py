"""A host model of one pcbenv handle, and seeded call sequences over the whole call alphabet (plain module, no test).

HandleModel keeps, next to an OracleBatch, what the oracle needs to follow every call of the C ABI: per row the instance
record of the current episode, the actions since its last reset, the reset count (the queue cursor) and `last_done`;
the queue contents per slot; the selected trajectory slot; what reward / done / info of every slot must hold, and which
rows of which slot show the current state.  A gather and a restore are modelled as "reset the oracle row with the
record, replay the actions".  Needs no GPU.

Run (the class tests/test_gather_gpu.py grew) and Driver put a BatchedPlacementEnv next to a model and compare after
every call: every observation tensor (`first_mismatch` per key, compact features after expansion), reward, done, info,
the mask marginals against the mask, and `mask_bits()` against the oracle's action mask -- bit for bit.

SETUPS is the table of handle configurations, `schedule(setup, seed)` a pure function giving the list of ops of one
sequence; tests/test_handle_model.py checks the coverage conditions on the schedules alone.
"""
import zlib
from collections import Counter

import numpy as np

from pcbenv import EnvConfig, env_seed, named_config
from pcbenv.config import KIND_PIN, KIND_SPATIAL, KIND_SQUARE

from logits_cases import RAGGED


def _bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _same_info(a, b):
    """NaN in the same places, identical bits elsewhere."""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and _bytes_equal(np.where(na, 0.0, a), np.where(nb, 0.0, b))


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
class HandleModel:
    def __init__(self, cfg, B, num_slots=1, queue_depth=3, auto_reset=False, run_seed=3, device_instances=False):
        from oracle import oracle as orc
        self.cfg, self.B, self.S, self.Q = cfg, B, num_slots, queue_depth
        self.auto_reset, self.square = bool(auto_reset), cfg.kind == KIND_SQUARE
        self.ob = orc.OracleBatch(cfg, B)
        self.streams = self.fresh = self.queue = None
        if not self.square:
            from pcbenv.instances import NativeInstanceStreams
            self.streams = NativeInstanceStreams(cfg, [env_seed(run_seed, i) for i in range(B)])
            if device_instances:
                self.fresh = []  # record k of every stream, drawn as the cursors get there
            else:
                self.queue = [self.streams.next_packed() for _ in range(queue_depth)]  # what generate_instances() loads
        self.cursor = np.zeros(B, np.int64)
        self.inst = [None] * B
        self.hist = [[] for _ in range(B)]
        self.slot = 0
        S = num_slots
        self.R = np.zeros((S, B), np.float64)        # what traj_reward / traj_done / traj_info must hold
        self.D = np.zeros((S, B), np.uint8)
        self.I = np.full((S, B, 2), np.nan, np.float64)
        self.fresh_rows = np.zeros((S, B), bool)     # row i of slot s shows the current state of environment i
        self.ld = ("slot", 0)                        # BatchedPlacementEnv._last_done: a view of a slot's done, or values

    # -- records --------------------------------------------------------------------------------
    def record(self, i):
        c = int(self.cursor[i])
        if self.fresh is not None:
            while len(self.fresh) <= c:
                self.fresh.append(self.streams.next_packed())
            return self.fresh[c][i]
        return self.queue[c % self.Q][i]

    def refill(self, slot):
        self.queue[slot] = self.streams.next_packed()
        return self.queue[slot]

    def _oracle_rows(self, rows, inst, hist):
        """Rows `rows` of the oracle: reset with inst[i], then the actions hist[i] replayed."""
        rows = np.asarray(rows, bool)
        if self.square:
            for i in np.flatnonzero(rows):
                self.ob.env(int(i)).reset()
        elif rows.any():
            rec = np.stack([inst[i] if rows[i] else self.inst[i] for i in range(self.B)])
            self.ob.reset_packed(rec, rows.astype(np.uint8))
        for i in np.flatnonzero(rows):
            e = self.ob.env(int(i))
            for a in hist[i]:
                e.step_raw(a)

    def _wrote(self, s, rows):
        self.fresh_rows[:, rows] = False
        self.fresh_rows[s, rows] = True

    def last_done(self):
        return self.D[self.ld[1]] if self.ld[0] == "slot" else self.ld[1]

    # -- calls ------------------------------------------------------------------------------------
    def _oracle_reset(self, rows):
        rows = np.asarray(rows).astype(bool)
        if not self.square:
            rec = {int(i): self.record(int(i)) for i in np.flatnonzero(rows)}
            inst = [rec.get(i) for i in range(self.B)]
        else:
            inst = [None] * self.B
        self._oracle_rows(rows, inst, [[] for _ in range(self.B)])
        for i in np.flatnonzero(rows):
            self.inst[i], self.hist[i] = inst[i], []
        self.cursor[rows] += 1

    def reset(self, mask=None):
        rows = np.ones(self.B, bool) if mask is None else np.asarray(mask).astype(bool)
        self._oracle_reset(rows)
        s = self.slot
        self.R[s, rows], self.D[s, rows], self.I[s, rows] = 0.0, 0, np.nan
        self._wrote(s, rows)

    def reset_done(self):
        self.reset(self.last_done() != 0)

    def step(self, actions, slot=None, set_last_done=True):
        """One transition of every row (in-launch resets with auto_reset) into `slot` (default: the selected one).
        Returns the oracle's (reward, done, info); I[slot] is left to the caller, who sees where the device has info."""
        s = self.slot if slot is None else slot
        a = np.ascontiguousarray(actions, np.int32).reshape(self.B, 3)
        rr, dd, ii = self.ob.step(a)
        for i in range(self.B):
            self.hist[i].append(a[i].copy())
        if self.auto_reset:
            self._oracle_reset(dd)
        self.R[s], self.D[s] = rr, dd
        self._wrote(s, np.ones(self.B, bool))
        if set_last_done:
            self.ld = ("slot", s)
        return rr, dd, ii

    def select(self, slot):
        self.slot = int(slot) % self.S

    def gather(self, idx, src=None):
        """Row i continues the episode of row idx[i] of `src` (-1 or out of range: keeps its own).  Returns the rows taken."""
        src = src or self
        idx = np.asarray(idx, np.int64)
        take = (idx >= 0) & (idx < src.B)
        j = idx.clip(0, src.B - 1)
        inst = [src.inst[k] for k in j]
        hist = [list(src.hist[k]) for k in j]
        r, d, inf = src.R[src.slot][j].copy(), src.D[src.slot][j].copy(), src.I[src.slot][j].copy()
        # gather_: where _last_done lives outside the selected slot (either side), the taken rows' flags are the source's
        in_slot = self.ld == ("slot", self.slot) and src.ld == ("slot", src.slot)
        if not in_slot:
            self.ld = ("val", np.where(take, src.last_done()[j], self.last_done()).astype(np.uint8))
        self._oracle_rows(take, inst, hist)
        for i in np.flatnonzero(take):
            self.inst[i], self.hist[i] = inst[i], hist[i]
        s = self.slot
        self.R[s, take], self.D[s, take], self.I[s, take] = r[take], d[take], inf[take]
        self._wrote(s, take)
        return take

    def snapshot(self):
        """What state_dict() holds, in the model's terms."""
        s = self.slot
        return dict(inst=list(self.inst), hist=[list(h) for h in self.hist], cursor=self.cursor.copy(),
                    last_done=self.last_done().copy(), slot=s, R=self.R[s].copy(), D=self.D[s].copy(), I=self.I[s].copy(),
                    fresh=self.fresh_rows[s].copy())

    def restore(self, snap):
        """load_state_dict(): the oracle rows rebuilt by replay; the queue contents stay what they are now."""
        everyone = np.ones(self.B, bool)
        self._oracle_rows(everyone, snap["inst"], snap["hist"])
        self.inst, self.hist = list(snap["inst"]), [list(h) for h in snap["hist"]]
        self.cursor = snap["cursor"].copy()
        s = self.slot = snap["slot"]
        self.R[s], self.I[s] = snap["R"], snap["I"]
        self.D[s] = snap["last_done"]  # load_state_dict points _last_done at the selected slot's done and copies into it
        self.ld = ("slot", s)
        self.fresh_rows[:, :] = False
        self.fresh_rows[s] = snap["fresh"]

    def obs_rows(self):
        """The oracle's observation of every row, stacked per key (slow: the self-tests only)."""
        rows = [self.ob.env(i).obs() for i in range(self.B)]
        return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


# ---------------------------------------------------------------------------------------------------------------
# Run: an environment next to its model, driven by hand (tests/test_gather_gpu.py)
# ---------------------------------------------------------------------------------------------------------------
class Run:
    """A BatchedPlacementEnv next to its CPU oracle and, per row, what the oracle needs to rebuild it: the instance
    record of the current episode, the actions since its last reset and the number of resets (the queue cursor)."""

    def __init__(self, cfg, B, run_seed=3, queue_depth=3, device_instances=False, max_resets=64, **kw):
        from pcbenv.batched_env import BatchedPlacementEnv
        self.cfg, self.B, self.Q = cfg, B, queue_depth
        self.env = BatchedPlacementEnv(cfg, B, queue_depth=queue_depth, run_seed=run_seed, **kw)
        self.S = self.env.num_slots
        self.model = HandleModel(cfg, B, self.S, queue_depth, self.env.auto_reset, run_seed, device_instances)
        self.square = cfg.kind == KIND_SQUARE
        if device_instances:
            self.env.enable_device_instances()
        elif not self.square:
            packed = self.env.generate_instances()
            assert all(np.array_equal(p, q) for p, q in zip(packed, self.model.queue)), "the model's queue is not the handle's"
        self.ob = self.model.ob
        self.max_resets = max_resets
        self.env.reset()
        self.model.reset()

    # the model's bookkeeping under the names the gather tests use
    inst = property(lambda self: self.model.inst)
    hist = property(lambda self: self.model.hist)
    cursor = property(lambda self: self.model.cursor)
    fresh = property(lambda self: [None] * self.max_resets if self.model.fresh is not None else None)

    @property
    def last_done(self):
        return self.model.last_done()

    @last_done.setter
    def last_done(self, values):  # a test that steps the oracle itself (tests/test_sample_logits_gpu.py) says what the step returned
        self.model.ld = ("val", np.asarray(values, np.uint8))

    def oracle_reset(self, mask):
        self.model.reset(mask)

    def host_obs(self, f64=False):
        e = self.env
        out = {k: v.cpu().numpy() for k, v in (e.obs_f64() if f64 else e.obs).items()}
        if not f64:
            out.update({"marginal_" + k: v.cpu().numpy() for k, v in e.mask_marginals.items()})
            out.update(reward=e.reward.cpu().numpy(), done=e.done.cpu().numpy(), info=e.info_raw.cpu().numpy())
        return out

    def host_rows(self):
        """host_obs() in the form two handles of one definition share whatever their layouts: the feature tensors as
        float64 (a compact layout expanded), reward / done / info, and the mask marginals where this handle binds them."""
        e = self.env
        out = self.host_obs(f64=True)
        out.update({"marginal_" + k: v.cpu().numpy() for k, v in e.mask_marginals.items()})
        out.update(reward=e.reward.cpu().numpy(), done=e.done.cpu().numpy(), info=e.info_raw.cpu().numpy())
        return out

    def same_layout(self, other):
        a, b = self.env, other.env
        return a.compact_features == b.compact_features and bool(a.mask_marginals) == bool(b.mask_marginals)

    def compare_oracle(self, tag):
        import torch
        obs = self.host_obs(f64=True)
        for k, v in obs.items():
            bad = self.ob.first_mismatch(k, v)
            assert bad < 0, (tag, k, bad)
        m = self.env.mask_marginals
        if m:  # marginals against the mask they summarise
            am = self.env.obs["action_mask"].reshape(self.B, -1, self.cfg.height, self.cfg.width)
            assert torch.equal(m["rows"], am.amax(dim=3)), tag
            assert torch.equal(m["orientation"], am.amax(dim=(2, 3))), tag

    def gather(self, idx, src=None, check_snapshot=True):
        """gather_ on the device; the snapshot and oracle bookkeeping on the host.  Returns the rows taken.  Between
        two handles whose tensors differ (compact against float64 features, marginals bound on one side only) the rows
        are compared as host_rows() gives them, key by key where the source has the key; marginals the source does not
        bind are checked against the mask by compare_oracle."""
        import torch
        src = src or self
        idx = np.asarray(idx, np.int64)
        take = (idx >= 0) & (idx < src.B)
        rows = Run.host_obs if self.same_layout(src) else Run.host_rows
        before_src = rows(src)
        before_own = before_src if src is self else rows(self)
        self.env.gather_(torch.from_numpy(idx).to(self.env.device), source=None if src is self else src.env)
        after = rows(self)
        if check_snapshot:
            assert set(after) - set(before_src) <= {"marginal_orientation", "marginal_rows"}
            for k, v in after.items():
                want = before_own[k].copy()
                if k not in before_src:  # marginals of a source that binds none: the rows kept must stay, the taken ones follow the mask
                    assert _bytes_equal(v[~take], want[~take]), ("snapshot", k, "a kept row changed")
                    continue
                want[take] = before_src[k][idx[take]]
                assert _bytes_equal(v, want), ("snapshot", k, np.flatnonzero([not _bytes_equal(v[i], want[i]) for i in range(self.B)])[:5])
        self.model.gather(idx, None if src is self else src.model)
        self.compare_oracle("after gather")
        return take

    def step(self, t, fused=True, p_bad=0.0, rng=None):
        import torch
        e = self.env
        if self.S > 1:
            e.select_slot(t + 1)
            self.model.select(t + 1)
        if fused:
            want = e.sample_actions(t).cpu().numpy()  # k_sample draws from the mask alone: a stale presample would differ
            _, r, d, _, a_dev = e.rollout_step(t)
            a = a_dev.cpu().numpy()
            assert np.array_equal(a, want), ("fused action", t)
        else:
            a = e.sample_actions(t).cpu().numpy()
            if p_bad:
                bad = rng.rand(self.B) < p_bad
                a[bad] = rng.randint(-1, 70, size=(int(bad.sum()), 3))
            _, r, d, _ = e.step(torch.from_numpy(a))
        rr, dd, ii = self.model.step(a)
        assert np.array_equal(d.cpu().numpy(), dd), ("done", t)
        assert _bytes_equal(r.cpu().numpy(), rr), ("reward", t)
        inf = e.info_raw.cpu().numpy()
        if self.cfg.kind in (KIND_PIN, KIND_SPATIAL):
            has = ~np.isnan(inf[:, 0])
            assert _bytes_equal(inf[has], ii[has]), ("info", t)
        self.model.I[self.model.slot] = inf
        self.compare_oracle(("step", t))
        return dd

    def reset_done(self):
        self.env.reset_done()
        self.model.reset_done()

    def close(self):
        self.env.close()


# ---------------------------------------------------------------------------------------------------------------
# the call alphabet, the setups and the schedules
# ---------------------------------------------------------------------------------------------------------------
OPS = ("step", "fused", "rollout", "reset_mask", "reset_done", "gather", "gather_x", "save", "load", "teams", "slot",
       "refill", "replay", "probe")          # ops 1..14 of the issue, in its order
PAIR_OPS = OPS[:13]                           # every ordered pair of these must occur; the probe bundle reads only
NEAR_REPLAY = ("step", "fused", "rollout", "reset_mask", "gather", "gather_x", "load", "teams")
TEAMS = (0, 16, 64, 48)


class Setup:
    """One handle configuration of the table.  `second`: a second handle of the same definition as gather source.
    `replay`: a step launch is captured into a graph early in the sequence and replayed by the `replay` op -- only with
    a host-fed queue (the generator works on a side stream) and in place (num_slots = 1: a captured launch writes the
    slot that was selected at capture time, and nothing on the host learns of its `done`)."""

    def __init__(self, name, cfg, B, seeds, length, auto_reset=True, queue_depth=3, device_instances=False, second=False,
                 replay=True, **kw):
        self.name, self.cfg, self.B, self.seeds, self.length = name, cfg, B, tuple(seeds), length
        self.auto_reset, self.Q, self.device_instances, self.second, self.kw = auto_reset, queue_depth, device_instances, second, kw
        self.S = kw.get("num_slots", 1)
        self.replay = replay and not device_instances and self.S == 1

    def config(self):
        return self.cfg()

    def alphabet(self):
        kind = self.config().kind
        ops = ["step", "fused", "reset_mask", "gather", "save", "load", "probe"]
        if self.auto_reset:
            ops.append("rollout")       # the persistent rollout restarts episodes in the launch
        else:
            ops.append("reset_done")
        if self.second:
            ops.append("gather_x")
        if kind in (KIND_PIN, KIND_SPATIAL):
            ops.append("teams")         # reward helpers exist for the routed kinds only
        if self.S > 1:
            ops.append("slot")
        if not self.device_instances and kind != KIND_SQUARE:
            ops.append("refill")
        if self.replay:
            ops.append("replay")
        return tuple(o for o in OPS if o in ops)


def _small_spatial():
    return EnvConfig.spatial(10, 10, 3, 4, 2, 4, 2, 4, 6, 1, 2, 4, 5, 2, "both", 2, 0.5)


SETUPS = {s.name: s for s in (
    Setup("c1_square", lambda: named_config("c1"), 32, (0, 1), 50, auto_reset=False),
    Setup("c2_plain", lambda: named_config("c2"), 48, (0, 1), 60, auto_reset=False, second=True),
    Setup("c2_slots5_marginals", lambda: named_config("c2"), 64, (0, 1, 2), 70, num_slots=5, mask_marginals=True, second=True),
    Setup("c2_slots5_manual", lambda: named_config("c2"), 32, (0, 1, 2), 70, auto_reset=False, num_slots=5, mask_marginals=True,
          second=True),
    Setup("c3_full", lambda: named_config("c3"), 64, (0, 1, 2, 3), 70, second=True),
    Setup("c3_both_t256", lambda: named_config("c3", "both"), 32, (0, 1, 2), 70, auto_reset=False, second=True, threads_per_env=256),
    Setup("c3_b1024_helpers", lambda: named_config("c3"), 1024, (0,), 60, replay=False),
    Setup("c3_generator", lambda: named_config("c3"), 64, (0, 1), 60, queue_depth=8, device_instances=True),
    Setup("c4_t64", lambda: named_config("c4"), 32, (0, 1), 60, threads_per_env=64),
    Setup("c4_slots4_compact", lambda: named_config("c4"), 32, (0, 1, 2), 70, num_slots=4, compact_features=True, second=True),
    Setup("c4_incremental", lambda: named_config("c4"), 32, (0, 1), 60, auto_reset=False, incremental_obs=True),
    Setup("spatial_7x100", RAGGED["spatial_7x100"], 32, (0, 1), 60),
)}


def _sequence(setup, seed, seen):
    """One walk over the setup's alphabet: mostly towards the (op, next op) pair seen least so far, so that a few
    sequences cover every pair; `seen` carries the counts from the setup's earlier seeds."""
    rng = np.random.RandomState((zlib.crc32(setup.name.encode()) + 7919 * seed) & 0x7FFFFFFF)
    alpha = setup.alphabet()
    ops, saves = [], 0

    def arg_of(name):
        if name == "rollout":
            return int(rng.randint(1, 6))
        if name == "reset_mask":
            return float((0.1, 0.5, 1.0)[rng.randint(3)])
        if name == "load":
            return int(rng.randint(saves))
        if name == "teams":
            return int(TEAMS[rng.randint(4)])
        if name == "slot":
            return int(rng.randint(setup.S))
        if name == "refill":
            return int(rng.randint(setup.Q))
        return 0

    def push(name):
        nonlocal saves
        if ops:
            seen[(ops[-1][0], name)] += 1
        seen[name] += 1
        ops.append((name, arg_of(name), int(rng.randint(1 << 30))))
        saves += name == "save"

    for name in ("step", "save") + (("capture",) if setup.replay else ()):  # something to restore, a graph to replay
        push(name)
    while len(ops) < setup.length:
        cur = ops[-1][0]
        allowed = [o for o in alpha if o != "load" or saves]
        if rng.rand() < 0.8:
            least = min(seen[(cur, o)] for o in allowed)
            allowed = [o for o in allowed if seen[(cur, o)] == least]
            rare = min(seen[o] for o in allowed)  # and among those, towards the op run least often
            allowed = [o for o in allowed if seen[o] == rare]
        push(allowed[rng.randint(len(allowed))])
    return ops


def schedule(setup, seed):
    """The ops of sequence `seed` of `setup`, [(op, argument, op seed)]: a pure function of (setup name, seed)."""
    if isinstance(setup, str):
        setup = SETUPS[setup]
    seen = Counter()
    for s in range(seed):  # the earlier seeds' pairs: this one goes where they have not been
        _sequence(setup, s, seen)
    return _sequence(setup, seed, seen)


# ---------------------------------------------------------------------------------------------------------------
# Driver: runs a schedule on the device and compares with the model after every call
# ---------------------------------------------------------------------------------------------------------------
class Driver:
    def __init__(self, setup, run_seed=3, B=None, other=None):
        from pcbenv.batched_env import BatchedPlacementEnv
        cfg = setup.config()
        self.setup, self.cfg, self.B, self.other = setup, cfg, B or setup.B, other
        B = self.B
        self.env = BatchedPlacementEnv(cfg, B, queue_depth=setup.Q, run_seed=run_seed, auto_reset=setup.auto_reset, **setup.kw)
        self.model = HandleModel(cfg, B, setup.S, setup.Q, setup.auto_reset, run_seed, setup.device_instances)
        if setup.device_instances:
            self.env.enable_device_instances()
        elif cfg.kind != KIND_SQUARE:
            packed = self.env.generate_instances()
            assert all(np.array_equal(p, q) for p, q in zip(packed, self.model.queue)), "the model's queue is not the handle's"
        self.t = 0                 # step index of the next transition
        self.explicit = 0          # explicit steps so far: tuple and flat actions alternate
        self.last_actions = np.zeros((B, 3), np.int32)
        self.snaps, self.graph, self.static = [], None, None
        self.shown = None          # per slot, what every observation tensor held at the last comparison
        self.counts = Counter()
        self.env.reset()
        self.model.reset()
        self.compare("first reset")

    def close(self):
        self.graph = None
        self.env.close()
        if self.other:
            self.other.close()

    # -- comparisons -------------------------------------------------------------------------------
    def host_traj(self):
        from pcbenv.batched_env import FEATURE_KEYS, expand_compact_features
        e = self.env
        traj = dict(e.traj)
        if e.compact_features:
            traj.update(expand_compact_features(self.cfg, {k: v for k, v in e.traj.items() if k in FEATURE_KEYS}))
        return {k: v.cpu().numpy() for k, v in traj.items()}

    def check_slot(self, traj, s, rows, tag):
        """Slot s of the device tensors: rows `rows` against the oracle, the others against what they held before."""
        ob = self.model.ob
        for k, v in traj.items():
            dev = v[s]
            if self.shown is not None and not rows.all():
                old = self.shown[s][k]
                bad = [i for i in np.flatnonzero(~rows) if not _bytes_equal(dev[i], old[i])]
                assert not bad, (tag, "a row nothing wrote has changed", k, "slot", s, "rows", bad[:5])
            if rows.all():
                bad = ob.first_mismatch(k, dev)
                assert bad < 0, (tag, k, "slot", s, "first row", bad)
        if rows.any() and not rows.all():
            for i in np.flatnonzero(rows):
                want = ob.env(int(i)).obs()
                for k, v in traj.items():
                    assert np.array_equal(v[s][i].astype(np.float64), want[k]), (tag, k, "slot", s, "row", int(i))

    def compare(self, tag, traj=None):
        import torch
        e, m = self.env, self.model
        assert e.slot == m.slot, (tag, "selected slot", e.slot, m.slot)
        traj = traj or self.host_traj()
        if self.shown is None:  # fresh tensors are zero-filled
            self.check_slot(traj, m.slot, m.fresh_rows[m.slot], tag)
            zero = {k: np.zeros_like(v[0]) for k, v in traj.items()}
            for s in range(m.S):
                if s != m.slot:
                    for k, v in traj.items():
                        assert _bytes_equal(v[s], zero[k]), (tag, "an unwritten slot is not zero", k, s)
        else:
            for s in range(m.S):
                self.check_slot(traj, s, m.fresh_rows[s] if s == m.slot else np.zeros(m.B, bool), tag)
        self.shown = [{k: v[s].copy() for k, v in traj.items()} for s in range(m.S)]
        r, d, inf = e.traj_reward.cpu().numpy(), e.traj_done.cpu().numpy(), e.traj_info.cpu().numpy()
        assert _bytes_equal(r, m.R), (tag, "reward", np.argwhere(r.view(np.uint64) != m.R.view(np.uint64))[:5].tolist())
        assert np.array_equal(d, m.D), (tag, "done", np.argwhere(d != m.D)[:5].tolist())
        assert _same_info(inf, m.I), (tag, "info")
        assert np.array_equal(e._last_done.cpu().numpy(), m.last_done()), (tag, "_last_done")
        if e.traj_marginals:  # marginals against the mask they summarise, every slot
            am = e.traj["action_mask"].reshape(m.S, m.B, -1, self.cfg.height, self.cfg.width)
            assert torch.equal(e.traj_marginals["rows"], am.amax(dim=4)), (tag, "marginal rows")
            assert torch.equal(e.traj_marginals["orientation"], am.amax(dim=(3, 4))), (tag, "marginal orientation")
        bad = m.ob.first_mismatch("action_mask", self.unpacked_mask_bits())
        assert bad < 0, (tag, "mask_bits", "first row", bad)

    def unpacked_mask_bits(self):
        """mask_bits() as the oracle's action_mask: bit y of word [b, plane, x, y // 64]; orientation o reads plane o & 1."""
        cfg = self.cfg
        bits = self.env.mask_bits().cpu().numpy()                                     # int64 [B, 2, H, WW]
        cells = np.unpackbits(bits.view(np.uint8), axis=-1, bitorder="little")[..., :cfg.width]  # [B, 2, H, W]
        if cfg.kind == KIND_SQUARE:
            return np.ascontiguousarray(cells[:, 0])
        return np.ascontiguousarray(cells[:, [o & 1 for o in range(cfg.num_orientations)]])

    def check_step(self, traj, s, expect, tag, rdi):
        """After the oracle has taken the transition that wrote slot s: reward, done, info and every tensor of the slot."""
        rr, dd, ii = expect
        r, d, inf = (x[s] for x in rdi)
        assert np.array_equal(d, dd), (tag, "done", "slot", s, np.flatnonzero(d != dd)[:5].tolist())
        assert _bytes_equal(r, rr), (tag, "reward", "slot", s, np.flatnonzero(r.view(np.uint64) != rr.view(np.uint64))[:5].tolist())
        if self.cfg.kind in (KIND_PIN, KIND_SPATIAL):
            has = ~np.isnan(inf[:, 0])
            assert _bytes_equal(inf[has], ii[has]), (tag, "info", "slot", s)
        self.model.I[s] = inf
        if traj is not None:
            self.check_slot(traj, s, np.ones(self.B, bool), tag)

    def stepped(self, a, tag, set_last_done=True):
        """The device has taken one transition with actions `a` into the selected slot."""
        e = self.env
        self.last_actions = np.ascontiguousarray(a, np.int32).reshape(self.B, 3)
        expect = self.model.step(self.last_actions, set_last_done=set_last_done)
        rdi = (e.traj_reward.cpu().numpy(), e.traj_done.cpu().numpy(), e.traj_info.cpu().numpy())
        self.check_step(None, self.model.slot, expect, tag, rdi)
        self.t += 1
        self.compare(tag)

    # -- ops -------------------------------------------------------------------------------------------
    def op_step(self, arg, seed, tag):
        import torch
        e, cfg, B = self.env, self.cfg, self.B
        rng = np.random.RandomState(seed)
        a = e.sample_actions(self.t).cpu().numpy()
        bad = rng.rand(B) < 0.03
        flat = self.explicit % 2 == 1
        self.explicit += 1
        if flat:
            HW, A = cfg.height * cfg.width, cfg.num_orientations * cfg.height * cfg.width
            f = (a[:, 0] * HW + a[:, 1] * cfg.width + a[:, 2]).astype(np.int64)
            f[bad] = rng.randint(-5, A + 5, size=int(bad.sum()))
            e.step(torch.from_numpy(f.astype(np.int32)))
            ok = (f >= 0) & (f < A)  # out of range: no such action (the wrappers' decoding)
            a = np.stack([np.where(ok, f // HW, -1), np.where(ok, (f % HW) // cfg.width, -1), np.where(ok, f % cfg.width, 0)], axis=1)
        else:
            a[bad] = rng.randint(-1, 70, size=(int(bad.sum()), 3))
            if cfg.kind == KIND_SQUARE:
                a[:, 0] = 0
            e.step(torch.from_numpy(a))
        self.stepped(a, tag)

    def op_fused(self, arg, seed, tag):
        e = self.env
        want = e.sample_actions(self.t).cpu().numpy()  # drawn from the mask alone: a stale presampled action would differ
        a = e.rollout_step(self.t)[-1].cpu().numpy()
        assert np.array_equal(a, want), (tag, "the fused launch took another action than sample_actions draws")
        self.stepped(a, tag)

    def op_rollout(self, n, seed, tag, flat=False, draw_seed=None, first_env_index=None, t0=None, expect=None):
        """One rollout_steps(n).  flat / draw_seed / first_env_index / t0: the launch through the ABI itself, with the
        flat action format, another seed than the run seed, another first_env_index than the handle's, another
        step_index0 than the transitions so far.  expect(k) -> the [B, 3] actions step k must have recorded, asked when
        the model has taken the steps before k.  Returns the recorded actions as the device wrote them."""
        import torch
        e, m, cfg = self.env, self.model, self.cfg
        if t0 is not None:
            self.t = int(t0)
        if flat or draw_seed is not None or first_env_index is not None:
            from pcbenv import _lib
            rec = torch.full((n, self.B) if flat else (n, self.B, 3), -7, dtype=torch.int32, device=e.device)
            _lib.check(e._L.pcbenv_rollout_sampled(
                e._h, rec.data_ptr(), _lib.ACTION_FLAT if flat else _lib.ACTION_TUPLE, int(n),
                e.run_seed if draw_seed is None else int(draw_seed),
                e.first_env_index if first_env_index is None else int(first_env_index), self.t, e._stream()), e._h)
            rec = rec.cpu().numpy()
            assert (rec >= 0).all(), (tag, "an action the launch did not record (or a negative one)", np.argwhere(rec < 0)[:5].tolist())
            HW = cfg.height * cfg.width
            acts = np.stack([rec // HW, rec % HW // cfg.width, rec % cfg.width], axis=-1).astype(np.int32) if flat else rec
        else:
            rec = acts = e.rollout_steps(self.t, n).cpu().numpy()
        traj = self.host_traj()
        rdi = (e.traj_reward.cpu().numpy(), e.traj_done.cpu().numpy(), e.traj_info.cpu().numpy())
        for k in range(n):
            s = (m.slot + k) % m.S
            if expect is not None:
                want = expect(k)
                assert np.array_equal(acts[k], want), (tag, "step", k, "recorded actions", np.flatnonzero((acts[k] != want).any(axis=1))[:5].tolist())
            oracle = m.step(acts[k], slot=s, set_last_done=False)
            if k + m.S >= n:  # (an earlier step's slot has been overwritten by a later one)
                self.check_step(traj, s, oracle, (tag, "step", k), rdi)
                self.shown[s] = {key: v[s].copy() for key, v in traj.items()}
        self.last_actions = acts[n - 1]
        self.t += n
        e.select_slot(m.slot + n - 1)  # the slot the last transition wrote
        m.select(m.slot + n - 1)
        self.compare(tag, traj)
        return rec

    def op_reset_mask(self, p, seed, tag):
        import torch
        mask = (np.random.RandomState(seed).rand(self.B) < p).astype(np.uint8)
        self.env.reset(torch.from_numpy(mask))
        self.model.reset(mask)
        self.compare(tag)

    def op_reset_done(self, arg, seed, tag):
        self.env.reset_done()
        self.model.reset_done()
        self.compare(tag)

    def _gather(self, src, seed, tag):
        import torch
        rng = np.random.RandomState(seed)
        idx = rng.randint(0, src.B, size=self.B)
        idx[rng.rand(self.B) < 0.1] = -1
        self.env.gather_(torch.from_numpy(idx).to(self.env.device), source=None if src is self else src.env)
        self.model.gather(idx, None if src is self else src.model)
        self.compare(tag)

    def op_gather(self, arg, seed, tag):
        self._gather(self, seed, tag)

    def op_gather_x(self, arg, seed, tag):
        """The second handle first moves on by up to two calls of its own."""
        o = self.other
        rng = np.random.RandomState(seed)
        for _ in range(rng.randint(3)):
            name = ("step", "fused", "reset_mask")[rng.randint(3)]
            getattr(o, "op_" + name)(0.5, int(rng.randint(1 << 30)), (tag, "second handle", name))
        self._gather(o, seed + 1, tag)

    def op_save(self, arg, seed, tag):
        self.snaps.append((self.env.state_dict(), self.model.snapshot(), {k: v.copy() for k, v in self.shown[self.model.slot].items()}))
        self.compare(tag)

    def op_load(self, which, seed, tag):
        sd, snap, shown = self.snaps[which]
        self.env.load_state_dict(sd)
        self.model.restore(snap)
        self.shown[snap["slot"]] = {k: v.copy() for k, v in shown.items()}
        self.compare(tag)

    def op_teams(self, v, seed, tag):
        self.env.set_option("terminal_teams", v)
        self.compare(tag)

    def op_slot(self, s, seed, tag):
        self.env.select_slot(s)
        self.model.select(s)
        self.compare(tag)

    def op_refill(self, slot, seed, tag):
        got = self.env.refill_slot(slot)
        assert np.array_equal(got, self.model.refill(slot)), (tag, "refill_slot queued other records than the streams' next")
        self.compare(tag)

    def op_capture(self, arg, seed, tag):
        """An explicit step captured once, on one stream; nothing runs, so the model does not move."""
        import torch
        e = self.env
        self.static = e.sample_actions(self.t).clone()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            e.step(self.static)
        self.model.ld = ("slot", self.model.slot)  # (step() points _last_done at the selected slot's done)
        self.compare(tag)

    def op_replay(self, arg, seed, tag):
        import torch
        e = self.env
        e.sample_actions(self.t, out=self.static)  # the static tensor the captured launch reads
        a = self.static.cpu().numpy()
        self.graph.replay()
        torch.cuda.synchronize()
        self.stepped(a, tag, set_last_done=False)

    def op_probe(self, arg, seed, tag):
        """Calls that only read: nothing of the handle may change (the comparison behind it sees to that)."""
        import torch
        e, cfg, B = self.env, self.cfg, self.B
        a1, a2 = e.sample_actions(self.t), e.sample_actions(self.t)
        assert torch.equal(a1, a2), (tag, "sample_actions twice")
        bits = e.mask_bits()
        out = torch.full_like(bits, -1)
        assert e.mask_bits(out=out) is out and torch.equal(out, bits), (tag, "mask_bits(out=)")
        A = cfg.num_orientations * cfg.height * cfg.width
        logits = torch.full((B, A), 0.25, dtype=torch.float32, device=e.device)
        drawn = e.sample_logits(logits, self.t)[0]
        assert torch.equal(drawn, a1), (tag, "sample_logits with constant logits against sample_actions")
        last = np.clip(self.last_actions, 0, [cfg.num_orientations - 1, cfg.height - 1, cfg.width - 1]).astype(np.int32)
        last = torch.from_numpy(last).to(e.device)
        lp1, h1 = e.evaluate_logits_forward(logits, bits, last)
        lp2, h2 = e.evaluate_logits_forward(logits, bits, last)
        assert torch.equal(lp1.view(torch.int32), lp2.view(torch.int32)) and torch.equal(h1.view(torch.int32), h2.view(torch.int32)), (tag, "evaluate_logits twice")
        self.compare(tag)

    def run_op(self, i, op):
        name, arg, seed = op
        self.counts[name] += 1
        getattr(self, "op_" + name)(arg, seed, (i, name, arg))


def run_sequence(setup, seed, counts=None, before_op=None):
    """Sequence `seed` of `setup` on the device.  A failure names the setup, the seed and the ops executed so far:
    `run_sequence(SETUPS[name], seed)` reproduces it.  before_op(i, op), if given, is called before every op (the stream
    tests put a delay on the current stream there); the comparisons are the same either way."""
    if isinstance(setup, str):
        setup = SETUPS[setup]
    ops = schedule(setup, seed)
    other = Driver(setup, run_seed=11 + seed, B=max(8, setup.B // 2 if setup.B <= 128 else 64)) if setup.second else None
    drv = Driver(setup, run_seed=3 + seed, other=other)
    done = []
    try:
        for i, op in enumerate(ops):
            done.append(op[:2])
            if before_op is not None:
                before_op(i, op)
            drv.run_op(i, op)
    except AssertionError as err:
        raise AssertionError(f"setup={setup.name} seed={seed} failed at op {len(done) - 1} {done[-1]}: {err.args[0] if err.args else ''}"
                             f" | ops so far: {done}") from err
    finally:
        if counts is not None:
            counts.update(drv.counts)
        drv.close()
    return drv.counts
