"""Step, reset and gather emission into guarded, misplaced, dirty tensors (tests/emission_cases.py), on the device.

Every case of the table runs under both store policies.  The observation tensors are views into sentinel-filled buffers
(PlacedAllocator): a guard in front and behind, the cell tensors at the case's offsets, the feature tensors off by their
element size, nothing zeroed.  After EVERY call one device -> host copy of each buffer is compared, byte for byte, with a
host shadow of what the buffer must hold: the oracle's observation in the rows the call writes, the bytes from before
everywhere else -- the sentinel in a slot the test has just dirtied -- and the sentinel in both guards.  So a store that
is dropped, forgotten, moved a few bytes or issued past the end shows, also where it writes a 0.

Measured on an MI355X, whole -m gpu suite in one run (619 tests, 251 s): the slowest test from before this file is
tests/test_gpu_parity.py::test_every_tensor_at_the_baseline_batches[c5-8192-None] at 32.43 s; the slowest id of this
file took 0.04 s in that run and 0.15 s (the first, with the imports) when the file ran alone (profiles/emission_cases.txt)."""
import numpy as np
import pytest

import emission_cases as ec
from handle_model import Run, _bytes_equal, _same_info
from pcbenv.config import KIND_PIN, KIND_SPATIAL

pytestmark = pytest.mark.gpu


class Shadow:
    """What every byte of every backing buffer must hold, kept on the host next to the model."""

    def __init__(self, run, alloc):
        self.run, self.alloc, self.cfg = run, alloc, run.cfg
        self.S, self.B = run.S, run.B
        self.want = {}
        for k, (start, n, shape, dtype) in alloc.where.items():
            assert shape[:2] == (self.S, self.B), (k, shape)
            self.want[k] = np.full(n, ec.SENTINEL, np.uint8).view(dtype).reshape(self.S, self.B, -1)

    def oracle_rows(self):
        """The oracle's observation of every row, float64 [B, n] per key."""
        return {k: v.reshape(self.B, -1) for k, v in self.run.model.obs_rows().items()}

    def in_device_type(self, k, rows64):
        """float64 rows as the bound tensor carries them: uint8 cells, float64 features, or the compact integers
        (include/pcbenv.h pcbenv_compact_features: all_components_feature[..., 4] as its numerator h * w)."""
        dtype = self.alloc.where[k][3]
        if dtype == np.float64:
            return rows64
        v = rows64
        if k == "all_components_feature":
            v = rows64.reshape(self.B, self.cfg.max_num_components, -1).copy()
            v[..., 4] = np.rint(v[..., 4] * float(self.cfg.height * self.cfg.width))
            v = v.reshape(self.B, -1)
        out = v.astype(dtype)
        assert np.array_equal(out.astype(np.float64), v), (k, "not an integer of the declared type")
        return out

    def dirty(self, slot):
        self.alloc.dirty(slot)
        for w in self.want.values():
            w[slot].view(np.uint8)[...] = ec.SENTINEL

    def wrote(self, slot, rows):
        self.rows64 = self.oracle_rows()
        assert set(self.rows64) == set(self.want)
        for k, w in self.want.items():
            w[slot, rows] = self.in_device_type(k, self.rows64[k])[rows]

    def check(self, tag, slot, rows):
        """`rows` of `slot` have just been written (wrote() has been told): every buffer against the shadow."""
        import torch
        from pcbenv.batched_env import FEATURE_KEYS, expand_compact_features
        for k, (front, inner, back) in self.alloc.snapshot().items():
            for side, g in (("front", front), ("back", back)):
                hit = np.flatnonzero(g != ec.SENTINEL)
                assert hit.size == 0, (tag, k, f"{side} guard written", "bytes", hit[:8].tolist(), "of", g.size)
            dtype = self.alloc.where[k][3]
            dev = inner.view(dtype).reshape(self.S, self.B, -1)
            want = self.want[k]
            if not _bytes_equal(dev, want):
                diff = (dev.view(np.uint8).reshape(self.S, self.B, -1) != want.view(np.uint8).reshape(self.S, self.B, -1))
                s, e = (int(v) for v in np.argwhere(diff.any(axis=2))[0])
                at = np.flatnonzero(diff[s, e])
                kind = "wrong bytes in a row the call writes" if (s == slot and rows[e]) else "a row the call does not write has changed"
                left = int((dev[s, e].view(np.uint8)[at] == ec.SENTINEL).sum())
                raise AssertionError((tag, k, kind, "slot", s, "row", e, "bytes", at[:8].tolist(), f"{at.size} differ, {left} of them still the sentinel"))
            # written whole: no element of a written row is still the sentinel
            item = dev[slot, rows].view(np.uint8).reshape(-1, dtype.itemsize)
            assert not (item == ec.SENTINEL).all(axis=1).any(), (tag, k, "a sentinel element is left in a written row")
            if self.run.env.compact_features and k in FEATURE_KEYS:  # raw above; here after expand_compact_features
                got = expand_compact_features(self.cfg, {k: torch.from_numpy(np.ascontiguousarray(self.alloc.typed(k, inner)[slot]))})[k].numpy()
                assert _bytes_equal(got.reshape(self.B, -1)[rows], self.rows64[k][rows]), (tag, k, "the expanded compact tensor is not the reference's")


def check_outputs(run, tag):
    """reward, done, info of every slot and _last_done against the model (as handle_model.Driver.compare)."""
    e, m = run.env, run.model
    r, d, inf = e.traj_reward.cpu().numpy(), e.traj_done.cpu().numpy(), e.traj_info.cpu().numpy()
    assert _bytes_equal(r, m.R), (tag, "reward", np.argwhere(r.view(np.uint64) != m.R.view(np.uint64))[:5].tolist())
    assert np.array_equal(d, m.D), (tag, "done", np.argwhere(d != m.D)[:5].tolist())
    assert _same_info(inf, m.I), (tag, "info")
    assert np.array_equal(e._last_done.cpu().numpy(), m.last_done()), (tag, "_last_done")


def run_case(name, policy):
    import torch
    case, plan = ec.CASES[name], ec.plan(name)
    cfg, B, S = case.cfg(), case.B, case.S
    alloc = ec.PlacedAllocator(case.offsets)
    run = Run(cfg, B, run_seed=plan.seed, queue_depth=case.Q, allocator=alloc, options=ec.POLICIES[policy], **case.kw)
    try:
        e, m = run.env, run.model
        for k, t in e.traj.items():  # the placement is what the predicates were evaluated for
            assert t.data_ptr() % 256 == alloc.offset(k, t.element_size()) % 256, k
        sh = Shadow(run, alloc)
        everyone = np.ones(B, bool)
        # the first reset (Run has made it) meets dirty tensors and must write every byte of slot 0, and nothing else
        sh.wrote(0, everyone)
        sh.check((name, "first reset"), 0, everyone)
        check_outputs(run, (name, "first reset"))
        run.compare_oracle((name, "first reset"))
        has_info = cfg.kind in (KIND_PIN, KIND_SPATIAL)
        for j, c in enumerate(plan.calls):
            tag = (name, policy, j, c["op"])
            if S > 1:  # the call writes the slot behind the selected one, dirtied just before
                e.select_slot(c["slot"])
                m.select(c["slot"])
                sh.dirty(c["slot"])
            assert e.slot == m.slot == c["slot"], tag
            rows = np.asarray(c["rows"], bool)
            if c["op"] in ("step", "fused"):
                drawn = e.sample_actions(c["t"]).cpu().numpy()
                assert np.array_equal(drawn, c["drawn"]), (tag, "sample_actions draws other actions than the sampling contract")
                if c["op"] == "fused":
                    a = e.rollout_step(c["t"])[-1].cpu().numpy()
                    assert np.array_equal(a, c["actions"]), (tag, "the fused launch took another action than sample_actions draws")
                else:
                    e.step(torch.from_numpy(c["actions"]))
                rr, dd, ii = m.step(c["actions"])
                assert np.array_equal(dd, c["done"]) and _bytes_equal(np.asarray(rr), c["reward"]), (tag, "the model left the plan")
                assert np.array_equal(e.done.cpu().numpy(), dd), (tag, "done")
                assert _bytes_equal(e.reward.cpu().numpy(), np.asarray(rr)), (tag, "reward")
                inf = e.info_raw.cpu().numpy()
                if has_info:
                    has = ~np.isnan(inf[:, 0])
                    assert _bytes_equal(inf[has], np.asarray(ii)[has]), (tag, "info")
                m.I[m.slot] = inf
            elif c["op"] in ("reset_mask", "reset_done"):
                if c["op"] == "reset_done":
                    assert np.array_equal(e._last_done.cpu().numpy() != 0, rows), (tag, "_last_done")
                    e.reset_done()
                else:
                    e.reset(torch.from_numpy(c["mask"]))
                m.reset(c["mask"])
            else:
                e.gather_(torch.from_numpy(c["index"]).to(e.device))
                take = m.gather(c["index"])
                assert np.array_equal(take, rows) and not rows.all() and rows.any(), tag
            sh.wrote(c["slot"], rows)
            sh.check(tag, c["slot"], rows)
            check_outputs(run, tag)
            if S == 1 or rows.all():
                run.compare_oracle(tag)
    finally:
        run.close()


@pytest.mark.parametrize("policy", list(ec.POLICIES))
@pytest.mark.parametrize("name", list(ec.CASES))
def test_emission(name, policy):
    run_case(name, policy)


def test_expand_compact_features_divides_on_the_device():
    """all_components_feature[..., 4] = h * w / (H * W) in float64, bit for bit, at a grid area that is no power of two:
    sp14x32_tail_slots showed torch multiplying by the reciprocal (9 / 448 and 22 more of the numerators 1..64 one bit off)."""
    import torch
    from pcbenv.batched_env import expand_compact_features
    cfg = ec.CASES["sp14x32_tail_slots"].cfg()
    area = cfg.height * cfg.width
    assert area == 448
    num = np.arange(1, 65, dtype=np.int16)
    compact = np.zeros((64, 5), np.int16)
    compact[:, 4] = num
    got = expand_compact_features(cfg, {"all_components_feature": torch.from_numpy(compact).to("cuda:0")})["all_components_feature"].cpu().numpy()
    want = num.astype(np.float64) / np.float64(area)
    assert (num.astype(np.float64) * (1.0 / area) != want).sum() == 23  # what the reciprocal would give
    assert _bytes_equal(got[:, 4], want) and not got[:, :4].any()
