"""pcbenv_gather on the GPU: fork / reorder episodes on the device, through the C ABI (BatchedPlacementEnv.gather_ and
direct calls), bit for bit.  The oracle for destination row i after a gather is OracleBatch.reset_packed with the
source's current instance record followed by a replay of the source's actions since its last reset; later resets of i
take the destination's own queue records.  Right after a gather every tensor row of i must equal the pre-gather
snapshot of the source row; every later step must equal the oracle (identical bytes, identical float64 bit patterns)."""
import numpy as np
import pytest
import torch

from pcbenv import EnvConfig, _lib, env_seed, named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.config import KIND_PIN, KIND_SPATIAL, KIND_SQUARE

from handle_model import Run, _bytes_equal  # the environment next to its host model (shared with the call-sequence tests)
from logits_cases import RAGGED

pytestmark = pytest.mark.gpu


def _perm_with_repeats(rng, B, src_B=None):
    src_B = src_B or B
    idx = rng.randint(0, src_B, size=B)
    idx[rng.rand(B) < 0.1] = -1
    return idx


@pytest.mark.parametrize("name", ["c2", "c3", "c4"])
def test_identity_and_keep_change_nothing(name):
    """arange and all -1: every tensor unchanged, and later steps equal those of a twin handle that never gathered."""
    cfg = named_config(name)
    a, b = (BatchedPlacementEnv(cfg, 32, queue_depth=2, run_seed=4, auto_reset=True) for _ in range(2))
    for e in (a, b):
        e.generate_instances()
        e.reset()

    def tensors(e):
        d = {k: v.cpu().numpy() for k, v in e.obs.items()}
        d.update(reward=e.reward.cpu().numpy(), done=e.done.cpu().numpy(), info=e.info_raw.cpu().numpy())
        return d
    for t in range(3 * cfg.max_num_components):
        if t % 5 == 2:
            before = tensors(a)
            idx = torch.arange(32, device=a.device) if t % 2 else torch.full((32,), -1, dtype=torch.int64, device=a.device)
            a.gather_(idx)
            after = tensors(a)
            for k in before:
                assert _bytes_equal(before[k], after[k]), (t, k)
        ra = a.rollout_step(t)[-1].cpu().numpy()
        rb = b.rollout_step(t)[-1].cpu().numpy()
        assert np.array_equal(ra, rb), t
        ta, tb = tensors(a), tensors(b)
        for k in ta:
            assert _bytes_equal(ta[k], tb[k]), (t, k)
    a.close(); b.close()


@pytest.mark.parametrize("name,reward", [("c1", "centroid"), ("c2", "centroid"), ("c3", "centroid"), ("c4", "centroid"),
                                         ("c3", "beam"), ("c3", "both")])
def test_permutation_with_repeats_mid_episode(name, reward):
    """A random index with repeats and -1 in the middle of episodes, same handle; then two episodes of device-sampled
    actions with auto-reset against the oracle -- and the explicit loop, gathering between step and reset_done."""
    cfg = named_config(name, reward) if name in ("c3", "c4") else named_config(name)
    rng = np.random.RandomState(11)
    L = max(cfg.max_num_components, 6)
    run = Run(cfg, 48, auto_reset=True)
    for t in range(4):
        run.step(t)
    run.gather(_perm_with_repeats(rng, 48))
    for t in range(4, 4 + 2 * L + 2):
        run.step(t)
        if t % 7 == 0:
            run.gather(_perm_with_repeats(rng, 48))
    run.close()
    run = Run(cfg, 32, auto_reset=False)
    pr = np.random.RandomState(2)
    for t in range(2 * L):
        run.step(t, fused=False, p_bad=0.03, rng=pr)
        if t % 3 == 1:
            run.gather(_perm_with_repeats(rng, 32))  # between the step and reset_done: reset_done acts on the forked flags
            assert np.array_equal(run.env._last_done.cpu().numpy(), run.last_done)
        run.reset_done()
    run.close()


def test_cross_handle_gather_and_errors():
    cfg = named_config("c3")
    rng = np.random.RandomState(5)
    src = Run(cfg, 64, run_seed=8, auto_reset=True)
    dst = Run(cfg, 256, run_seed=9, queue_depth=2, auto_reset=True)
    for t in range(5):
        src.step(t)
        dst.step(t)
    idx = _perm_with_repeats(rng, 256, 64)
    dst.gather(idx, src=src)
    for t in range(5, 5 + 2 * cfg.max_num_components):
        dst.step(t)
        src.step(t)
        if t % 6 == 0:
            dst.gather(_perm_with_repeats(rng, 256, 64), src=src)
    # out-of-range indices keep the row and set the error word
    bad = np.arange(256) % 64
    bad[[3, 70, 200]] = [64, -2, 100000]
    dst.env.gather_(torch.from_numpy(bad).to(dst.env.device), source=src.env)  # (rows checked below through the oracle)
    take = (bad >= 0) & (bad < 64)
    keep_hist = {i: list(dst.hist[i]) for i in np.flatnonzero(~take)}
    dst_inst = {i: dst.inst[i] for i in np.flatnonzero(~take)}
    rec = np.stack([src.inst[j] if take[i] else dst.inst[i] for i, j in enumerate(bad.clip(0, 63))])
    dst.ob.reset_packed(rec, take.astype(np.uint8))
    for i in np.flatnonzero(take):
        e = dst.ob.env(int(i))
        for a in src.hist[bad[i]]:
            e.step_raw(a)
        dst.inst[i], dst.hist[i] = src.inst[bad[i]], list(src.hist[bad[i]])
    for i in keep_hist:
        assert dst.inst[i] is dst_inst[i]
    dst.compare_oracle("out of range")
    err = torch.zeros(1, dtype=torch.int32, device=dst.env.device)
    idx_dev = torch.from_numpy(bad.astype(np.int32)).to(dst.env.device)
    L = dst.env._L
    assert L.pcbenv_gather(dst.env._h, src.env._h, idx_dev.data_ptr(), err.data_ptr(), dst.env._stream()) == _lib.PCBENV_OK
    assert int(err.item()) == 1
    with pytest.raises(IndexError):
        dst.env.gather_(idx_dev, source=src.env, check=True)
    dst.env.gather_(torch.full((256,), -1, device=dst.env.device), check=True)  # nothing out of range: no error
    assert L.pcbenv_gather(dst.env._h, src.env._h, None, None, dst.env._stream()) == _lib.PCBENV_EINVAL
    # a different definition
    other = BatchedPlacementEnv(named_config("c3", "both"), 64, queue_depth=1)
    other.generate_instances(); other.reset()
    with pytest.raises(ValueError):
        dst.env.gather_(idx_dev, source=other)
    assert L.pcbenv_gather(dst.env._h, other._h, idx_dev.data_ptr(), None, dst.env._stream()) == _lib.PCBENV_EINVAL
    other.close()
    # batch fields may differ: flags (no auto-reset on the source) and queue depth
    plain = BatchedPlacementEnv(cfg, 16, queue_depth=1, run_seed=1)
    plain.generate_instances(); plain.reset()
    dst.env.gather_(torch.full((256,), -1, device=dst.env.device), source=plain)
    plain.close()
    src.close(); dst.close()


@pytest.mark.parametrize("name,kw", [
    ("c2", dict(num_slots=5)), ("c4", dict(num_slots=5)), ("c4", dict(num_slots=5, compact_features=True)),
    ("c3", dict(num_slots=4, compact_features=True, mask_marginals=True)), ("c2", dict(mask_marginals=True)),
    ("c3", dict(incremental_obs=True)), ("c4", dict(incremental_obs=True)),
    ("c3", dict(threads_per_env=256)), ("c4", dict(threads_per_env=256)), ("c4", dict(threads_per_env=64, num_slots=3)),
    ("c5", dict()), ("c5", dict(num_slots=3))])
def test_layouts(name, kw):
    cfg = named_config(name)
    B = 8 if name == "c5" else 32
    rng = np.random.RandomState(3)
    run = Run(cfg, B, auto_reset=True, **kw)
    steps = cfg.max_num_components + 6 if name != "c5" else 12
    for t in range(steps):
        run.step(t)
        if t % 4 == 1:  # (trajectory layout: into the selected slot, the one the step just wrote)
            run.gather(_perm_with_repeats(rng, B))
    run.close()


def _spatial_max():
    return EnvConfig.spatial(128, 128, 9, 9, 2, 8, 2, 8, 64, 40, 8, 16, 16, 4, "both", 4, 0.5)


EDGE_CONFIGS = dict(RAGGED, spatial_max=_spatial_max)


@pytest.mark.parametrize("name,kw", [
    ("spatial_7x100", dict()), ("spatial_7x100", dict(threads_per_env=256)), ("pin_100x9", dict()), ("rect_33x65", dict()),
    ("pin_40x48", dict(num_slots=3, compact_features=True)), ("spatial_max", dict(threads_per_env=64))],
    ids=["spatial_7x100", "spatial_7x100-t256", "pin_100x9", "rect_33x65", "pin_40x48-slots3-compact", "spatial_max-t64"])
def test_edge_shapes(name, kw):
    """test_layouts at the ragged and maximal shapes: two mask words per row with padding bits behind W on one and on four
    wavefronts, more rows than lanes, one valid bit in word 1, H != W with compact features, and 128 rows, 64 components
    and up to 256 pins on 64 lanes."""
    cfg = EDGE_CONFIGS[name]()
    B = 4 if name == "spatial_max" else 16
    rng = np.random.RandomState(3)
    run = Run(cfg, B, auto_reset=True, **kw)
    steps = cfg.max_num_components + 6 if name != "spatial_max" else 12
    moved = 0
    for t in range(steps):
        run.step(t)
        if t % 4 == 1:  # (trajectory layout: into the selected slot, the one the step just wrote)
            idx = _perm_with_repeats(rng, B)
            moved += int((run.gather(idx) & (idx != np.arange(B))).sum())
    assert moved >= B  # (on the host alone: the indices are not all -1 or the identity)
    run.close()


@pytest.mark.parametrize("name,src_kw,dst_kw", [
    ("c3", dict(threads_per_env=64), dict(threads_per_env=256)),
    ("c3", dict(threads_per_env=256), dict(threads_per_env=64)),
    ("c4", dict(), dict(num_slots=4, compact_features=True)),
    ("c4", dict(num_slots=4, compact_features=True), dict()),
    ("c3", dict(incremental_obs=True), dict(mask_marginals=True)),
    ("spatial_7x100", dict(threads_per_env=64), dict(threads_per_env=256)),
    ("c3", dict(auto_reset=False), dict(auto_reset=True, queue_depth=5))],
    ids=["c3-t64-to-t256", "c3-t256-to-t64", "c4-inplace-to-slots4-compact", "c4-slots4-compact-to-inplace",
         "c3-incremental-to-marginals", "spatial_7x100-t64-to-t256", "c3-manual-to-auto-reset-q5"])
def test_cross_handle_rows_move(name, src_kw, dst_kw):
    """What the header promises of two handles of one definition -- num_envs, queue_depth, flags and threads_per_env may
    differ -- with rows that move: 16 source environments after 3 launches, 32 destination environments of another run
    seed after 7, an index with repeats and some -1.  Every taken row equals the source's pre-gather snapshot (Run.gather:
    compact features after expansion, marginals against the mask where only the destination binds them), then one more
    episode of the destination against the oracle."""
    cfg = named_config(name) if name in ("c3", "c4") else RAGGED[name]()
    rng = np.random.RandomState(13)
    src = Run(cfg, 16, run_seed=8, **dict(dict(auto_reset=True), **src_kw))
    dst = Run(cfg, 32, run_seed=9, **dict(dict(auto_reset=True), **dst_kw))
    for t in range(3):
        src.step(t)
    for t in range(7):
        dst.step(t)
    idx = _perm_with_repeats(rng, 32, 16)
    assert ((idx >= 0).sum() >= 16) and (idx < 0).any() and len(set(idx[idx >= 0])) < (idx >= 0).sum()
    take = dst.gather(idx, src=src)
    assert take.sum() >= 16
    for i in np.flatnonzero(take):  # the rows did move: the destination's episodes are the source's, three transitions old
        assert len(dst.hist[i]) == len(src.hist[idx[i]]) and dst.inst[i] is src.inst[idx[i]]
    for t in range(7, 7 + cfg.max_num_components + 1):
        dst.step(t)
    src.step(3)  # the source goes on as if nothing had happened
    src.close(); dst.close()


@pytest.mark.parametrize("name,B", [("c3", 512), ("c4", 256)])
def test_staggered_episodes_with_helper_teams(name, B):
    """Episode phases spread over the batch (1 / L of it terminal in every launch, helper teams on): gathers while
    environments sit on the terminal list must still match the oracle."""
    cfg = named_config(name)
    L = cfg.max_num_components
    rng = np.random.RandomState(9)
    run = Run(cfg, B, auto_reset=True)
    for t in range(3 * L):
        run.step(t, fused=bool(t % 2))
        if t < L:
            m = (np.arange(B) % L == t).astype(np.uint8)
            run.env.reset(torch.from_numpy(m))
            run.oracle_reset(m)
        if t % 3 == 2:
            run.gather(_perm_with_repeats(rng, B), check_snapshot=(t % 6 == 2))
    run.close()


@pytest.mark.parametrize("name", ["c3", "c4"])
def test_device_generator_streams_stay_the_destinations(name):
    cfg = named_config(name)
    B = 64
    rng = np.random.RandomState(4)
    run = Run(cfg, B, queue_depth=8, device_instances=True, auto_reset=True, max_resets=16)
    for t in range(3 * cfg.max_num_components):
        run.step(t)
        if t % 5 == 3:
            before = run.env.queue_cursors()
            run.gather(_perm_with_repeats(rng, B))
            assert run.env.queue_cursors() == before
    assert run.env.device_instance_errors() == 0 and int(run.cursor.max()) < len(run.fresh)
    run.close()


def test_fused_sampler_right_after_a_gather():
    """The presampled action is cleared by a gather: the fused launch right after it draws what k_sample draws from the
    new mask (Run.step asserts it), and the results equal the oracle -- same handle and across handles with equal seeds."""
    cfg = named_config("c3")
    rng = np.random.RandomState(1)
    a = Run(cfg, 32, run_seed=5, auto_reset=True)
    b = Run(cfg, 32, run_seed=5, auto_reset=True)
    for t in range(20):
        a.step(t)
        b.step(t)
        a.gather(rng.permutation(32))
        a.gather(rng.randint(0, 32, 32), src=b)
    a.close(); b.close()


def test_best_of_k_vs_oracle():
    from oracle import oracle as orc
    from pcbenv.search import best_of_k
    cfg = named_config("c3")
    P, k = 8, 6
    root = Run(cfg, P, run_seed=6, auto_reset=False)
    for t in range(3):
        root.step(t)
    planner = BatchedPlacementEnv(cfg, P * k, queue_depth=1, run_seed=7)
    planner.generate_instances(); planner.reset()
    res = best_of_k(root.env, planner, k, step_index=1000)
    reward, child, acts, length, all_r = (x.cpu().numpy() for x in (res.reward, res.child, res.actions, res.length, res.child_rewards))
    assert _bytes_equal(reward, all_r.max(axis=1)) and np.array_equal(child // k, np.arange(P))
    assert _bytes_equal(all_r[np.arange(P), child % k], reward)
    ob = orc.OracleBatch(cfg, 1)
    for p in range(P):
        ob.reset_packed(root.inst[p][None])
        e = ob.env(0)
        assert length[p] >= 1
        for a in root.hist[p]:
            e.step_raw(a)
        for s in range(int(length[p])):
            r, d, _ = e.step_raw(acts[s, p])
            assert d == (s == length[p] - 1), (p, s)
        assert np.float64(r).tobytes() == np.float64(reward[p]).tobytes(), (p, r, reward[p])
    planner.close(); root.close()
