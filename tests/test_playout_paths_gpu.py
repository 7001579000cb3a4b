"""pcbenv_playout_paths on the GPU, through BatchedPlacementEnv.playout(paths=...) and direct calls of the C ABI, bit for
bit against the CPU oracle (path_cases.oracle_path_playout) on plans made before any device call (path_cases.Plan: per
root an empty path, two prefixes of the playout's own path-less twin, a prefix of a sibling and a path with an illegal
action; tests/test_path_cases.py checks on the CPU that every plan holds every kind of end).  The roots are brought to the
plan with test_playout_gpu.device_roots.  60 playouts per launch (40 where a case has 8 roots)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from pcbenv import _lib, named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.config import KIND_SQUARE

import path_cases as pa
import playout_cases as pc
from handle_model import _bytes_equal, _same_info
from stream_cases import LAG_MS, lagged
from test_playout_gpu import _forced_cases, check_against, device_roots

pytestmark = pytest.mark.gpu

K, STEP0 = pa.K, pa.STEP0
_PLANS = {}


def plan_of(name, parity=0):
    if (name, parity) not in _PLANS:
        _PLANS[name, parity] = pa.Plan(name, parity)
    return _PLANS[name, parity]


def defined_bits(cfg):
    """uint64 [2, 1, WW]: the bits of a leaf mask the contract defines (columns < W; plane 0 only for the square kind)."""
    W, WW = cfg.width, (cfg.width + 63) // 64
    m = np.zeros((2, 1, 64 * WW), np.uint8)
    m[:, :, :W] = 1
    if cfg.kind == KIND_SQUARE:
        m[1] = 0
    return np.packbits(m, axis=-1, bitorder="little").view(np.uint64)


def check_leaf(leaf, expected, cfg, rows=None):
    got = (leaf.cpu().numpy() if isinstance(leaf, torch.Tensor) else leaf).view(np.uint64)
    keep = defined_bits(cfg)
    for i, e in enumerate(expected):
        if rows is None or i in rows:
            assert np.array_equal(got[i] & keep, e["leaf"] & keep), (i, "leaf mask")


@pytest.mark.parametrize("name, parity", [(n, 0) for n in pa.GPU_CASES] + [(n, 1) for n in pa.BOTH_PARITIES])
def test_paths_against_the_oracle(name, parity):
    """Every kind and team shape (one and four wavefronts, one and two mask words, more rows than lanes, a grid the first
    placement fills); c3_centroid and spatial_7x100 after an even and an odd number of step launches (the state sets are
    double-buffered).  Path rows behind a path's end hold an action that is no action: they are never read."""
    plan = plan_of(name, parity)
    cfg, n = plan.cfg, plan.n
    figures, missing = pa.mix(plan)
    print(f"PATH-MIX {name} parity {parity}: {figures}")
    assert not missing, (missing, figures)
    run = device_roots(plan.roots)
    dev = run.env.device
    paths = torch.from_numpy(plan.path_tensor(fill=-9)).to(dev)
    plen = torch.from_numpy(plan.path_len).to(dev)
    po = run.env.playout(k=K, step_index=STEP0, paths=paths, path_len=plen, leaf_mask=True, max_steps=plan.limit, check=True)
    assert po.actions.shape == (plan.limit, n, 3) and po.leaf_mask.shape == (n, 2, cfg.height, (cfg.width + 63) // 64)
    assert po.leaf_mask.dtype == torch.int64
    check_against(po, plan.expected, cfg)
    check_leaf(po.leaf_mask, plan.expected, cfg)
    # path_len == 0 for everyone: the path-less playouts, and every leaf is its root's own mask -- the whole row, word for word
    po0 = run.env.playout(k=K, step_index=STEP0, paths=paths, path_len=torch.zeros_like(plen), leaf_mask=True, max_steps=plan.limit)
    check_against(po0, plan.base, cfg)
    own = run.env.mask_bits()[torch.tensor(plan.root_of, device=dev)]
    assert torch.equal(po0.leaf_mask, own)
    check_leaf(po0.leaf_mask, [dict(leaf=pa.leaf_of(cfg, plan.roots.model.ob.env(r))) for r in plan.root_of], cfg)
    # ... and the same through the old entry point (no path keyword at all)
    old = run.env.playout(k=K, step_index=STEP0, max_steps=plan.limit)
    assert old.leaf_mask is None
    for f in ("reward", "done", "length", "actions"):
        assert _bytes_equal(getattr(old, f).cpu().numpy(), getattr(po0, f).cpu().numpy()), f
    run.compare_oracle("the roots after the playouts")
    run.close()


def _same_playout(a, b):
    for f in ("reward", "done", "length", "actions"):
        assert _bytes_equal(getattr(a, f).cpu().numpy(), getattr(b, f).cpu().numpy()), f
    assert (a.info is None) == (b.info is None)
    if a.info is not None:
        assert _same_info(a.info.cpu().numpy(), b.info.cpu().numpy())


@pytest.mark.parametrize("name, flat", [("c3_centroid", False), ("spatial_7x100", True)], ids=["tuple", "spatial_7x100-flat"])
def test_one_path_step_is_a_forced_first_action(name, flat):
    """path_steps == 1 equals playout(first_actions=...) bit for bit: legal, illegal and out-of-range actions, both formats."""
    roots = plan_of(name).roots
    cfg, P = roots.cfg, roots.P
    first, kinds = _forced_cases(roots)
    H, W, A = cfg.height, cfg.width, cfg.num_orientations * cfg.height * cfg.width
    given = first
    if flat:
        given = first[:, 0].astype(np.int64) * H * W + first[:, 1] * W + first[:, 2]
        for i, k in enumerate(kinds):
            if k == "range":
                given[i] = (-3, A, A + 12345)[(i // 4) % 3]
        given = given.astype(np.int32)
    run = device_roots(roots)
    dev = run.env.device
    idx = torch.arange(P, dtype=torch.int32, device=dev)
    g = torch.from_numpy(given).to(dev)
    want = run.env.playout(index=idx, step_index=STEP0, first_actions=g)
    got = run.env.playout(index=idx, step_index=STEP0, paths=g[None], leaf_mask=True)
    _same_playout(got, want)
    assert int((want.length == 1).sum()) >= 4 and int((want.length > 1).sum()) >= 1
    with pytest.raises(ValueError):
        run.env.playout(index=idx, first_actions=g, paths=g[None])
    with pytest.raises(ValueError):
        run.env.playout(index=idx, first_actions=g, leaf_mask=True)
    run.close()


def test_variants():
    """The flat format; path_len=None; actions_steps below the path length and 0; a root_index with repeats."""
    plan = plan_of("c3_centroid")
    cfg, n = plan.cfg, plan.n
    run = device_roots(plan.roots)
    dev = run.env.device
    tuples = plan.path_tensor()
    plen = torch.from_numpy(plan.path_len).to(dev)
    # flat: paths and the recorded actions
    po = run.env.playout(k=K, step_index=STEP0, paths=torch.from_numpy(plan.flat(tuples)).to(dev), path_len=plen, leaf_mask=True)
    assert po.actions.shape == (plan.limit, n)
    check_against(po, plan.expected, cfg)
    check_leaf(po.leaf_mask, plan.expected, cfg)
    # path_len=None: everyone walks path_steps = 2 steps of their path-less twin (a twin of length 1 ends on the path: its
    # second row, zeros, is not read for effect)
    two = [np.concatenate([b["actions"][:2], np.zeros((2, 3), np.int32)])[:2] for b in plan.base]
    want = plan.playouts(two, plan.limit)
    assert any(e["length"] < 2 for e in want) and any(e["length"] > 2 for e in want)
    po = run.env.playout(k=K, step_index=STEP0, paths=torch.from_numpy(plan.path_tensor(two)).to(dev), leaf_mask=True)
    check_against(po, want, cfg)
    check_leaf(po.leaf_mask, want, cfg)
    # actions_steps below the path length, and 0
    paths = torch.from_numpy(tuples).to(dev)
    assert plan.path_steps > 1
    po1 = run.env.playout(k=K, step_index=STEP0, paths=paths, path_len=plen, actions_steps=1, leaf_mask=True)
    assert po1.actions.shape == (1, n, 3)
    check_against(po1, plan.expected, cfg)
    check_leaf(po1.leaf_mask, plan.expected, cfg)
    po0 = run.env.playout(k=K, step_index=STEP0, paths=paths, path_len=plen, actions_steps=0)
    assert po0.actions is None and po0.leaf_mask is None
    check_against(po0, plan.expected, cfg)
    # a root_index with repeats: playout i walks the plan's path of playout index[i] * K + i % K from root index[i]
    index = np.array([0, 0, 3, 2, 5, 5, 1, 11, 3, 3, 7, 2], np.int32)
    some = [plan.paths[int(r) * K + i % K] for i, r in enumerate(index)]
    want = plan.playouts(some, plan.limit, root_of=[int(r) for r in index])
    po = run.env.playout(index=torch.from_numpy(index).to(dev), step_index=STEP0, paths=torch.from_numpy(plan.path_tensor(some)).to(dev),
                         path_len=torch.tensor([len(p) for p in some], dtype=torch.int32, device=dev), leaf_mask=True, check=True)
    check_against(po, want, cfg)
    check_leaf(po.leaf_mask, want, cfg)
    run.compare_oracle("the roots after the playouts")
    run.close()


GUARD, SENTINEL = 256, 0xA5


class Guarded:
    """Caller-owned outputs of a direct call, each in a buffer of its own with GUARD sentinel bytes on either side and
    filled with a value the kernel never writes."""

    def __init__(self, dev, n, steps, H, WW):
        self.back, self.t = {}, {}
        for k, (shape, dtype, fill) in dict(reward=((n,), torch.float64, -5.0), done=((n,), torch.uint8, 9), length=((n,), torch.int32, -9),
                                            info=((n, 2), torch.float64, 5.0), actions=((steps, n, 3), torch.int32, -7),
                                            leaf=((n, 2, H, WW), torch.int64, 0x1111), errors=((1,), torch.int32, 0)).items():
            nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
            b = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
            t = b[GUARD:GUARD + nbytes].view(dtype).view(shape)
            t.fill_(fill)
            self.back[k], self.t[k] = (b, nbytes), t

    def intact(self):
        for k, (b, nbytes) in self.back.items():
            h = b.cpu().numpy()
            assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + nbytes:] == SENTINEL).all(), (k, "a guard byte was written")

    def host(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}


def direct(env, n, index, paths, path_len, path_steps, max_steps, actions_steps, errors=True, stream=None):
    """pcbenv_playout_paths called directly with guarded tensors of the caller's own -> (rc, outputs on the host)."""
    cfg, dev = env.cfg, env.device
    g = Guarded(dev, n, max(actions_steps, 1), cfg.height, (cfg.width + 63) // 64)
    ptr = lambda t: None if t is None else t.data_ptr()
    R = _lib.PcbenvPlayoutRequest
    req = R(struct_size=C.sizeof(R), action_format=_lib.ACTION_TUPLE, root_index_dev=ptr(index), num_playouts=n, path_actions_dev=ptr(paths),
            path_len_dev=ptr(path_len), path_steps=path_steps, max_steps=max_steps, reward_dev=ptr(g.t["reward"]), done_dev=ptr(g.t["done"]),
            length_dev=ptr(g.t["length"]), info_dev=ptr(g.t["info"]), actions_out_dev=ptr(g.t["actions"]) if actions_steps else None,
            actions_steps=actions_steps, leaf_mask_bits_dev=ptr(g.t["leaf"]), errors_dev=ptr(g.t["errors"]) if errors else None,
            seed=env.run_seed, first_env_index=0, step_index0=STEP0, stream=(env._stream() if stream is None else stream).value)
    rc = env._L.pcbenv_playout_paths(env._h, C.byref(req))
    out = g.host()
    g.intact()
    return rc, out


def check_direct(out, expected, cfg, rows, actions_steps):
    for i in rows:
        e = expected[i]
        assert out["length"][i] == e["length"] and out["done"][i] == e["done"], (i, out["length"][i], out["done"][i], e["length"], e["done"])
        assert out["reward"][i].tobytes() == e["reward"].tobytes(), i
        assert not pc.has_info(cfg) or _same_info(out["info"][i], e["info"]), i
        m = min(e["length"], actions_steps)
        assert np.array_equal(out["actions"][:m, i], e["actions"][:m]) and (out["actions"][m:, i] == -7).all(), i
    check_leaf(out["leaf"], expected, cfg, rows=set(rows))


@pytest.mark.parametrize("name", ["c3_centroid", "spatial_7x100_t256", "rect_11x10"])
def test_guarded_outputs_and_refused_rows(name):
    """Every output in a sentinel-guarded buffer of its own.  First the plan as it is; then one out-of-range root and two
    out-of-range path_len (above path_steps, negative) in a single launch: both error bits, the refused rows report
    length 0, done 0, reward 0.0, NaN info, a zero leaf mask and no action row, and their neighbours are correct."""
    plan = plan_of(name)
    cfg, n = plan.cfg, plan.n
    run = device_roots(plan.roots)
    dev = run.env.device
    paths = torch.from_numpy(plan.path_tensor(fill=-9)).to(dev)
    plen = torch.from_numpy(plan.path_len).to(dev)
    index = torch.tensor(plan.root_of, dtype=torch.int32, device=dev)
    rc, out = direct(run.env, n, None, paths, plen, plan.path_steps, plan.limit, plan.limit)
    assert rc == _lib.PCBENV_OK and out["errors"][0] == 0
    check_direct(out, plan.expected, cfg, range(n), plan.limit)
    bad_root, bad_len_hi, bad_len_lo = 7, 21, 33
    index[bad_root] = plan.P
    plen[bad_len_hi] = plan.path_steps + 1
    plen[bad_len_lo] = -1
    rc, out = direct(run.env, n, index, paths, plen, plan.path_steps, plan.limit, plan.limit)
    assert rc == _lib.PCBENV_OK and out["errors"][0] == 3
    refused = (bad_root, bad_len_hi, bad_len_lo)
    for i in refused:
        assert out["length"][i] == 0 and out["done"][i] == 0 and out["reward"][i].tobytes() == np.float64(0.0).tobytes(), i
        assert not pc.has_info(cfg) or np.isnan(out["info"][i]).all(), i
        assert (out["actions"][:, i] == -7).all() and not out["leaf"][i].any(), i
    check_direct(out, plan.expected, cfg, [i for i in range(n) if i not in refused], plan.limit)
    # one bit each
    index[bad_root] = plan.root_of[bad_root]
    rc, out = direct(run.env, n, index, paths, plen, plan.path_steps, plan.limit, plan.limit)
    assert rc == _lib.PCBENV_OK and out["errors"][0] == 2
    plen = torch.from_numpy(plan.path_len).to(dev)
    index[bad_root] = -1
    rc, out = direct(run.env, n, index, paths, plen, plan.path_steps, plan.limit, 0, errors=True)
    assert rc == _lib.PCBENV_OK and out["errors"][0] == 1 and (out["actions"] == -7).all()
    rc, out2 = direct(run.env, n, index, paths, plen, plan.path_steps, plan.limit, 0, errors=False)  # without an error word: the same rows
    assert rc == _lib.PCBENV_OK and all(_bytes_equal(out[k], out2[k]) for k in ("reward", "done", "length", "leaf"))
    with pytest.raises(IndexError):
        run.env.playout(index=index, step_index=STEP0, paths=paths, path_len=plen, check=True)
    run.compare_oracle("the roots after the playouts")
    run.close()


@pytest.mark.parametrize("name", ["small_pin", "c3_centroid", "spatial_7x100"])
def test_truncation(name):
    """max_steps cuts at the path's last action and right after it: d = 2 actions of the path-less twin, max_steps = 2 (no
    transition is drawn) and 3 (one is).  A cut playout reports done = 0 and the leaf mask is still the defined one -- the
    state after the path.  max_steps below path_steps is refused (path_steps is in 0 ... max_steps), so a cut cannot fall
    deeper inside a path than on its last action."""
    plan = plan_of(name, 1)
    cfg, n = plan.cfg, plan.n
    two = [b["actions"][:2] for b in plan.base]
    run = device_roots(plan.roots)
    dev = run.env.device
    paths = torch.from_numpy(plan.path_tensor(two, steps=2, fill=-9)).to(dev)
    plen = torch.tensor([len(p) for p in two], dtype=torch.int32, device=dev)
    for limit in (2, 3):
        want = plan.playouts(two, limit)
        cut = [i for i, e in enumerate(want) if not e["done"]]
        assert len(cut) >= 4 and all(want[i]["length"] == limit for i in cut) and any(e["done"] for e in want)
        rc, out = direct(run.env, n, None, paths, plen, 2, limit, limit)
        assert rc == _lib.PCBENV_OK
        check_direct(out, want, cfg, range(n), limit)
        for i in cut:
            assert out["done"][i] == 0 and out["reward"][i] == 0.0 and (not pc.has_info(cfg) or np.isnan(out["info"][i]).all())
        po = run.env.playout(k=K, step_index=STEP0, paths=paths, path_len=plen, max_steps=limit, leaf_mask=True)
        check_against(po, want, cfg)
        check_leaf(po.leaf_mask, want, cfg)
    # at max_steps = 2 the leaf of a cut playout is what the one-step-longer playout starts its draw from
    assert all(np.array_equal(a["leaf"], b["leaf"]) for a, b in zip(plan.playouts(two, 2), plan.playouts(two, 3)))
    with pytest.raises(ValueError):
        run.env.playout(k=K, paths=paths, path_len=plen, max_steps=1)
    rc, _ = direct(run.env, n, None, paths, plen, 2, 1, 0)
    assert rc == _lib.PCBENV_EINVAL
    run.close()


def test_state_errors():
    cfg = named_config("c2")
    env = BatchedPlacementEnv(cfg, 8, queue_depth=1, run_seed=1)
    paths = torch.zeros((1, 16, 3), dtype=torch.int32, device=env.device)
    with pytest.raises(_lib.PcbenvError) as ei:  # no episode yet
        env.playout(k=2, paths=paths)
    assert ei.value.code == _lib.PCBENV_ESTATE
    env.generate_instances()
    env.reset()
    po = env.playout(k=2, paths=paths[:0], leaf_mask=True)  # no path at all: null path_actions with path_steps == 0
    assert int(po.length.min()) >= 1 and torch.equal(po.leaf_mask, env.mask_bits().repeat_interleave(2, dim=0))
    rc, _ = direct(env, 12, None, None, None, 0, 3, 0)  # 12 playouts over 8 environments without an index
    assert rc == _lib.PCBENV_EINVAL
    reward = torch.full((1,), -5.0, dtype=torch.float64, device=env.device)  # no playout: a no-op success that writes nothing
    R = _lib.PcbenvPlayoutRequest
    req = R(struct_size=C.sizeof(R), num_playouts=0, max_steps=3, reward_dev=reward.data_ptr(), stream=env._stream().value)
    assert env._L.pcbenv_playout_paths(env._h, C.byref(req)) == _lib.PCBENV_OK and float(reward[0]) == -5.0
    # buffers not bound; the stream being captured (as tests/test_sample_axis_gpu.py does it: every tensor exists before the capture)
    out = torch.full((8,), -5.0, dtype=torch.float64, device=env.device)

    def call(handle, stream):
        q = R(struct_size=C.sizeof(R), num_playouts=8, max_steps=3, reward_dev=out.data_ptr(), stream=stream)
        return env._L.pcbenv_playout_paths(handle, C.byref(q))
    ccfg = _lib.make_config(cfg, 8)
    h = C.c_void_p()
    _lib.check(env._L.pcbenv_create(C.byref(ccfg), torch.cuda.current_device(), C.byref(h)))
    assert call(h, None) == _lib.PCBENV_ESTATE and "pcbenv_bind_buffers" in env._L.pcbenv_last_error(h).decode()
    env._L.pcbenv_destroy(h)
    assert call(env._h, env._stream().value) == _lib.PCBENV_OK
    torch.cuda.synchronize()
    scratch = torch.zeros(4, device=env.device)
    scratch.add_(1.0)  # loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        scratch.add_(1.0)
        rc = call(env._h, env._stream().value)
        msg = env._L.pcbenv_last_error(env._h).decode()
    assert rc == _lib.PCBENV_ESTATE and "pcbenv_playout_paths cannot be captured" in msg
    assert int(env.playout(k=2, paths=paths[:0]).length.min()) >= 1  # the handle works on
    env.close()


def test_side_stream():
    """One call on a non-blocking side stream behind a delay: it returns before the stream reaches it, and the result
    equals the default-stream result."""
    plan = plan_of("c3_centroid")
    cfg, n = plan.cfg, plan.n
    run = device_roots(plan.roots)
    dev = run.env.device
    paths = torch.from_numpy(plan.path_tensor(fill=-9)).to(dev)
    plen = torch.from_numpy(plan.path_len).to(dev)
    call = lambda: run.env.playout(k=K, step_index=STEP0, paths=paths, path_len=plen, leaf_mask=True, max_steps=plan.limit)
    want = call()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with lagged(side) as before:
        call()  # once without a delay: the wrapper's buffers exist on this stream
        side.synchronize()
        before()
        reached = torch.cuda.Event()
        reached.record(side)
        t0 = time.perf_counter()
        got = call()
        dt = 1e3 * (time.perf_counter() - t0)
        ev = torch.cuda.Event()
        ev.record(side)
        assert not reached.query(), f"pcbenv_playout_paths returned only after the stream had passed a {LAG_MS} ms delay ({dt:.2f} ms on the host)"
        assert not ev.query()
        side.synchronize()
        _same_playout(got, want)
        assert torch.equal(got.leaf_mask, want.leaf_mask)
        check_against(got, plan.expected, cfg)
    run.close()
