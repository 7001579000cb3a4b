"""k_top_priors (pcbenv_top_priors) against the float64 contract of include/pcbenv_priors.h
(tests/top_priors_cases.py:contract, checked on the CPU by tests/test_top_priors_cases.py and against csrc/pcb_topk.h by
tests/test_top_priors_model.py) on the values the kernel read, i.e. the logits after the cast to the test dtype.

cand_count, cand_actions, the padding and the error bits are exact.  A prior is allowed
    4 x e_ref + 4 x ulp32(want)
against the contract: e_ref is the largest error, over the same entries, of torch's float32 chain on the CPU
(masked_logits, then a float32 softmax, gathered at the contract's actions so that it does not depend on torch's sort) --
the convention of tests/test_logits_edges_gpu.py, whose factor 4 is the margin for a float32 chain with another summation
order; 4 ulp because the kernel's Z is a float32 sum per segment.  Bad rows are float32(1.0 / n) exactly.  No bound is
taken from the kernel's output; every case prints e_ref, the kernel's error and the bound (profiles/top_priors.txt).

Kernel-against-kernel comparisons -- dirty against clean bit rows, poisoned illegal logits, an element-aligned pointer, a
second launch, the handle's own bit rows against the same rows passed in, a side stream -- are bit for bit."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import logits_cases as lc
import path_cases as pa
import playout_cases as pc
import top_priors_cases as tc
from pcbenv import _lib, _priors_lib, named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.search import Evaluation, network_evaluator, puct_search, puct_search_device
from stream_cases import lagged
from test_playout_gpu import device_roots
from test_puct_search_gpu import C_PUCT, FIELDS, STEP_INDEX, constant_logits, linear_logits, same

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
NAMES = list(tc.GEOMETRIES) + ["c3"]
SENTINEL = 0x5A5A5A5A
_HANDLES = {}


def _geometry(name):
    cfg = lc.RAGGED[name]() if name in lc.RAGGED else named_config(name)
    return cfg, cfg.num_orientations, cfg.height, cfg.width


def _handle(name):
    """One handle per configuration: the calls with mask_bits take their geometry from it and nothing else."""
    if name not in _HANDLES:
        _HANDLES[name] = BatchedPlacementEnv(_geometry(name)[0], 4, queue_depth=1, run_seed=5)
    return _HANDLES[name]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for env in _HANDLES.values():
        env.close()
    _HANDLES.clear()


def _rows(name):
    """(legal, bit rows): the synthetic classes of the ragged geometries; at c3 (4 x 64 x 64) their first 8 rows."""
    if name in lc.RAGGED:
        legal, bits, _ = tc.synthetic(name)
        return legal, bits
    cfg, O, H, W = _geometry(name)
    clean = np.concatenate([b for _, b, _ in lc.mask_classes(cfg.kind, O, H, W, tc.rng_for("masks", name))])[:8]
    return tc.ec.legal_rows(clean, O, H, W), clean.view(np.int64)


def _logits(name, regime, legal, dtype):
    """(the float32 values the kernel reads, the device tensor in `dtype`)."""
    l = tc.to_dtype(tc.REGIMES[regime](tc.rng_for("logits", name, regime), legal), dtype == torch.bfloat16)
    return l, torch.from_numpy(l).to(dtype)


def _launch(env, x, K, bits=None, errors=True):
    err = torch.zeros(1, dtype=torch.int32, device=env.device) if errors else None
    count, actions, prior = env.top_priors(x, K, mask_bits=bits, errors=err)
    return SimpleNamespace(count=count.cpu().numpy(), actions=actions.cpu().numpy(), prior=prior.cpu().numpy(), errors=int(err.item()) if errors else 0)


def _bytes(got):
    return got.count.tobytes(), got.actions.tobytes(), got.prior.tobytes(), got.errors


def _check(label, l, legal, K, H, W, got):
    count, actions, prior, errors = tc.contract(l, legal, K, H, W)
    assert np.array_equal(got.count, count), label
    assert np.array_equal(got.actions, actions), label  # the padding included
    assert got.errors == errors, label
    kept = np.arange(K)[None, :] < count[:, None]
    assert not got.prior[~kept].any(), label
    n = legal.sum(1)
    bad = np.array([n[r] > 0 and (np.isnan(l[r, legal[r]]).any() or (l[r, legal[r]] == np.inf).any() or (l[r, legal[r]] == -np.inf).all())
                    for r in range(legal.shape[0])])
    want32 = prior.astype(np.float32)
    assert np.array_equal(got.prior[bad], want32[bad]), label  # float32(1.0 / n), exactly
    good = kept & ~bad[:, None]
    chain = tc.chain32_priors(np.where(np.isnan(l), 0.0, l), legal, tc.flat_of(actions, H, W), count)
    e_ref = float(np.abs(chain - prior)[good].max()) if good.any() else 0.0
    bound = 4.0 * e_ref + 4.0 * lc.ulp32(want32)
    err = np.abs(got.prior.astype(np.float64) - prior)
    worst = int(np.argmax(np.where(good, err - bound, -np.inf))) if good.any() else 0
    print(f"TOP-PRIORS {label}: e_ref {e_ref:.3e}, kernel error {float(err[good].max()) if good.any() else 0.0:.3e}, "
          f"bound at the worst entry {float(bound.reshape(-1)[worst]):.3e}")
    assert np.isfinite(e_ref) and (err[good] <= bound[good]).all(), label


# ---- a. against the contract: geometry x regime x K x dtype ---------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("name", NAMES)
def test_against_the_contract(name, dtype):
    cfg, O, H, W = _geometry(name)
    env = _handle(name)
    legal, bits = _rows(name)
    bits_dev = torch.from_numpy(bits).to(env.device)
    vec, nw = lc.launch_path(cfg)
    for regime in tc.REGIMES:
        l, x = _logits(name, regime, legal, dtype)
        x = x.to(env.device)
        for K in tc.KS:
            _check(f"{name} <{'VEC' if vec else 'scalar'},NW{nw}> {regime} K={K} {str(dtype)[6:]}", l, legal, K, H, W, _launch(env, x, K, bits_dev))


@DTYPES
@pytest.mark.parametrize("name", tc.GEOMETRIES)
def test_legal_counts_around_K(name, dtype):
    cfg, O, H, W = _geometry(name)
    env = _handle(name)
    for K in tc.KS:
        legal, bits, targets = tc.counted(name, K)
        bits_dev = torch.from_numpy(bits).to(env.device)
        for regime in ("tame", "constant", "bad_rows"):
            l, x = _logits(name, regime, legal, dtype)
            _check(f"{name} n in {targets} {regime} K={K} {str(dtype)[6:]}", l, legal, K, H, W, _launch(env, x.to(env.device), K, bits_dev))


# ---- b. invariances, bit for bit ------------------------------------------------------------------------------------

def _placed(x, offset):
    """The same values `offset` elements past a 16-byte boundary, C-contiguous, with slack behind the last row."""
    big = torch.zeros(x.numel() + 4 + 256, dtype=x.dtype, device=x.device)
    v = big[offset:offset + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and big.data_ptr() % 16 == 0 and v.data_ptr() % 16 == offset * x.element_size()
    return v


@DTYPES
@pytest.mark.parametrize("name", NAMES)
def test_invariances(name, dtype):
    cfg, O, H, W = _geometry(name)
    env = _handle(name)
    legal, bits = _rows(name)
    rng = tc.rng_for("invariances", name)
    twin = lc.dirty_twin(bits, cfg.kind, W, rng)
    assert np.array_equal(tc.ec.legal_rows(twin.view(np.uint64), O, H, W), legal) and (name == "c3" or not np.array_equal(twin, bits))
    bits_dev, twin_dev = torch.from_numpy(bits).to(env.device), torch.from_numpy(twin).to(env.device)
    for regime in ("tame", "four_values", "bad_rows"):
        l, x = _logits(name, regime, legal, dtype)
        poison = torch.from_numpy(np.where(legal, l, rng.choice(np.array([np.nan, 3e38, -3e38], np.float32), size=l.shape))).to(dtype)
        x, poison = x.to(env.device), poison.to(env.device)
        for K in (3, 64):
            base = _bytes(_launch(env, x, K, bits_dev))
            assert _bytes(_launch(env, x, K, twin_dev)) == base, (name, regime, K, "dirty padding or a dirty plane 1 changed an output")
            assert _bytes(_launch(env, poison, K, bits_dev)) == base, (name, regime, K, "an illegal logit changed an output")
            assert _bytes(_launch(env, _placed(x, 1), K, bits_dev)) == base, (name, regime, K, "an element-aligned pointer changed an output")
            assert _bytes(_launch(env, x, K, bits_dev)) == base, (name, regime, K, "a second launch gave other bits")


# ---- c. emission: every element written, nothing beside them --------------------------------------------------------

@pytest.mark.parametrize("name", ["rect_33x65", "pin_100x9", "square_3x128", "c3"])
@pytest.mark.parametrize("K", [1, 3, 64])
def test_every_output_element_is_written_and_nothing_else(name, K):
    cfg, O, H, W = _geometry(name)
    env = _handle(name)
    legal, bits = _rows(name)
    N = legal.shape[0]
    l, x = _logits(name, "few_finite", legal, torch.float32)
    bufs = [torch.full((N + 2,) + tail, SENTINEL, dtype=torch.int32, device=env.device) for tail in ((), (K, 3), (K,))]
    out = (bufs[0][1:N + 1], bufs[1][1:N + 1], bufs[2].view(torch.float32)[1:N + 1])
    assert all(t.is_contiguous() for t in out)
    env.top_priors(x.to(env.device), K, mask_bits=torch.from_numpy(bits).to(env.device), out=out)
    torch.cuda.synchronize()
    for b in bufs:
        assert (b[0] == SENTINEL).all() and (b[N + 1] == SENTINEL).all(), "a guard row was written"
        assert not (b[1:N + 1] == SENTINEL).any(), "an element of an output was left as it was"
    count, actions, prior, _ = tc.contract(l, legal, K, H, W)
    assert np.array_equal(out[0].cpu().numpy(), count) and np.array_equal(out[1].cpu().numpy(), actions)
    assert (count == 0).any() and (count == K).any()


# ---- d. the handle's own bit rows ------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("name", ["pin_40x48", "small_pin"])
def test_the_handles_current_state_set(name, dtype):
    cfg = lc.RAGGED[name]() if name in lc.RAGGED else pc.case(name)[0]()
    O, H, W = cfg.num_orientations, cfg.height, cfg.width
    B = 24
    env = BatchedPlacementEnv(cfg, B, queue_depth=2, run_seed=3, auto_reset=False)
    env.generate_instances()
    env.reset()
    def advance(t):  # as the episodes of tests/test_sample_logits_gpu.py
        env.step(env.sample_actions(t))
        env.reset_done()
    for t in range(3):
        advance(t)
    for t in (3, 4):  # the current state set alternates from step to step
        l = tc.to_dtype(lc.tame(tc.rng_for("handle", name, t), np.ones((B, O * H * W), bool)), dtype == torch.bfloat16)
        x = torch.from_numpy(l).to(dtype).to(env.device)
        legal = env.action_mask.reshape(B, -1).cpu().numpy() != 0
        assert legal.any(1).sum() > B // 2
        for K in (3, 16):
            own, given = _launch(env, x, K), _launch(env, x, K, env.mask_bits())
            assert _bytes(own) == _bytes(given), (name, t, K)
            _check(f"{name} own rows after {t} steps K={K} {str(dtype)[6:]}", l, legal, K, H, W, own)
        advance(t)
    # without mask_bits the rows are the handle's environments
    with pytest.raises(ValueError):
        env.top_priors(x[:B - 1], 3)
    R = _priors_lib.PcbenvTopPriorsRequest
    outs = env.top_priors(x, 3)

    def call(handle, rows, stream=None):
        q = R(struct_size=C.sizeof(R), logits_dtype=_lib.LOGITS_F32 if dtype == torch.float32 else _lib.LOGITS_BF16, num_candidates=3, num_rows=rows,
              logits=x.data_ptr(), cand_count=outs[0].data_ptr(), cand_actions=outs[1].data_ptr(), cand_prior=outs[2].data_ptr(), stream=stream)
        return env._L.pcbenv_top_priors(handle, C.byref(q))
    assert call(env._h, B - 1) == _lib.PCBENV_EINVAL and "num_rows must be num_envs" in env._L.pcbenv_last_error(env._h).decode()
    assert call(env._h, 0) == _lib.PCBENV_EINVAL
    # buffers not bound (as tests/test_playout_paths_gpu.py does it)
    ccfg = _lib.make_config(cfg, B)
    h = C.c_void_p()
    _lib.check(env._L.pcbenv_create(C.byref(ccfg), torch.cuda.current_device(), C.byref(h)))
    assert call(h, B) == _lib.PCBENV_ESTATE and "pcbenv_bind_buffers" in env._L.pcbenv_last_error(h).decode()
    env._L.pcbenv_destroy(h)
    assert call(env._h, B, env._stream().value) == _lib.PCBENV_OK
    torch.cuda.synchronize()
    env.close()


def test_no_rows_is_a_no_op():
    env = _handle("rect_9x70")
    cfg, O, H, W = _geometry("rect_9x70")
    x = torch.zeros((0, O * H * W), dtype=torch.float32, device=env.device)
    bits = torch.zeros((0, 2, H, (W + 63) // 64), dtype=torch.int64, device=env.device)
    count, actions, prior = env.top_priors(x, 5, mask_bits=bits)
    assert count.shape == (0,) and actions.shape == (0, 5, 3) and prior.shape == (0, 5)
    one = torch.zeros((1, O * H * W), dtype=torch.float32, device=env.device)
    R = _priors_lib.PcbenvTopPriorsRequest
    q = R(struct_size=C.sizeof(R), logits_dtype=_lib.LOGITS_F32, num_candidates=5, num_rows=0, logits=one.data_ptr(), mask_bits=one.data_ptr(),
          cand_count=one.data_ptr(), cand_actions=one.data_ptr(), cand_prior=one.data_ptr())
    assert env._L.pcbenv_top_priors(env._h, C.byref(q)) == _lib.PCBENV_OK and not one.any()
    for bad_K in (0, 65):
        with pytest.raises(Exception):
            env.top_priors(one, bad_K, mask_bits=torch.zeros((1, 2, H, (W + 63) // 64), dtype=torch.int64, device=env.device))


# ---- e. streams -----------------------------------------------------------------------------------------------------

def test_side_stream():
    """On a non-blocking side stream, behind a delay and a copy that makes the logits what they should be: the call returns
    before the stream reaches it, runs where it was put -- on any other stream it would read the logits as they still are --
    and gives the default-stream result."""
    name, K = "pin_40x48", 16
    cfg, O, H, W = _geometry(name)
    env = _handle(name)
    legal, bits = _rows(name)
    bits_dev = torch.from_numpy(bits).to(env.device)
    l, x = _logits(name, "tame", legal, torch.float32)
    right = x.to(env.device)
    want = _bytes(_launch(env, right, K, bits_dev, errors=False))
    staged = torch.zeros_like(right)  # valid but wrong until the side stream has passed the lag
    assert _bytes(_launch(env, staged, K, bits_dev, errors=False)) != want
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with lagged(side) as before:
        env.top_priors(staged, K, mask_bits=bits_dev)  # once without a delay: nothing is created on this stream later
        side.synchronize()
        before()
        reached = torch.cuda.Event()
        reached.record(side)
        staged.copy_(right, non_blocking=True)
        out = env.top_priors(staged, K, mask_bits=bits_dev)
        ev = torch.cuda.Event()
        ev.record(side)
        assert not reached.query() and not ev.query(), "pcbenv_top_priors returned only after the stream had passed the delay"
        side.synchronize()
    got = SimpleNamespace(count=out[0].cpu().numpy(), actions=out[1].cpu().numpy(), prior=out[2].cpu().numpy(), errors=0)
    assert _bytes(got) == want


# ---- f. the whole stack ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("iterations, Cc, logits", [(12, 3, constant_logits), (8, 16, constant_logits), (16, 16, linear_logits)])
def test_the_search_with_device_priors(iterations, Cc, logits):
    roots = pa.Plan("small_pin").roots
    cfg, P, T = roots.cfg, roots.P, pc.max_steps(roots.cfg)
    run = device_roots(roots)
    dev = run.env.device
    planner = BatchedPlacementEnv(cfg, P, queue_depth=2, run_seed=roots.seed, auto_reset=False, **roots.kw)
    planner.generate_instances()
    planner.reset()
    fn = logits(cfg, P, dev)
    evaluate = network_evaluator(run.env, planner, fn, max_children=Cc, priors="device")

    def copied_over(paths, path_len, step_index0):
        ev = evaluate(paths.to(dev), path_len.to(dev), step_index0)
        return Evaluation(*(getattr(ev, f).cpu() for f in ("value", "terminal", "cand_count", "cand_actions", "cand_prior")))
    want = puct_search(SimpleNamespace(num_envs=P, cfg=cfg, device="cpu"), iterations, STEP_INDEX, copied_over, c_puct=C_PUCT, max_children=Cc, max_steps=T)
    got = puct_search_device(run.env, iterations, STEP_INDEX, evaluate, c_puct=C_PUCT, max_children=Cc, max_steps=T)
    assert int(want.errors) == 0 and int(want.num_nodes.max()) > 1 + Cc and int(want.depth.max()) >= 2
    for f in FIELDS:
        assert same(getattr(got, f), getattr(want, f)), f
    again = puct_search_device(run.env, iterations, STEP_INDEX, evaluate, c_puct=C_PUCT, max_children=Cc, max_steps=T)
    for f in FIELDS:
        assert same(getattr(again, f), getattr(got, f)), f  # the same tree twice
    if logits is constant_logits:  # Z = n exactly and float32(1 / n) on both sides: the torch chain's search, bit for bit
        chain = puct_search_device(run.env, iterations, STEP_INDEX, network_evaluator(run.env, planner, fn, max_children=Cc, priors="torch"),
                                   c_puct=C_PUCT, max_children=Cc, max_steps=T)
        for f in FIELDS:
            assert same(getattr(chain, f), getattr(got, f)), f
    else:
        assert len(set(got.child_priors[got.child_priors > 0].cpu().numpy().tolist())) > P  # priors that differ
    with pytest.raises(ValueError):
        network_evaluator(run.env, planner, fn, max_children=Cc, priors="sorted")
    run.compare_oracle("the roots after the searches")
    planner.close()
    run.close()
