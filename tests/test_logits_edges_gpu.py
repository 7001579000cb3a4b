"""k_sample_logits, k_evaluate_logits and k_evaluate_logits_backward where the other logits tests do not go: grids with
H != W and a partial second mask word, every <T, VEC, NW> instantiation, caller-made bit rows (single bits, word 1 only,
plane 1 only, dirty padding), pointers aligned to one element only, and logits that are large, shifted, peaked,
underflowing or so far apart that their difference is no float32.  Configurations, bit rows and regimes come from
tests/logits_cases.py.

The reference is always the float64 restatement of the header (tests/evaluate_contract.py, tests/sampling_contract.py)
on the values the kernel read, i.e. the logits after the cast to the test dtype.  Kernel-against-kernel comparisons
(dirty against clean bit rows, misaligned against aligned pointers, shifted against unshifted logits) come on top and are
exact: both sides run the same arithmetic on the same numbers.

Tolerances.  log_prob and entropy: with `want` the contract value as a float32,
    allowed = 4 x e_ref + ulp32(want) + 1e-6,
e_ref being the error of torch's float32 chain (masked_logits + Categorical, on the CPU, same inputs) against the
contract over the rows where that chain is finite: 4 x for reordered float32 sums and exp2-based weights, one ulp because
the output is a float32, 1e-6 to keep the bound off zero.  The chain is finite on every row of every regime but
huge_spread (asserted); there the rows it loses (the stored action sits on a -3.0e38 logit) are held to 4 float32 ulp of
`want`, +-inf exactly: Z is a count, and the kernels form these outputs in float64 and round once.  The gradient keeps the
rule of tests/test_evaluate_logits_gpu.py: 4 x the chain's gradient error + 1e-7, for bf16 against the rounded contract
plus one bf16 ulp.  The sampler's place on the inverse CDF keeps its 3e-5.  No bound is taken from a kernel's output.

The two huge regimes are held tighter than that rule alone would.  At 3.0e38 the chain's float32 logsumexp absorbs log Z,
so where it is finite it is off by log Z itself (e_ref 7.2 - 11.1 measured on the CPU) and 4 x e_ref bounds nothing.
Every row of huge_equal and huge_spread is therefore held to the 4-ulp rule, and the gradient to the chain's error on
the collapsed twin of the logits (+3.0e38 -> 0, -3.0e38 -> -inf), for which the contract gives the same numbers
(asserted) and the chain is accurate.

Single-bit rows: with O = 4 one bit is two legal actions (orientations o and o + 2 read the same plane), so
log_prob = entropy = 0 and the zero gradient row are asserted where the legal count is 1 (square and rect kinds)."""
import zlib

import numpy as np
import pytest
import torch

import evaluate_contract as ec
import logits_cases as lc
import sampling_contract as sc
from pcbenv import named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.config import KIND_SQUARE
from test_sample_logits_gpu import SEED, _env, _host_dist, _legal

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
SENTINEL = {torch.float32: (torch.int32, 0x5A5A5A5A), torch.bfloat16: (torch.int16, 0x5A5A)}
FIRST = 11  # first_env_index of the environments that draw
_HANDLES = {}


def _cfg(name):
    return lc.RAGGED[name]() if name in lc.RAGGED else named_config(name)


def _tag(name, cfg, aligned=True):
    vec, nw = lc.launch_path(cfg, aligned)
    return f"{name} <{'VEC' if vec else 'scalar'},NW{nw}>"


def _handle(name):
    """One handle per configuration: the evaluate calls take their geometry from it and nothing else."""
    if name not in _HANDLES:
        _HANDLES[name] = BatchedPlacementEnv(_cfg(name), 4, queue_depth=1, run_seed=SEED)
    return _HANDLES[name]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for env in _HANDLES.values():
        env.close()
    _HANDLES.clear()


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _placed(x, offset):
    """The same values `offset` elements past a 16-byte boundary, C-contiguous, with slack behind the last row."""
    big = torch.zeros(x.numel() + 4 + 256, dtype=x.dtype, device=x.device)
    v = big[offset:offset + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and big.data_ptr() % 16 == 0 and v.data_ptr() % 16 == offset * x.element_size()
    return v


def _misaligned(x):
    return _placed(x, 1)


def _guarded(N, A, dtype, device, misaligned):
    """A gradient buffer [N, A] filled with NaN, between one guard row before and one after it."""
    itype, sentinel = SENTINEL[dtype]
    flat = torch.empty((N + 2) * A + 4, dtype=dtype, device=device)
    rows = flat[int(misaligned):int(misaligned) + (N + 2) * A].view(N + 2, A)
    rows.view(itype).fill_(sentinel)
    rows[1:N + 1] = float("nan")
    out = rows[1:N + 1]
    assert out.is_contiguous()
    if misaligned:
        assert out.data_ptr() % out.element_size() == 0 and (out.data_ptr() % 16 != 0 or A % 4 != 0)
    return rows, out


def _actions(a, cfg, fmt, device):
    t = torch.from_numpy(np.asarray(a).astype(np.int32))
    if fmt == "tuple":
        HW, W = cfg.height * cfg.width, cfg.width
        t = torch.stack([t // HW, (t % HW) // W, t % W], 1).to(torch.int32)
    return t.contiguous().to(device)


def _run_eval(env, x, bits, acts, g_lp, g_h, misaligned_grad=False):
    """Forward with stats, then backward into the guarded buffer -> host copies of everything, the guards checked."""
    N, A = x.shape
    itype, sentinel = SENTINEL[x.dtype]
    stats = torch.full((N, 4), float("nan"), dtype=torch.float32, device=x.device)
    err = torch.zeros(1, dtype=torch.int32, device=x.device)
    lp, ent = env.evaluate_logits_forward(x, bits, acts, stats, err)
    rows, out = _guarded(N, A, x.dtype, x.device, misaligned_grad)
    env.evaluate_logits_backward(x, bits, acts, stats, torch.from_numpy(g_lp).float().to(x.device),
                                 torch.from_numpy(g_h).float().to(x.device), out=out)
    guards = rows.view(itype)[[0, N + 1]].cpu().numpy()
    assert (guards == sentinel).all(), "a guard row of the gradient buffer was written"
    return dict(lp=lp.cpu().numpy(), ent=ent.cpu().numpy(), stats=stats.cpu().numpy(), err=int(err.item()),
                g=out.float().cpu().numpy().astype(np.float64), g_raw=out.contiguous().view(itype).cpu().numpy())


def _rows_of(got, sl):
    return {k: (v if k == "err" else v[sl]) for k, v in got.items()}


def _same_bytes(x, y, keys=("lp", "ent", "stats", "g_raw")):
    return all(np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)) for k in keys)


def _bf16_round(x):
    return torch.from_numpy(np.asarray(x, np.float64)).to(torch.bfloat16).double().numpy()


def _bf16_ulp(x):
    ax = np.abs(x)
    return np.where(ax > 0, 2.0 ** (np.floor(np.log2(np.where(ax > 0, ax, 1.0))) - 7), 0.0)


def _forward_errors(got, want, e_ref, loose):
    """-> (error, allowed) per row; loose rows: 4 e_ref + ulp32(want) + 1e-6 against the float64 value; the others 4 ulp
    of the float32 value; +-inf must match exactly (error 0 where it does, inf where not)."""
    with np.errstate(over="ignore"):
        want32 = np.asarray(want, np.float64).astype(np.float32)
    got = np.asarray(got, np.float32)
    inf = np.isinf(want32)
    u = lc.ulp32(want32)
    allowed = np.where(loose, 4.0 * e_ref + u + 1e-6, 4.0 * u)
    with np.errstate(all="ignore"):
        err = np.where(loose, np.abs(got.astype(np.float64) - want), np.abs(got.astype(np.float64) - want32.astype(np.float64)))
        err = np.where(inf, np.where(got == want32, 0.0, np.inf), err)
    return err, np.where(inf, 0.0, allowed)


def _chain_conditions(regime, fin, has):
    """Before any e_ref is used: the chain is finite on every row with a legal action -- in huge_spread on at least a
    quarter of them."""
    if regime == "huge_spread":
        assert 4 * int(fin[has].sum()) >= int(has.sum()) and fin[has].any(), (regime, int(fin[has].sum()), int(has.sum()))
    else:
        assert fin[has].all(), (regime, np.flatnonzero(has & ~fin))


HUGE_REGIMES = ("huge_equal", "huge_spread")


def _collapsed_twin_grad_error(l, legal, a, g_lp, g_h, want_g, has):
    """The float32 chain's gradient error on +HUGE -> 0, -HUGE -> -inf: the same distribution at a tame magnitude."""
    twin = np.where(l > 0, 0.0, -np.inf)
    np.testing.assert_allclose(ec.gradient(twin, legal, a, g_lp, g_h), want_g, atol=1e-12, rtol=0)
    _, _, c_g, fin = lc.chain32(twin, legal, a, g_lp, g_h)
    assert 4 * int((fin & has).sum()) >= int(has.sum())
    return float(np.abs(c_g - want_g)[fin & has].max()) if (fin & has).any() else 0.0


def _check_eval(label, regime, dtype, l, legal, a, g_lp, g_h, got):
    """The outputs of one forward + backward pair against the contract."""
    has = legal.any(1)
    want_lp, want_ent, want_bits, want_status = ec.evaluate(l, legal, a)
    want_g = ec.gradient(l, legal, a, g_lp, g_h)
    assert want_bits == 0 and np.isfinite(want_g).all()
    c_lp, c_ent, c_g, fin = lc.chain32(l, legal, a, g_lp, g_h)
    _chain_conditions(regime, fin, has)
    use = fin & has  # a row without a legal action is 0 by contract and uniform over all A for the chain
    e_lp = float(np.abs(c_lp - want_lp)[use].max()) if use.any() else 0.0
    e_ent = float(np.abs(c_ent - want_ent)[use].max()) if use.any() else 0.0
    e_g = float(np.abs(c_g - want_g)[use].max()) if use.any() else 0.0
    loose = (use | ~has) & (regime not in HUGE_REGIMES)
    err_lp, ok_lp = _forward_errors(got["lp"], want_lp, e_lp, loose)
    err_ent, ok_ent = _forward_errors(got["ent"], want_ent, e_ent, loose)
    if regime in HUGE_REGIMES:
        e_g = min(e_g, _collapsed_twin_grad_error(l, legal, a, g_lp, g_h, want_g, has))
    bound = 4.0 * e_g + 1e-7
    gk = got["g"]
    if dtype == torch.float32:
        want, allow = want_g, bound
    else:
        want = _bf16_round(want_g)
        allow = bound + _bf16_ulp(want)
    with np.errstate(all="ignore"):
        err_g = np.abs(gk - want)
    print(f"EDGE-EVAL {label} {regime} {dtype} rows {len(a)} chain_finite {int(use.sum())}/{int(has.sum())} | log_prob e_ref {e_lp:.3e} "
          f"kernel_err {err_lp.max():.3e} bound {ok_lp.max():.3e} | entropy e_ref {e_ent:.3e} kernel_err {err_ent.max():.3e} "
          f"bound {ok_ent.max():.3e} | grad e_ref {e_g:.3e} kernel_err {err_g.max():.3e} bound {bound:.3e}")
    assert got["err"] == 0, (label, regime, got["err"])
    assert np.array_equal(got["stats"][:, 3], want_status.astype(np.float32)), (label, regime)
    assert (err_lp <= ok_lp).all(), (label, regime, "log_prob", np.flatnonzero(~(err_lp <= ok_lp))[:8], got["lp"][~(err_lp <= ok_lp)][:8])
    assert (err_ent <= ok_ent).all(), (label, regime, "entropy", np.flatnonzero(~(err_ent <= ok_ent))[:8], got["ent"][~(err_ent <= ok_ent)][:8])
    assert np.array_equal(got["stats"][:, 2].view(np.uint32), got["ent"].view(np.uint32)), (label, regime)
    assert not got["lp"][~has].any() and not got["ent"][~has].any()
    # structural, exact: written and finite everywhere, zero off the legal set and in rows without one
    assert np.isfinite(gk).all(), (label, regime, "gradient not finite", int((~np.isfinite(gk)).sum()))
    assert not gk[~legal].any(), (label, regime)
    assert not gk[~has].any(), (label, regime)
    assert (err_g <= allow).all(), (label, regime, "gradient", float(err_g.max()), bound)


def _eval_case(label, regime, env, cfg, dtype, rng, l32, legal, bits, fmt, misaligned=(False, False), twins=1):
    """Cast, run and check one case; twins = 2: `bits` holds the rows twice (clean, then dirty) and so do all inputs.
    -> (the outputs of the first copy, of the second or None)."""
    n = legal.shape[0]
    x1 = torch.from_numpy(l32).to(env.device).to(dtype)
    l = x1.float().cpu().numpy().astype(np.float64)  # what the kernels read
    a = lc.stored_actions(rng, legal, l, peak_rows=regime.startswith("peaked"))
    g_lp, g_h = rng.randn(n), 0.01 * rng.randn(n)
    x = torch.cat([x1] * twins).contiguous()
    x = _placed(x, int(misaligned[0]))
    got = _run_eval(env, x, bits, _actions(np.tile(a, twins), cfg, fmt, env.device), np.tile(g_lp, twins), np.tile(g_h, twins),
                    misaligned_grad=misaligned[1])
    first = _rows_of(got, slice(0, n))
    _check_eval(label, regime, dtype, l, legal, a, g_lp, g_h, first)
    return first, (_rows_of(got, slice(n, 2 * n)) if twins == 2 else None)


def _synthetic(cfg, rng, dirty=False):
    """-> (legal bool [n, A], int64 bit rows as numpy (the clean rows, then their dirty twins if asked), the classes)."""
    O, H, W = cfg.num_orientations, cfg.height, cfg.width
    classes = lc.mask_classes(cfg.kind, O, H, W, rng)
    clean = np.concatenate([b for _, b, _ in classes])
    legal = ec.legal_rows(clean, O, H, W)
    assert np.array_equal(legal.sum(1), np.concatenate([c for _, _, c in classes]))
    rows = clean.view(np.int64)
    if dirty:
        twin = lc.dirty_twin(clean, cfg.kind, W, rng)
        assert np.array_equal(ec.legal_rows(twin, O, H, W), legal)
        rows = np.concatenate([rows, twin])
    return legal, rows, classes


# ---- a. evaluate, forward and backward: ragged geometry x synthetic masks -------------------------------------------

@DTYPES
@pytest.mark.parametrize("name", list(lc.RAGGED) + ["c3", "c5"])
def test_evaluate_on_ragged_grids_and_synthetic_masks(name, dtype):
    cfg, env = _cfg(name), _handle(name)
    rng = _rng("a", name, str(dtype))
    legal, rows, classes = _synthetic(cfg, rng, dirty=True)
    bits = torch.from_numpy(rows).to(env.device)
    single = legal.sum(1) == 1
    assert single.any() or cfg.num_orientations == 4
    for fmt in ("flat", "tuple"):
        clean, dirty = _eval_case(f"{_tag(name, cfg)} synthetic {fmt}", "tame", env, cfg, dtype, rng, lc.tame(rng, legal), legal,
                                  bits, fmt, twins=2)
        assert _same_bytes(clean, dirty), (name, fmt, "dirty padding or a dirty plane 1 changed an output")
        assert not clean["lp"][single].any() and not clean["ent"][single].any() and not clean["g"][single].any()


# ---- b. element-aligned pointers -----------------------------------------------------------------------------------

def _draw(env, dev, t, greedy):
    a, lp, ent = env.sample_logits(dev, t, greedy=greedy, flat=True, check=True)  # check: no error bit
    return a.cpu().numpy().astype(np.int64), lp.cpu().numpy(), ent.cpu().numpy()


def _check_draw(label, regime, dtype, l, legal, t, greedy, got):
    """One pcbenv_sample_logits call against the contract: legal, on the inverse CDF of the float64 weights (never on a
    weight of 0) or the lowest-index argmax, log_prob and entropy under the forward rule."""
    fa, lp, ent = got
    B = legal.shape[0]
    has = legal.any(1)
    assert legal[has, fa[has]].all() and (fa[~has] == 0).all(), (label, regime, greedy)
    M, Z, C, _ = _host_dist(l, legal)
    for e in np.flatnonzero(has):
        if greedy:
            assert fa[e] == sc.greedy(l[e], legal[e]), (label, regime, e)
        else:
            u = sc.u_of(SEED, FIRST + e, t)
            lo = C[e, fa[e] - 1] if fa[e] > 0 else 0.0
            assert lo - 3e-5 <= u <= C[e, fa[e]] + 3e-5, (label, regime, e, lo, u, C[e, fa[e]])
            assert np.exp(l[e, fa[e]] - M[e]) > 0, (label, regime, e, "drew an action whose weight is 0")
    zero = np.zeros(B)
    want_lp, want_ent, want_bits, _ = ec.evaluate(l, legal, fa)
    assert want_bits == 0
    c_lp, c_ent, _, fin = lc.chain32(l, legal, fa, zero, zero)
    _chain_conditions(regime, fin, has)
    use = fin & has
    e_lp = float(np.abs(c_lp - want_lp)[use].max()) if use.any() else 0.0
    e_ent = float(np.abs(c_ent - want_ent)[use].max()) if use.any() else 0.0
    loose = (use | ~has) & (regime not in HUGE_REGIMES)
    err_lp, ok_lp = _forward_errors(lp, want_lp, e_lp, loose)
    err_ent, ok_ent = _forward_errors(ent, want_ent, e_ent, loose)
    print(f"EDGE-DRAW {label} {regime} {dtype} {'greedy' if greedy else 'sample'} | log_prob e_ref {e_lp:.3e} kernel_err {err_lp.max():.3e} "
          f"bound {ok_lp.max():.3e} | entropy e_ref {e_ent:.3e} kernel_err {err_ent.max():.3e} bound {ok_ent.max():.3e}")
    assert (err_lp <= ok_lp).all(), (label, regime, greedy, "log_prob", np.flatnonzero(~(err_lp <= ok_lp))[:8])
    assert (err_ent <= ok_ent).all(), (label, regime, greedy, "entropy", np.flatnonzero(~(err_ent <= ok_ent))[:8])
    assert not lp[~has].any() and not ent[~has].any()


def _stepped(name, B, upto):
    env = _env(_cfg(name), B, first_env_index=FIRST)
    for t in range(upto):
        env.step(env.sample_actions(t))
        env.reset_done()
    return env


def _midway(cfg):
    return (cfg.max_num_components if cfg.kind != KIND_SQUARE else 6) // 2


@DTYPES
@pytest.mark.parametrize("name", ["c3", "spatial_7x100", "rect_20x68"])
def test_element_aligned_pointers(name, dtype):
    """Logits and gradient one element past a 16-byte boundary: the header allows it, select_launch then takes one load
    and one store per element (<VEC false>; c3: with four wavefronts).  Against the contract as everywhere, and bit for bit
    what the aligned call gives: the two paths differ in how they load and store, not in what they compute."""
    cfg, env = _cfg(name), _handle(name)
    assert lc.launch_path(cfg)[0] and not lc.launch_path(cfg, aligned=False)[0]
    legal, rows, _ = _synthetic(cfg, _rng("b", name))
    bits = torch.from_numpy(rows).to(env.device)
    outs = {}
    for mis in ((False, False), (True, False), (False, True), (True, True)):
        rng = _rng("b", name, str(dtype))  # the same logits, actions and gradients in all four
        label = f"{_tag(name, cfg, not any(mis))} logits{'+1' if mis[0] else ''} grad{'+1' if mis[1] else ''}"
        outs[mis], _ = _eval_case(label, "tame", env, cfg, dtype, rng, lc.tame(rng, legal), legal, bits, "flat", misaligned=mis)
        assert _same_bytes(outs[mis], outs[(False, False)]), (name, dtype, mis)

    drawer = _stepped(name, 32, _midway(cfg))
    legal = _legal(drawer)
    rng = _rng("b-draw", name, str(dtype))
    dev = torch.from_numpy(lc.tame(rng, legal)).to(drawer.device).to(dtype)
    l = dev.float().cpu().numpy().astype(np.float64)
    for greedy in (False, True):
        want = _draw(drawer, dev, 3, greedy)
        got = _draw(drawer, _misaligned(dev), 3, greedy)
        _check_draw(f"{_tag(name, cfg, False)} logits+1", "tame", dtype, l, legal, 3, greedy, got)
        for x, y in zip(got, want):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (name, dtype, greedy)
    drawer.close()


# ---- c. logit regimes ----------------------------------------------------------------------------------------------

def _shift_invariance(label, base, shifted, shift):
    """Outputs of the offset regime's two tensors: every l - M is the same float, so everything but M is the same bits."""
    ok = base["stats"][:, 3] != ec.ROW_ZERO
    assert np.array_equal(base["stats"][:, 3], shifted["stats"][:, 3])
    assert _same_bytes(base, shifted, keys=("lp", "ent", "g_raw")), label
    assert np.array_equal(base["stats"][:, 1:].view(np.uint32), shifted["stats"][:, 1:].view(np.uint32)), label
    assert np.array_equal(shifted["stats"][ok, 0].astype(np.float64) - base["stats"][ok, 0].astype(np.float64), np.full(int(ok.sum()), shift)), label
    assert not base["stats"][~ok, 0].any() and not shifted["stats"][~ok, 0].any()


def _regimes_evaluate(label, env, cfg, dtype, rng, legal, bits, fmts=("flat", "tuple")):
    for k, (regime, make) in enumerate(lc.REGIMES.items()):
        _eval_case(label, regime, env, cfg, dtype, rng, make(rng, legal), legal, bits, fmts[k % len(fmts)])
    base, shifted, shift = lc.offset_pair(rng, legal, dtype == torch.bfloat16)
    state = rng.get_state()
    out0, _ = _eval_case(label, "offset", env, cfg, dtype, rng, base, legal, bits, "flat")
    rng.set_state(state)  # the same stored actions and gradients
    out1, _ = _eval_case(label, "offset+shift", env, cfg, dtype, rng, shifted, legal, bits, "flat")
    _shift_invariance(label, out0, out1, shift)


@DTYPES
@pytest.mark.parametrize("name", ["c3", "c5", "spatial_7x100"])
def test_regimes_on_synthetic_masks(name, dtype):
    """Evaluate, forward and backward, in every regime over the synthetic bit rows (near_uniform over the fully legal row:
    n = A, 65 536 at c5)."""
    cfg, env = _cfg(name), _handle(name)
    rng = _rng("c-syn", name, str(dtype))
    legal, rows, _ = _synthetic(cfg, rng)
    assert (legal.sum(1) == legal.shape[1]).any()
    _regimes_evaluate(f"{_tag(name, cfg)} synthetic", env, cfg, dtype, rng, legal, torch.from_numpy(rows).to(env.device))


@DTYPES
@pytest.mark.parametrize("name", ["c3", "c5", "spatial_7x100"])
def test_regimes_on_real_masks(name, dtype):
    """All three kernels in every regime on the masks of real episodes, right after reset and midway."""
    cfg = _cfg(name)
    B = 16 if name == "c5" else 32
    env = _env(cfg, B, first_env_index=FIRST)
    rng = _rng("c-real", name, str(dtype))
    done = 0
    for pname, at in (("reset", 0), ("midway", _midway(cfg))):
        while done < at:
            env.step(env.sample_actions(done))
            env.reset_done()
            done += 1
        legal = _legal(env)
        bits = env.mask_bits().clone()
        assert np.array_equal(ec.legal_rows(bits.cpu().numpy(), cfg.num_orientations, cfg.height, cfg.width), legal)
        label = f"{_tag(name, cfg)} {pname}"
        _regimes_evaluate(label, env, cfg, dtype, rng, legal, bits, fmts=("tuple", "flat"))
        t = done + 100
        for regime, make in lc.REGIMES.items():
            dev = torch.from_numpy(make(rng, legal)).to(env.device).to(dtype)
            l = dev.float().cpu().numpy().astype(np.float64)
            for greedy in (False, True):
                _check_draw(label, regime, dtype, l, legal, t, greedy, _draw(env, dev, t, greedy))
        base, shifted, shift = lc.offset_pair(rng, legal, dtype == torch.bfloat16)
        for greedy in (False, True):
            d0 = _draw(env, torch.from_numpy(base).to(env.device).to(dtype), t, greedy)
            d1 = _draw(env, torch.from_numpy(shifted).to(env.device).to(dtype), t, greedy)
            _check_draw(label, "offset", dtype, base.astype(np.float64), legal, t, greedy, d0)
            for x, y in zip(d0, d1):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (label, "shift", greedy)
    env.close()

