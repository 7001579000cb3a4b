"""pcbenv_evaluate_visits / pcbenv_evaluate_visits_backward on the GPU: the cross entropy of the masked categorical
against a visit target, the entropy and their gradient, against the float64 restatement of the contract
(tests/visits_contract.py) at the shapes where the launch changes, on caller-made bit rows (tests/logits_cases.py), so
that no episode has to be played; against pcbenv_evaluate_logits, which it must equal with one target; and its edge rows,
guards, streams and argument checks.

Tolerances.  cross_entropy and entropy: the family's atol = 1e-4 against the contract (the cross entropy is a convex
combination of -log_prob values, each of which tests/test_evaluate_logits_gpu.py bounds at 1e-4); +inf, where a target
sits on a legal -inf logit, must match exactly.  The gradient keeps the rule of tests/test_evaluate_logits_gpu.py
unchanged: the kernel may err 4 x what torch's float32 chain on the CPU (pcbenv/visit_targets.py:cross_entropy_torch with
autograd, same inputs) errs against the float64 contract, plus 1e-7; bf16 against the rounded contract plus one bf16 ulp.
Every case prints the chain's error, the kernel's and the bound.  No bound is taken from a kernel's output."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import evaluate_contract as ec
import logits_cases as lc
import visits_cases as vc
import visits_contract as vt
from pcbenv import EnvConfig, _lib, _train_lib
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.visit_targets import cross_entropy, cross_entropy_torch
from stream_cases import lagged
from test_evaluate_logits_gpu import _close_with_inf
from test_logits_edges_gpu import SENTINEL, _bf16_round, _bf16_ulp, _guarded, _placed

pytestmark = pytest.mark.gpu

SHAPES = {"square_3x128": lc.RAGGED["square_3x128"], "rect_9x70": lc.RAGGED["rect_9x70"], "rect_33x65": lc.RAGGED["rect_33x65"],
          "pin_40x48": lc.RAGGED["pin_40x48"],
          "spatial_10x10": lambda: EnvConfig.spatial(10, 10, 9, 9, 2, 2, 2, 2, 5, 5, 3, 3, 6, 6, "centroid", 2, 0.75)}
# (O, VEC with aligned pointers, NW): what each shape is there for
PATHS = {"square_3x128": (1, True, 1), "rect_9x70": (2, False, 1), "rect_33x65": (2, False, 4), "pin_40x48": (4, True, 4),
         "spatial_10x10": (4, False, 1)}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
ROWS = 8
_HANDLES = {}


def _handle(name):
    """One handle per shape: the calls take geometry and device from it and nothing else."""
    if name not in _HANDLES:
        _HANDLES[name] = BatchedPlacementEnv(SHAPES[name](), 4, queue_depth=1, run_seed=7)
    return _HANDLES[name]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for env in _HANDLES.values():
        env.close()
    _HANDLES.clear()


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _geom(cfg):
    return cfg.num_orientations, cfg.height, cfg.width, cfg.num_orientations * cfg.height * cfg.width


def _rows(cfg, rng, N=ROWS):
    """N caller-made bit rows with a legal action each, of as many classes of tests/logits_cases.py as N allows (single
    bits, word 1 only, plane 1 only, full, three densities) -> (bits int64 [N, 2, H, WW], legal bool [N, A])."""
    O, H, W, _ = _geom(cfg)
    rows = []
    for _, clean, count in lc.mask_classes(cfg.kind, O, H, W, rng):
        rows += [clean[i] for i in range(len(clean)) if count[i] > 0][:1]
    classes = np.stack(rows).view(np.int64)
    pick = np.arange(N) % len(classes)
    bits = np.ascontiguousarray(classes[pick])
    return bits, ec.legal_rows(bits, O, H, W)


def _draw(rng, legal, l, C_):
    """Targets drawn from the legal logits that are finite; the last row, where it has one, puts its first entry on a
    legal -inf logit: that row's cross entropy is +inf."""
    visits, idx = vc.draw_targets(rng, legal & np.isfinite(l), C_)
    dead = np.flatnonzero(legal[-1] & np.isneginf(l[-1]))
    if dead.size:
        idx[-1, 0], visits[-1, 0] = dead[0], max(1, visits[-1, 0])
    return visits, idx


def _up(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t if dtype is None else t.to(dtype)


def _chain32(cfg, l, bits, visits, actions, g_ce, g_h):
    """torch's float32 chain on the CPU with autograd -> its gradient as float64."""
    x = torch.tensor(l, dtype=torch.float32, requires_grad=True)
    ce, ent = cross_entropy_torch(cfg, x, torch.from_numpy(bits), torch.from_numpy(visits), torch.from_numpy(actions))
    # (a target on a legal -inf logit makes ce +inf; its gradient is still -pi at that logit, and the chain gives it)
    (ce * torch.from_numpy(np.asarray(g_ce)).float() + ent * torch.from_numpy(np.asarray(g_h)).float()).sum().backward()
    return x.grad.double().numpy()


def _run(env, x, bits, visits, acts, g_ce, g_h, misaligned_grad=False, errors=True, use_stats=True):
    """Forward into guarded outputs and stats, then backward into the guarded NaN-filled buffer -> host copies, the guards
    checked."""
    N, A = x.shape
    dev = x.device
    itype, sentinel = SENTINEL[x.dtype]
    guard = torch.full((3, N + 2), -7.25, dtype=torch.float32, device=dev)
    stats_all = torch.full((N + 2, 4), -7.25, dtype=torch.float32, device=dev)
    ce, ent, stats = guard[0, 1:N + 1], guard[1, 1:N + 1], stats_all[1:N + 1]
    err = torch.zeros(1, dtype=torch.int32, device=dev) if errors else None
    env.evaluate_visits_forward(x, bits, visits, acts, stats if use_stats else None, err, out=(ce, ent))
    assert bool((guard[:2, [0, N + 1]] == -7.25).all()) and bool((guard[2] == -7.25).all()), "an output guard was written"
    assert bool((stats_all[[0, N + 1]] == -7.25).all()), "a guard row of stats was written"
    if not use_stats:
        assert bool((stats == -7.25).all())
        return dict(ce=ce.cpu().numpy(), ent=ent.cpu().numpy())
    rows, out = _guarded(N, A, x.dtype, dev, misaligned_grad)
    env.evaluate_visits_backward(x, bits, visits, acts, stats, None if g_ce is None else _up(np.asarray(g_ce, np.float32), dev),
                                 None if g_h is None else _up(np.asarray(g_h, np.float32), dev), out=out)
    assert (rows.view(itype)[[0, N + 1]].cpu().numpy() == sentinel).all(), "a guard row of the gradient buffer was written"
    return dict(ce=ce.cpu().numpy(), ent=ent.cpu().numpy(), stats=stats.cpu().numpy(), err=int(err.item()) if errors else None,
                g=out.float().cpu().numpy().astype(np.float64), g_raw=out.contiguous().view(itype).cpu().numpy())


def _same_bytes(a, b, keys=("ce", "ent", "stats", "g_raw")):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in keys)


def _gradient_bound(cfg, tag, l, bits, legal, visits, actions, fi, in_range, g_ce, g_h, gk, dtype):
    """Asserts the kernel's gradient gk against the contract under the rule of the module docstring; returns the
    elementwise allowance."""
    want_g = vt.gradient(l, legal, visits, fi, in_range, g_ce, g_h)
    ref = _chain32(cfg, l, bits, visits, actions, np.zeros(len(l)) if g_ce is None else g_ce, np.zeros(len(l)) if g_h is None else g_h)
    has = legal.any(1)
    assert np.isfinite(ref[has]).all()
    e_ref = float(np.abs(ref - want_g)[has].max()) if has.any() else 0.0
    bound = 4.0 * e_ref + 1e-7
    want = want_g if dtype == torch.float32 else _bf16_round(want_g)
    allow = np.full_like(want, bound) if dtype == torch.float32 else bound + _bf16_ulp(want)
    e_k = float(np.abs(gk - want).max())
    print(f"VISITS-GRAD {tag} |g|max {np.abs(want_g).max():.3f} ref_f32_chain_err {e_ref:.3e} kernel_err {e_k:.3e} bound {bound:.3e}")
    assert (np.abs(gk - want) <= allow).all(), (tag, e_k, bound)
    return allow


@DTYPES
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_and_backward_against_the_contract(name, dtype):
    env = _handle(name)
    cfg, dev = env.cfg, env.device
    O, H, W, A = _geom(cfg)
    assert (O,) + lc.launch_path(cfg) == PATHS[name]
    rng = _rng(name, str(dtype))
    bits, legal = _rows(cfg, rng)
    tb = _up(bits, dev)
    x = _up(lc.tame(rng, legal), dev, dtype)
    l = x.float().cpu().numpy().astype(np.float64)  # what the kernels read
    for C_ in (1, 16, 64):
        visits, idx = _draw(rng, legal, l, C_)
        for k, fmt in enumerate(("flat", "tuple")):
            misaligned = bool(k & 1) if C_ == 1 else None  # C = 16 and 64: both placements
            for mis in ((False, True) if misaligned is None else (misaligned,)):
                tag = f"{name} {dtype} C={C_} {fmt} {'misaligned' if mis else 'aligned'}"
                actions = vc.as_actions(idx, H, W, fmt)
                fi, in_range = vt.flat_targets(actions, O, H, W)
                g_ce, g_h = rng.randn(ROWS), 0.01 * rng.randn(ROWS)
                want_ce, want_ent, want_bits, want_status = vt.evaluate(l, legal, visits, fi, in_range)
                assert want_bits == 0 and (want_status == vt.ROW_OK).all()
                xs = _placed(x, 1) if mis else x
                got = _run(env, xs, tb, _up(visits, dev), _up(actions, dev), g_ce, g_h, misaligned_grad=mis)
                assert got["err"] == 0
                assert np.array_equal(got["stats"][:, 3], want_status.astype(np.float32))
                fin = np.isfinite(want_ce)
                print(f"VISITS-FWD {tag} max|dce| {np.abs(got['ce'][fin] - want_ce[fin]).max() if fin.any() else 0.0:.3e} "
                      f"max|dent| {np.abs(got['ent'] - want_ent).max():.3e} inf rows {int((~fin).sum())}")
                _close_with_inf(got["ce"], want_ce, 1e-4)
                np.testing.assert_allclose(got["ent"], want_ent, atol=1e-4, rtol=0)
                # structural, exact: every element written, zero off the legal set
                assert np.isfinite(got["g"]).all()
                assert not got["g"][~legal].any()
                _gradient_bound(cfg, tag, l, bits, legal, visits, actions, fi, in_range, g_ce, g_h, got["g"], dtype)
                # g_H = 0: the rows of the gradient of a loss on the simplex sum to 0
                got0 = _run(env, xs, tb, _up(visits, dev), _up(actions, dev), g_ce, None, misaligned_grad=mis)
                allow = _gradient_bound(cfg, tag + " g_H=0", l, bits, legal, visits, actions, fi, in_range, g_ce, None, got0["g"], dtype)
                assert (np.abs(got0["g"].sum(1)) <= (allow * legal).sum(1)).all(), tag
                if mis:  # the placement changes the arm, not the arithmetic
                    aligned = _run(env, x, tb, _up(visits, dev), _up(actions, dev), g_ce, g_h)
                    assert _same_bytes(got, aligned), tag


@DTYPES
@pytest.mark.parametrize("name", list(SHAPES))
def test_one_target_is_evaluate_logits(name, dtype):
    """C = 1, visits = [1]: cross_entropy == -log_prob of pcbenv_evaluate_logits and the gradient with g_ce = -g_lp, each
    within one ulp of the output's format (float64 sums written in another order; one subtraction may differ)."""
    env = _handle(name)
    cfg, dev = env.cfg, env.device
    O, H, W, A = _geom(cfg)
    rng = _rng("one", name, str(dtype))
    bits, legal = _rows(cfg, rng)
    tb = _up(bits, dev)
    l32 = lc.tame(rng, legal)
    x = _up(l32, dev, dtype)
    a = lc.stored_actions(rng, legal, x.float().cpu().numpy())
    g_lp, g_h = rng.randn(ROWS).astype(np.float32), (0.01 * rng.randn(ROWS)).astype(np.float32)
    for fmt in ("flat", "tuple"):
        acts1 = vc.as_actions(a[:, None], H, W, fmt)                      # [N, 1] / [N, 1, 3]
        stored = _up(acts1[:, 0], dev)                                     # [N] / [N, 3]
        stats = torch.empty((ROWS, 4), dtype=torch.float32, device=dev)
        lp, ent = env.evaluate_logits_forward(x, tb, stored, stats)
        g_eval = env.evaluate_logits_backward(x, tb, stored, stats, _up(g_lp, dev), _up(g_h, dev))
        got = _run(env, x, tb, _up(np.ones((ROWS, 1), np.int32), dev), _up(acts1, dev), -g_lp, g_h)
        ce, want = got["ce"].astype(np.float64), -lp.cpu().numpy().astype(np.float64)
        assert np.isfinite(want).all()
        assert (np.abs(ce - want) <= lc.ulp32(want)).all(), (name, fmt, np.abs(ce - want).max())
        assert np.array_equal(got["ent"], ent.cpu().numpy())
        assert np.array_equal(got["stats"], stats.cpu().numpy())  # ROW_OK is 0 in both
        ge = g_eval.float().cpu().numpy().astype(np.float64)
        ulp = lc.ulp32(ge) if dtype == torch.float32 else _bf16_ulp(ge)
        assert (np.abs(got["g"] - ge) <= ulp).all(), (name, fmt, np.abs(got["g"] - ge).max())


@DTYPES
@pytest.mark.parametrize("name", list(SHAPES))
def test_constant_logits_give_log_n(name, dtype):
    """Constant logits, any targets: Z is the legal count exactly, so cross_entropy == entropy == float32(log n)."""
    env = _handle(name)
    cfg, dev = env.cfg, env.device
    O, H, W, A = _geom(cfg)
    rng = _rng("const", name)
    bits, legal = _rows(cfg, rng)
    visits, idx = vc.draw_targets(rng, legal, 16)
    want = np.log(legal.sum(1).astype(np.float64)).astype(np.float32)
    for value in (0.0, 3.25):
        x = torch.full((ROWS, A), value, dtype=dtype, device=dev)
        got = _run(env, x, _up(bits, dev), _up(visits, dev), _up(vc.as_actions(idx, H, W, "tuple"), dev), None, None)
        assert np.array_equal(got["ce"], want) and np.array_equal(got["ent"], want), (name, value)
        assert not got["g"].any()  # NULL gradients mean zero


def _edge_inputs(cfg, rng, C_=5):
    O, H, W, A = _geom(cfg)
    N = len(vc.EDGE_ROWS)
    cells, legal = vc.planes_legal(rng, O, H, W, N)
    legal, l, visits, idx = vc.edge_batch(rng, legal, lc.tame(rng, legal, p_neg_inf=0.0), C_, A)
    cells[vc.EDGE_ROWS.index("no_legal")] = False
    bits = lc._pack(cells).view(np.int64)
    assert np.array_equal(ec.legal_rows(bits, O, H, W), legal)
    return bits, legal, l, visits, idx


@DTYPES
@pytest.mark.parametrize("fmt", ["flat", "tuple"])
def test_edge_rows_are_data(fmt, dtype):
    """One batch holds every row of the header's table: outputs, bits, row status and gradient rows; then NULL errors_dev,
    NULL stats, NULL gradients and NULL outputs."""
    name = "spatial_10x10"
    env = _handle(name)
    cfg, dev = env.cfg, env.device
    O, H, W, A = _geom(cfg)
    rng = _rng("edge", fmt)
    bits, legal, l32, visits, idx = _edge_inputs(cfg, rng)
    N, row = len(vc.EDGE_ROWS), {n: i for i, n in enumerate(vc.EDGE_ROWS)}
    x = _up(l32, dev, dtype)
    l = x.float().cpu().numpy().astype(np.float64)
    actions = vc.as_actions(idx, H, W, fmt)
    fi, in_range = vt.flat_targets(actions, O, H, W)
    g_ce, g_h = rng.randn(N), 0.01 * rng.randn(N)
    want_ce, want_ent, want_bits, want_status = vt.evaluate(l, legal, visits, fi, in_range)
    assert want_bits == 7
    tb, tv, ta = _up(bits, dev), _up(visits, dev), _up(actions, dev)
    got = _run(env, x, tb, tv, ta, g_ce, g_h)
    assert got["err"] == 7
    assert np.array_equal(got["stats"][:, 3], want_status.astype(np.float32))
    _close_with_inf(got["ce"], want_ce, 1e-4)
    np.testing.assert_allclose(got["ent"], want_ent, atol=1e-4, rtol=0)
    n = legal.sum(1)
    assert got["ce"][row["no_legal"]] == 0 and got["ent"][row["no_legal"]] == 0
    for r in (row["nan"], row["pos_inf"], row["all_neg_inf"]):
        assert got["ce"][r] == got["ent"][r] == np.float32(np.log(n[r]))
    assert got["ce"][row["no_target"]] == 0 and got["ce"][row["target_on_neg_inf"]] == np.inf
    assert np.isfinite(got["g"]).all() and not got["g"][~legal].any()
    for r in (row["no_legal"], row["nan"], row["pos_inf"], row["all_neg_inf"]):
        assert not got["g"][r].any() and got["stats"][r, 3] == vt.ROW_ZERO
    # the rows that are distributions, against the contract (the chain has nothing to say about the others)
    ok = np.flatnonzero(want_status != vt.ROW_ZERO)
    _gradient_bound(cfg, f"edge {fmt} {dtype}", l[ok], bits[ok], legal[ok], visits[ok], actions[ok], fi[ok], in_range[ok], g_ce[ok], g_h[ok],
                    got["g"][ok], dtype)
    # T == 0: the g_ce term is dropped -- the row of the entropy's gradient alone
    only_h = _run(env, x, tb, tv, ta, None, g_h)
    assert np.array_equal(only_h["g_raw"][row["no_target"]], got["g_raw"][row["no_target"]])
    # the error bits of each kind of row, alone
    for names, want in ((("plain", "zero_visits_entry", "no_target", "duplicates", "target_on_neg_inf", "no_legal"), 0),
                        (("negative_visits",), 4), (("illegal_action",), 4), (("out_of_range",), 4), (("nan",), 1), (("pos_inf",), 1), (("all_neg_inf",), 2)):
        rows = [row[k] for k in names]
        part = _run(env, x[rows].contiguous(), tb[rows].contiguous(), tv[rows].contiguous(), ta[rows].contiguous(), g_ce[rows], g_h[rows])
        assert part["err"] == want, names
        assert _same_bytes(part, {k: got[k][rows] for k in ("ce", "ent", "stats", "g_raw")}), names  # rows are independent
    # NULL errors_dev, NULL stats (no gradient wanted)
    quiet = _run(env, x, tb, tv, ta, g_ce, g_h, errors=False)
    assert _same_bytes(quiet, got)
    no_stats = _run(env, x, tb, tv, ta, None, None, use_stats=False)
    assert np.array_equal(no_stats["ce"].view(np.uint32), got["ce"].view(np.uint32)) and np.array_equal(no_stats["ent"].view(np.uint32), got["ent"].view(np.uint32))
    # NULL gradients: a zero gradient, every element written
    none = _run(env, x, tb, tv, ta, None, None)
    assert not none["g"].any()
    zeros = _run(env, x, tb, tv, ta, np.zeros(N), np.zeros(N))
    only_ce, ce_zero_h = _run(env, x, tb, tv, ta, g_ce, None), _run(env, x, tb, tv, ta, g_ce, np.zeros(N))
    assert np.array_equal(only_ce["g_raw"], ce_zero_h["g_raw"]) and not zeros["g"].any()
    # NULL outputs: the call goes through, stats and the bits are as before
    R = _train_lib.PcbenvVisitsRequest
    stats = torch.full((N, 4), -7.25, dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    req = R(struct_size=C.sizeof(R), logits_dtype=_lib.LOGITS_F32 if dtype == torch.float32 else _lib.LOGITS_BF16,
            action_format=_lib.ACTION_FLAT if fmt == "flat" else _lib.ACTION_TUPLE, num_targets=visits.shape[1], num_rows=N,
            logits=x.data_ptr(), mask_bits=tb.data_ptr(), visits=tv.data_ptr(), target_actions=ta.data_ptr(), stats=stats.data_ptr(),
            errors_dev=err.data_ptr(), stream=env._stream().value)
    _lib.check(env._L.pcbenv_evaluate_visits(env._h, C.byref(req)), env._h)
    assert int(err.item()) == 7 and np.array_equal(stats.cpu().numpy().view(np.uint32), got["stats"].view(np.uint32))


@DTYPES
def test_num_rows_is_arbitrary_and_rows_may_be_permuted(dtype):
    """0, 1 and 257 rows (more rows than one XCD's share of workgroups; the last block of xcd_contiguous_env is ragged);
    permuting the rows permutes every output exactly."""
    name = "rect_9x70"
    env = _handle(name)
    cfg, dev = env.cfg, env.device
    O, H, W, A = _geom(cfg)
    rng = _rng("rows", str(dtype))
    N, C_ = 257, 16
    bits, legal = _rows(cfg, rng, N)
    x = _up(lc.tame(rng, legal), dev, dtype)
    l = x.float().cpu().numpy().astype(np.float64)
    visits, idx = _draw(rng, legal, l, C_)
    actions = vc.as_actions(idx, H, W, "tuple")
    g_ce, g_h = rng.randn(N), 0.01 * rng.randn(N)
    tb, tv, ta = _up(bits, dev), _up(visits, dev), _up(actions, dev)
    got = _run(env, x, tb, tv, ta, g_ce, g_h)
    fi, in_range = vt.flat_targets(actions, O, H, W)
    want_ce, want_ent, _, _ = vt.evaluate(l, legal, visits, fi, in_range)
    _close_with_inf(got["ce"], want_ce, 1e-4)
    np.testing.assert_allclose(got["ent"], want_ent, atol=1e-4, rtol=0)
    _gradient_bound(cfg, f"257 rows {dtype}", l, bits, legal, visits, actions, fi, in_range, g_ce, g_h, got["g"], dtype)
    perm = rng.permutation(N)
    tp = torch.from_numpy(perm).to(dev)
    shuffled = _run(env, x[tp].contiguous(), tb[tp].contiguous(), tv[tp].contiguous(), ta[tp].contiguous(), g_ce[perm], g_h[perm])
    assert _same_bytes(shuffled, {k: got[k][perm] for k in ("ce", "ent", "stats", "g_raw")})
    one = _run(env, x[:1].contiguous(), tb[:1].contiguous(), tv[:1].contiguous(), ta[:1].contiguous(), g_ce[:1], g_h[:1])
    assert _same_bytes(one, {k: got[k][:1] for k in ("ce", "ent", "stats", "g_raw")})
    # no row: the wrappers return empty tensors, and at the ABI the call succeeds and writes nothing
    ce0, ent0 = env.evaluate_visits_forward(x[:0].contiguous(), tb[:0].contiguous(), tv[:0].contiguous(), ta[:0].contiguous())
    assert ce0.shape == (0,) and ent0.shape == (0,)
    g0 = env.evaluate_visits_backward(x[:0].contiguous(), tb[:0].contiguous(), tv[:0].contiguous(), ta[:0].contiguous(),
                                      torch.empty((0, 4), dtype=torch.float32, device=dev), None, None)
    assert g0.shape == (0, A)
    keep = torch.full((8,), 7.0, device=dev)
    R = _train_lib.PcbenvVisitsRequest
    req = R(struct_size=C.sizeof(R), logits_dtype=_lib.LOGITS_F32 if dtype == torch.float32 else _lib.LOGITS_BF16, action_format=_lib.ACTION_TUPLE,
            num_targets=C_, num_rows=0, logits=x.data_ptr(), mask_bits=tb.data_ptr(), visits=tv.data_ptr(), target_actions=ta.data_ptr(),
            cross_entropy=keep.data_ptr(), entropy=keep.data_ptr(), stats=keep.data_ptr(), grad_logits=keep.data_ptr(), stream=env._stream().value)
    _lib.check(env._L.pcbenv_evaluate_visits(env._h, C.byref(req)), env._h)
    _lib.check(env._L.pcbenv_evaluate_visits_backward(env._h, C.byref(req)), env._h)
    assert bool((keep == 7.0).all())


@pytest.mark.parametrize("name", ["rect_9x70", "pin_40x48"])
def test_illegal_logits_are_never_read(name):
    """NaN on every illegal position changes no output bit, forward or backward."""
    env = _handle(name)
    cfg, dev = env.cfg, env.device
    O, H, W, A = _geom(cfg)
    rng = _rng("illegal", name)
    bits, legal = _rows(cfg, rng)
    visits, idx = vc.draw_targets(rng, legal, 16)
    tb, tv, ta = _up(bits, dev), _up(visits, dev), _up(vc.as_actions(idx, H, W, "flat"), dev)
    g_ce, g_h = rng.randn(ROWS), 0.01 * rng.randn(ROWS)
    tl = _up(legal, dev)
    assert not legal.all()
    for dtype in (torch.float32, torch.bfloat16):
        raw = _up(lc.tame(rng, legal), dev, dtype)
        base = _run(env, raw, tb, tv, ta, g_ce, g_h)
        for fill in (float("nan"), 3.0e38):
            got = _run(env, torch.where(tl, raw, torch.full_like(raw, fill)).contiguous(), tb, tv, ta, g_ce, g_h)
            assert _same_bytes(got, base) and got["err"] == base["err"] == 0, (name, dtype, fill)


@DTYPES
def test_autograd_wrapper_and_a_lagging_side_stream(dtype):
    """pcbenv.visit_targets.cross_entropy gives the bits of the direct calls; and both launches run on the stream they are
    given: on a non-blocking side stream, behind a delay, with inputs that are valid but stale until the delay has passed."""
    name = "pin_40x48"
    env = _handle(name)
    cfg, dev = env.cfg, env.device
    O, H, W, A = _geom(cfg)
    rng = _rng("stream", str(dtype))
    bits, legal = _rows(cfg, rng)
    visits, idx = vc.draw_targets(rng, legal, 16)
    g_ce, g_h = rng.randn(ROWS).astype(np.float32), (0.01 * rng.randn(ROWS)).astype(np.float32)
    true = dict(x=_up(lc.tame(rng, legal), dev, dtype), bits=_up(bits, dev), visits=_up(visits, dev),
                acts=_up(vc.as_actions(idx, H, W, "tuple"), dev), g_ce=_up(g_ce, dev), g_h=_up(g_h, dev))
    want = _run(env, true["x"], true["bits"], true["visits"], true["acts"], g_ce, g_h)
    # the autograd wrapper
    xg = true["x"].clone().requires_grad_(True)
    ce, ent = cross_entropy(env, xg, true["bits"], true["visits"], true["acts"])
    (ce * true["g_ce"] + ent * true["g_h"]).sum().backward()
    assert xg.grad.dtype == dtype
    itype = SENTINEL[dtype][0]
    assert np.array_equal(ce.detach().cpu().numpy().view(np.uint32), want["ce"].view(np.uint32))
    assert np.array_equal(ent.detach().cpu().numpy().view(np.uint32), want["ent"].view(np.uint32))
    assert np.array_equal(xg.grad.view(itype).cpu().numpy(), want["g_raw"])
    # the side stream: logits 0, no legal bit, no visits, action (0, 0, 0), gradients 0 until the delay has passed
    buf = {k: torch.zeros_like(v) for k, v in true.items()}
    stats = torch.zeros((ROWS, 4), dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    with lagged(side) as before:
        before()
        for k in ("x", "bits", "visits", "acts"):
            buf[k].copy_(true[k])
        ce_s, ent_s = env.evaluate_visits_forward(buf["x"], buf["bits"], buf["visits"], buf["acts"], stats, err)
        before()  # stats: still in flight
        buf["g_ce"].copy_(true["g_ce"]); buf["g_h"].copy_(true["g_h"])
        grad = env.evaluate_visits_backward(buf["x"], buf["bits"], buf["visits"], buf["acts"], stats, buf["g_ce"], buf["g_h"])
        side.synchronize()
    assert before.calls == 2 and int(err.item()) == 0
    assert np.array_equal(ce_s.cpu().numpy().view(np.uint32), want["ce"].view(np.uint32))
    assert np.array_equal(ent_s.cpu().numpy().view(np.uint32), want["ent"].view(np.uint32))
    assert np.array_equal(stats.cpu().numpy().view(np.uint32), want["stats"].view(np.uint32))
    assert np.array_equal(grad.view(itype).cpu().numpy(), want["g_raw"])


def test_einval_walk_with_a_handle():
    """The refusals in the header's order, on a live handle: each leaves pcbenv_last_error naming the field; the null handle
    comes last; and what passes them all with num_rows == 0 succeeds."""
    env = _handle("spatial_10x10")
    cfg, dev = env.cfg, env.device
    O, H, W, A = _geom(cfg)
    N, C_ = 4, 8
    L, R = env._L, _train_lib.PcbenvVisitsRequest
    x = torch.zeros((N, A + 4), dtype=torch.float32, device=dev)
    tb = torch.zeros((N, 2, H, 1), dtype=torch.int64, device=dev)
    tv = torch.zeros((N, C_ + 1), dtype=torch.int32, device=dev)
    ta = torch.zeros((N, C_, 3), dtype=torch.int32, device=dev)
    stats = torch.zeros((N + 1, 4), dtype=torch.float32, device=dev)
    grad = torch.zeros((N, A + 4), dtype=torch.float32, device=dev)
    ptr = dict(logits=x.data_ptr(), mask_bits=tb.data_ptr(), visits=tv.data_ptr(), target_actions=ta.data_ptr(), stats=stats.data_ptr(),
               grad_logits=grad.data_ptr())
    assert all(p % 16 == 0 for p in ptr.values())

    def call(backward, handle=True, request=True, **kw):
        fields = dict(struct_size=C.sizeof(R), logits_dtype=_lib.LOGITS_F32, action_format=_lib.ACTION_TUPLE, num_targets=C_, num_rows=N,
                      reserved=0, stream=env._stream().value, **ptr)
        fields.update(kw)
        req = R(**{k: v for k, v in fields.items() if v is not None})
        h = env._h if handle else None
        rc = (L.pcbenv_evaluate_visits_backward if backward else L.pcbenv_evaluate_visits)(h, C.byref(req) if request else None)
        return rc, L.pcbenv_last_error(h).decode()

    walk = [(dict(request=False), "null request"), (dict(struct_size=64), "struct_size"), (dict(logits_dtype=5), "unknown logits dtype"),
            (dict(action_format=3), "unknown action format"), (dict(num_targets=0), "num_targets"), (dict(num_targets=65), "num_targets"),
            (dict(num_rows=-1), "num_rows"), (dict(reserved=2), "reserved"),
            *[({k: None}, "null logits, mask_bits, visits or target_actions") for k in ("logits", "mask_bits", "visits", "target_actions")],
            (dict(logits=ptr["logits"] + 2), "logits pointer not aligned"), (dict(mask_bits=ptr["mask_bits"] + 4), "mask bits pointer not aligned"),
            (dict(visits=ptr["visits"] + 2), "4-byte aligned"), (dict(target_actions=ptr["target_actions"] + 1), "4-byte aligned"),
            (dict(stats=ptr["stats"] + 8), "stats pointer not aligned"), (dict(handle=False), "null handle")]
    for backward in (False, True):
        for i, (kw, msg) in enumerate(walk):
            rc, text = call(backward, **kw)
            assert rc == _lib.PCBENV_EINVAL and msg in text, (backward, kw, text)
            if 0 < i < len(walk) - 1:  # the order: what a later check refuses is also wrong, and the earlier one still decides
                later = walk[i + 1][0]
                if "handle" not in later and "request" not in kw and not set(later) & set(kw):
                    rc, text = call(backward, **{**later, **kw})
                    assert rc == _lib.PCBENV_EINVAL and msg in text, (backward, kw, later, text)
    for kw, msg in ((dict(stats=None), "null stats or grad_logits"), (dict(grad_logits=None), "null stats or grad_logits"),
                    (dict(grad_logits=None, logits=ptr["logits"] + 2), "null stats or grad_logits"),
                    (dict(grad_logits=ptr["grad_logits"] + 2), "grad logits pointer not aligned"),
                    (dict(grad_logits=ptr["grad_logits"] + 2, stats=ptr["stats"] + 4), "stats pointer not aligned")):
        rc, text = call(True, **kw)
        assert rc == _lib.PCBENV_EINVAL and msg in text, (kw, text)
    for backward in (False, True):  # one element past a 16-byte boundary is aligned enough; no row is a no-op
        assert call(backward, num_rows=0, logits=ptr["logits"] + 4, grad_logits=ptr["grad_logits"] + 4, visits=ptr["visits"] + 4)[0] == _lib.PCBENV_OK
