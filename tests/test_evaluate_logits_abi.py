"""pcbenv_evaluate_logits / pcbenv_evaluate_logits_backward on the CPU side: the header declares both, libpcbenv.so
exports them, pcbenv/_lib.py binds them, and every argument check refuses what it must before anything touches a device.
Also the float64 restatement of the contract (tests/evaluate_contract.py) against torch float64 autograd through the
reference's chain (masked_logits + Categorical), and masked_categorical.evaluate_torch against the restatement.  No
compute call is made."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import evaluate_contract as ec
from abi_header import text as _header
from pcbenv import _lib
from pcbenv.masked_categorical import evaluate, evaluate_torch, unpack_mask_bits
from pcbenv.rollout import masked_logits

SHAPES = [(1, 8, 8), (2, 6, 6), (4, 10, 10), (4, 16, 64), (4, 5, 128), (4, 7, 100), (2, 33, 65), (1, 3, 128), (4, 100, 9)]


def test_header_declares_both_signatures():
    text = _header()
    common = (r"\s*\(\s*const\s+pcbenv\s*\*\s*env\s*,\s*const\s+void\s*\*\s*logits_dev\s*,\s*int32_t\s+logits_dtype\s*,"
              r"\s*const\s+uint64_t\s*\*\s*mask_bits_dev\s*,\s*const\s+int32_t\s*\*\s*actions_dev\s*,\s*int32_t\s+action_format\s*,"
              r"\s*int64_t\s+num_rows\s*,")
    fwd = (r"\bint\s+pcbenv_evaluate_logits" + common + r"\s*float\s*\*\s*log_prob_dev\s*,\s*float\s*\*\s*entropy_dev\s*,"
           r"\s*float\s*\*\s*stats_dev\s*,\s*uint32_t\s*\*\s*errors_dev\s*,\s*void\s*\*\s*stream\s*\)\s*;")
    bwd = (r"\bint\s+pcbenv_evaluate_logits_backward" + common + r"\s*const\s+float\s*\*\s*stats_dev\s*,"
           r"\s*const\s+float\s*\*\s*grad_log_prob_dev\s*,\s*const\s+float\s*\*\s*grad_entropy_dev\s*,"
           r"\s*void\s*\*\s*grad_logits_dev\s*,\s*void\s*\*\s*stream\s*\)\s*;")
    assert re.search(fwd, text)
    assert re.search(bwd, text)
    assert re.search(r"#define\s+PCBENV_ABI_VERSION\s+3\b", text)


def test_exported_and_bound():
    L = _lib.load()
    for name in ("pcbenv_evaluate_logits", "pcbenv_evaluate_logits_backward"):
        assert name in _lib.EXPORTS
        assert hasattr(L, name)
        assert len(getattr(L, name).argtypes) == 12
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3  # an addition: the ABI version stays


def _call(which, env=None, logits=True, dtype=_lib.LOGITS_F32, mask=True, actions=True, fmt=_lib.ACTION_FLAT, rows=4,
          stats=True, grad=True, offset=0, grad_offset=0, mask_offset=0, stats_offset=0):
    L = _lib.load()
    host = (C.c_uint64 * 16)()  # host memory: never dereferenced, every call below fails before a device is touched
    base = (C.addressof(host) + 15) & ~15
    acts = (C.c_int32 * 4)()
    lp = C.c_void_p(base + offset) if logits else None
    mp = C.c_void_p(base + mask_offset) if mask else None
    ap = C.cast(acts, C.c_void_p) if actions else None
    sp = C.c_void_p(base + stats_offset) if stats else None
    if which == "forward":
        rc = L.pcbenv_evaluate_logits(env, lp, dtype, mp, ap, fmt, rows, None, None, sp, None, None)
    else:
        gp = C.c_void_p(base + grad_offset) if grad else None
        rc = L.pcbenv_evaluate_logits_backward(env, lp, dtype, mp, ap, fmt, rows, sp, None, None, gp, None)
    return rc, L.pcbenv_last_error(None).decode()


COMMON_CHECKS = [
    ({}, "null handle"),
    ({"logits": False}, "null logits"),
    ({"mask": False}, "null mask bits"),
    ({"actions": False}, "null actions"),
    ({"dtype": 2}, "unknown logits dtype"),
    ({"dtype": -1}, "unknown logits dtype"),
    ({"fmt": 7}, "unknown action format"),
    ({"offset": 1}, "logits pointer not aligned"),
    ({"offset": 2}, "logits pointer not aligned"),
    ({"offset": 1, "dtype": _lib.LOGITS_BF16}, "logits pointer not aligned"),
    ({"offset": 2, "dtype": _lib.LOGITS_BF16}, "null handle"),  # 2-byte alignment is enough for bf16
    ({"mask_offset": 4}, "mask bits pointer not aligned"),
    ({"stats_offset": 8}, "stats pointer not aligned"),
    ({"rows": -1}, "num_rows"),
    ({"rows": 0}, "null handle"),  # the handle is checked before the no-op return
    ({"fmt": _lib.ACTION_TUPLE}, "null handle"),
]


@pytest.mark.parametrize("kw, msg", COMMON_CHECKS + [({"stats": False}, "null handle")])  # forward: stats may be NULL
def test_forward_argument_checks_need_no_device(kw, msg):
    rc, err = _call("forward", **kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err


@pytest.mark.parametrize("kw, msg", COMMON_CHECKS + [
    ({"stats": False}, "null stats"),
    ({"grad": False}, "null grad logits"),
    ({"grad_offset": 2}, "grad logits pointer not aligned"),
    ({"grad_offset": 1, "dtype": _lib.LOGITS_BF16}, "grad logits pointer not aligned"),
    ({"grad_offset": 2, "dtype": _lib.LOGITS_BF16}, "null handle"),
])
def test_backward_argument_checks_need_no_device(kw, msg):
    rc, err = _call("backward", **kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err


# ---- the float64 restatement against torch float64 autograd through the reference's chain --------------------------

def _random_bits(rng, H, W, p):
    bits = np.zeros((2, H, (W + 63) // 64), np.uint64)
    cells = rng.rand(2, H, W) < p
    for pl in range(2):
        for x in range(H):
            for y in np.flatnonzero(cells[pl, x]):
                bits[pl, x, y // 64] |= np.uint64(1) << np.uint64(y % 64)
    return bits


def _case(O, H, W, N=12, seed=0, p_neg_inf=0.05):
    """Random legal sets (sparse, medium, full), scale-3 logits with legal -inf entries, stored legal actions."""
    rng = np.random.RandomState(seed + O * 1000 + H + W)
    A = O * H * W
    bits = np.stack([_random_bits(rng, H, W, rng.choice([0.05, 0.3, 1.0])) for _ in range(N)])
    legal = ec.legal_rows(bits, O, H, W)
    l = rng.randn(N, A) * 3.0
    l[rng.rand(N, A) < p_neg_inf] = -np.inf
    a = np.zeros(N, np.int64)
    for r in range(N):
        idx = np.flatnonzero(legal[r])
        if idx.size == 0:
            bits[r, 0, 0, 0] |= np.uint64(1)
            legal[r] = ec.legal_rows(bits[r:r + 1], O, H, W)[0]
            idx = np.flatnonzero(legal[r])
        if not np.isfinite(l[r, idx]).any():
            l[r, idx[0]] = 0.0
        finite = idx[np.isfinite(l[r, idx])]
        a[r] = finite[rng.randint(finite.size)]
    return rng, bits, legal, l, a


def _torch_chain(l, legal, a, g_lp, g_h, dtype=torch.float64):
    """masked_logits + Categorical, autograd: (log_prob, entropy, gradient) as numpy float64."""
    x = torch.tensor(l, dtype=dtype, requires_grad=True)
    d = torch.distributions.Categorical(logits=masked_logits(x, torch.from_numpy(legal)), validate_args=False)
    lp, ent = d.log_prob(torch.from_numpy(a)), d.entropy()
    (lp * torch.tensor(g_lp, dtype=dtype) + ent * torch.tensor(g_h, dtype=dtype)).sum().backward()
    return lp.detach().double().numpy(), ent.detach().double().numpy(), x.grad.double().numpy()


@pytest.mark.parametrize("O, H, W", SHAPES)
def test_restatement_equals_torch_float64_autograd(O, H, W):
    for seed in range(3):
        rng, bits, legal, l, a = _case(O, H, W, seed=seed)
        assert (legal & np.isneginf(l)).any()  # legal -inf entries are part of the case
        g_lp, g_h = rng.randn(len(a)), 0.01 * rng.randn(len(a))
        lp, ent, err, status = ec.evaluate(l, legal, a)
        g = ec.gradient(l, legal, a, g_lp, g_h)
        assert err == 0 and (status == ec.ROW_OK).all()
        # the chain needs finite inputs where the mask is 0; what it computes there is the masked value's business
        want_lp, want_ent, want_g = _torch_chain(np.where(legal, l, 0.0), legal, a, g_lp, g_h)
        np.testing.assert_allclose(lp, want_lp, atol=1e-12, rtol=0)
        np.testing.assert_allclose(ent, want_ent, atol=1e-12, rtol=0)
        np.testing.assert_allclose(g, want_g, atol=1e-12, rtol=0)
        assert np.isfinite(g).all()
        assert not g[~legal].any()  # exactly 0 at illegal positions


@pytest.mark.parametrize("O, H, W", SHAPES)
def test_restatement_never_reads_an_illegal_logit(O, H, W):
    rng, bits, legal, l, a = _case(O, H, W, seed=5)
    g_lp, g_h = rng.randn(len(a)), 0.01 * rng.randn(len(a))
    base = ec.evaluate(l, legal, a), ec.gradient(l, legal, a, g_lp, g_h)
    for junk in (np.nan, np.inf, -3.4e38):
        hurt = np.where(legal, l, junk)
        lp, ent, err, status = ec.evaluate(hurt, legal, a)
        assert err == 0
        assert np.array_equal(lp, base[0][0]) and np.array_equal(ent, base[0][1])
        assert np.array_equal(ec.gradient(hurt, legal, a, g_lp, g_h), base[1])


def test_restatement_edge_cases():
    O, H, W = 2, 6, 6
    rng, bits, legal, l, a = _case(O, H, W, N=6, seed=9, p_neg_inf=0.0)
    A = O * H * W
    legal[0] = False                                        # no legal action
    l[1, np.flatnonzero(legal[1])[0]] = np.nan              # a legal NaN
    l[2, np.flatnonzero(legal[2])[-1]] = np.inf             # a legal +inf
    l[3, legal[3]] = -np.inf                                # every legal logit -inf
    legal[4, 7] = False
    a[4] = 7                                                # stored action not legal
    g_lp, g_h = rng.randn(6), rng.randn(6)
    lp, ent, err, status = ec.evaluate(l, legal, a)
    g = ec.gradient(l, legal, a, g_lp, g_h)
    n = legal.sum(1)
    assert err == ec.ERR_NONFINITE | ec.ERR_ALL_NEG_INF | ec.ERR_ACTION
    assert lp[0] == 0 and ent[0] == 0
    for r in (1, 2, 3):
        assert lp[r] == -np.log(n[r]) and ent[r] == np.log(n[r])
    assert lp[4] == 0 and ent[4] > 0
    assert list(status) == [ec.ROW_ZERO] * 4 + [ec.ROW_NO_ONE_HOT, ec.ROW_OK]
    assert not g[:4].any() and np.isfinite(g).all()
    # row 4: the gradient of g_H * entropy alone plus the -g_lp p term, no one-hot
    b = a.copy()
    b[4] = np.flatnonzero(legal[4])[0]
    with_hot = ec.gradient(l, legal, b, g_lp, g_h)
    diff = with_hot[4] - g[4]
    assert diff[b[4]] == pytest.approx(g_lp[4], rel=1e-12) and np.count_nonzero(diff) == 1
    # out of range: the same as not legal
    for bad in (-1, A, 1 << 20):
        c = a.copy()
        c[5] = bad
        lp2, ent2, err2, status2 = ec.evaluate(l[5:], legal[5:], c[5:])
        assert lp2[0] == 0 and ent2[0] == ent[5] and err2 == ec.ERR_ACTION and status2[0] == ec.ROW_NO_ONE_HOT
    assert ec.evaluate(l[5:], legal[5:], a[5:])[2] == 0


def test_tuple_and_flat_actions_agree():
    O, H, W = 4, 10, 10
    rng, bits, legal, l, a = _case(O, H, W, seed=2)
    tup = np.stack([a // (H * W), (a % (H * W)) // W, a % W], 1)
    assert np.array_equal(ec.flat_actions(tup, H, W), a)
    assert ec.tuple_in_range(tup, O, H, W).all()
    assert not ec.tuple_in_range(np.array([[0, 0, W], [O, 0, 0], [0, -1, 0]]), O, H, W).any()


# ---- evaluate_torch (what evaluate() runs off the device) against the restatement ----------------------------------

@pytest.mark.parametrize("O, H, W", SHAPES)
@pytest.mark.parametrize("fmt", ["flat", "tuple"])
def test_evaluate_torch_equals_the_restatement(O, H, W, fmt):
    cfg = SimpleNamespace(num_orientations=O, height=H, width=W)
    rng, bits, legal, l, a = _case(O, H, W, seed=3)
    bits[0] = 0                                             # a row without a legal action: 0 / 0 / zero gradient
    legal[0] = False
    tb = torch.from_numpy(bits.view(np.int64))
    assert np.array_equal(unpack_mask_bits(cfg, tb).numpy(), legal)
    acts = torch.from_numpy(a.astype(np.int32))
    if fmt == "tuple":
        acts = torch.stack([acts // (H * W), (acts % (H * W)) // W, acts % W], 1).to(torch.int32)
    g_lp, g_h = rng.randn(len(a)), 0.01 * rng.randn(len(a))
    want_lp, want_ent, err, _ = ec.evaluate(l, legal, a)
    want_lp[0] = 0.0  # row 0's stored action is moot
    want_g = ec.gradient(l, legal, a, g_lp, g_h)
    for junk in (0.0, np.nan):                              # NaNs planted at illegal positions change nothing
        x = torch.tensor(np.where(legal, l, junk), dtype=torch.float64, requires_grad=True)
        lp, ent = evaluate(SimpleNamespace(cfg=cfg), x, tb, acts)  # CPU tensors: evaluate_torch
        (lp * torch.from_numpy(g_lp) + ent * torch.from_numpy(g_h)).sum().backward()
        np.testing.assert_allclose(lp.detach().numpy(), want_lp, atol=1e-12, rtol=0)
        np.testing.assert_allclose(ent.detach().numpy(), want_ent, atol=1e-12, rtol=0)
        np.testing.assert_allclose(x.grad.numpy(), want_g, atol=1e-12, rtol=0)
        assert not x.grad.numpy()[~legal].any()
    # float32 logits: the float32 chain, within float32 rounding of the float64 statement
    x32 = torch.tensor(np.where(legal, l, 0.0), dtype=torch.float32)
    lp32, ent32 = evaluate_torch(cfg, x32, tb, acts)
    l32 = x32.double().numpy()
    l32[~legal] = 0.0
    w_lp, w_ent, _, _ = ec.evaluate(np.where(legal, x32.double().numpy(), 0.0), legal, a)
    w_lp[0] = 0.0
    np.testing.assert_allclose(lp32.numpy(), w_lp, atol=1e-4, rtol=0)
    np.testing.assert_allclose(ent32.numpy(), w_ent, atol=1e-4, rtol=0)
