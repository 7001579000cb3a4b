"""tests/visits_contract.py -- the float64 restatement of include/pcbenv_train.h -- against torch float64 autograd through
the reference's masked chain (masked_logits + log_softmax) with the dense scattered target, and
pcbenv/visit_targets.py:cross_entropy_torch, the specification the kernels replace, against both.  No device."""
from types import SimpleNamespace

import numpy as np
import torch

import visits_cases as vc
import visits_contract as vt
from logits_cases import _pack
from pcbenv.rollout import masked_logits
from pcbenv.visit_targets import cross_entropy_torch, dense_targets

O, H, W = 2, 5, 7
A = O * H * W
CFG = SimpleNamespace(num_orientations=O, height=H, width=W)


def _chain64(l, legal, visits, actions, g_ce, g_h):
    """torch float64: (cross entropy, entropy, gradient of sum g_ce ce + g_h ent)."""
    tl = torch.from_numpy(legal)
    x = torch.tensor(np.where(legal, l, 0.0), dtype=torch.float64, requires_grad=True)
    masked = masked_logits(x, tl)
    logp = torch.log_softmax(masked, dim=1)
    pi, T = dense_targets(CFG, tl, torch.from_numpy(visits), torch.from_numpy(actions), torch.float64)
    ce = -torch.where(pi > 0, pi * logp, torch.zeros_like(logp)).sum(1)
    ent = torch.distributions.Categorical(logits=masked, validate_args=False).entropy()
    (ce * torch.from_numpy(g_ce) + ent * torch.from_numpy(g_h)).sum().backward()
    return ce.detach().numpy(), ent.detach().numpy(), x.grad.numpy(), T.numpy()


def _random(seed, N, C):
    rng = np.random.RandomState(seed)
    cells, legal = vc.planes_legal(rng, O, H, W, N)
    l = (rng.randn(N, A) * 3).astype(np.float32).astype(np.float64)
    visits, idx = vc.draw_targets(rng, legal, C)
    return rng, cells, legal, l, visits, idx


def test_contract_is_torch_float64_autograd():
    for C, fmt in ((1, "flat"), (4, "tuple"), (16, "flat"), (64, "tuple")):
        rng, _, legal, l, visits, idx = _random(C, 12, C)
        if C >= 4:  # duplicates, zero, negative and illegal entries, T == 0
            idx[0, :] = idx[0, 0]
            visits[1, 0], visits[1, 1] = 0, 7
            visits[2, 0], visits[2, 1] = -4, 7
            idx[3, 1] = np.flatnonzero(~legal[3])[0]
            visits[3, 1], visits[3, 2] = 9, 5
            idx[4, 0], visits[4, 0], visits[4, 1] = A + 3, 6, 2
            visits[5] = 0
            on_dead = idx[6, 0]                      # a target on a legal -inf logit: cross entropy +inf, g = -g_ce pi there
            l[6, on_dead], visits[6, 0] = -np.inf, 3
            idx[6, 1:] = np.flatnonzero(legal[6] & (np.arange(A) != on_dead))[0]  # (the other entries name one finite logit)
            visits[6, 1] = 5
            off = np.flatnonzero(legal[7] & ~np.isin(np.arange(A), idx[7]))[0]
            l[7, off] = -np.inf                      # a legal -inf logit no entry names: p = 0, gradient 0 there
        actions = vc.as_actions(idx, H, W, fmt)
        fi, in_range = vt.flat_targets(actions, O, H, W)
        g_ce, g_h = rng.randn(12), rng.uniform(-1, 1, 12)  # |g_h| <= 1: the chain multiplies it with the mask's float.min
        ce, ent, bits, status = vt.evaluate(l, legal, visits, fi, in_range)
        g = vt.gradient(l, legal, visits, fi, in_range, g_ce, g_h)
        tce, tent, tg, T = _chain64(l, legal, visits, actions, g_ce, g_h)
        assert legal.any(1).all()
        inf = np.isinf(tce)
        assert np.array_equal(ce[inf], tce[inf]) and np.array_equal(np.flatnonzero(inf), [6] if C >= 4 else [])
        np.testing.assert_allclose(ce[~inf], tce[~inf], atol=1e-12, rtol=0)
        np.testing.assert_allclose(ent, tent, atol=1e-12, rtol=0)
        assert np.isfinite(tg).all()
        np.testing.assert_allclose(g, tg, atol=1e-12, rtol=0)
        assert not g[~legal].any()
        assert bits == (vt.ERR_TARGET if C >= 4 else 0)
        assert np.array_equal(status, np.where(T > 0, vt.ROW_OK, vt.ROW_NO_TARGET))
        if C >= 4:
            assert ce[6] == np.inf and g[7, off] == 0 and tg[7, off] == 0
            assert abs(g[6, on_dead] + g_ce[6] * 3.0 / visits[6].sum()) < 1e-15 and g[6, on_dead] != 0  # p = 0: -g_ce pi alone
            assert status[5] == vt.ROW_NO_TARGET and ce[5] == 0 and ent[5] > 0
            # the g_ce term is dropped where T == 0: the row is the entropy's gradient alone
            only_h = vt.gradient(l, legal, visits, fi, in_range, None, g_h)
            assert np.array_equal(g[5], only_h[5])
            # rows of a probability-simplex gradient sum to 0 when g_H = 0
            assert np.abs(vt.gradient(l, legal, visits, fi, in_range, g_ce, None).sum(1)).max() < 1e-12


def test_the_edge_table():
    rng = np.random.RandomState(3)
    N, C = len(vc.EDGE_ROWS), 5
    _, legal = vc.planes_legal(rng, O, H, W, N)
    l = (rng.randn(N, A) * 3).astype(np.float32)
    legal, l, visits, idx = vc.edge_batch(rng, legal, l, C, A)
    row = {n: i for i, n in enumerate(vc.EDGE_ROWS)}
    n = legal.sum(1)
    for fmt in ("flat", "tuple"):
        fi, in_range = vt.flat_targets(vc.as_actions(idx, H, W, fmt), O, H, W)
        assert not in_range[row["out_of_range"], 1] and in_range.sum() == in_range.size - 1
        ce, ent, bits, status = vt.evaluate(l.astype(np.float64), legal, visits, fi, in_range)
        g = vt.gradient(l.astype(np.float64), legal, visits, fi, in_range, rng.randn(N), rng.randn(N))
        assert bits == vt.ERR_NONFINITE | vt.ERR_ALL_NEG_INF | vt.ERR_TARGET
        assert ce[row["no_legal"]] == 0 and ent[row["no_legal"]] == 0
        for name in ("nan", "pos_inf", "all_neg_inf"):
            r = row[name]
            assert ce[r] == ent[r] == np.log(n[r]) and status[r] == vt.ROW_ZERO and not g[r].any()
        assert status[row["no_legal"]] == vt.ROW_ZERO and not g[row["no_legal"]].any()
        for name in ("plain", "zero_visits_entry", "negative_visits", "illegal_action", "out_of_range", "duplicates", "target_on_neg_inf"):
            assert status[row[name]] == vt.ROW_OK, name
        assert status[row["no_target"]] == vt.ROW_NO_TARGET and ce[row["no_target"]] == 0 and ent[row["no_target"]] > 0
        assert ce[row["target_on_neg_inf"]] == np.inf and np.isfinite(np.delete(ce, row["target_on_neg_inf"])).all()
        assert np.isfinite(g).all()
        # each bit-2 row alone raises the bit; the silent rows raise none
        for name, want in (("plain", 0), ("zero_visits_entry", 0), ("no_target", 0), ("duplicates", 0), ("target_on_neg_inf", 0),
                           ("negative_visits", vt.ERR_TARGET), ("illegal_action", vt.ERR_TARGET), ("out_of_range", vt.ERR_TARGET), ("no_legal", 0)):
            r = [row[name]]
            assert vt.evaluate(l[r].astype(np.float64), legal[r], visits[r], fi[r], in_range[r])[2] == want, name
        # an ignored entry is as if it were not there
        for name, c in (("zero_visits_entry", 1), ("negative_visits", 0), ("illegal_action", 2), ("out_of_range", 1)):
            r = [row[name]]
            keep = [k for k in range(C) if k != c]
            assert vt.evaluate(l[r].astype(np.float64), legal[r], visits[r][:, keep], fi[r][:, keep], in_range[r][:, keep])[0] == ce[r[0]]
        # duplicates add up: the same row with the repeated entries merged into one
        r = [row["duplicates"]]
        merged_v = np.array([[visits[r[0], :-1].sum(), visits[r[0], -1]]], np.int32)
        merged_i = fi[r][:, [0, C - 1]]
        np.testing.assert_allclose(vt.evaluate(l[r].astype(np.float64), legal[r], merged_v, merged_i, np.ones((1, 2), bool))[0], ce[r[0]], atol=1e-12)


def test_cross_entropy_torch_is_the_contract():
    """The specification in pcbenv/visit_targets.py, from packed bits, float64 and float32, both formats, with autograd."""
    rng, cells, legal, l, visits, idx = _random(9, 10, 8)
    legal[0] = False
    cells[0] = False
    visits[1] = 0
    idx[2, :] = idx[2, 0]
    bits = torch.from_numpy(_pack(cells).view(np.int64))
    g_ce, g_h = rng.randn(10), rng.uniform(-1, 1, 10)
    for fmt in ("flat", "tuple"):
        actions = vc.as_actions(idx, H, W, fmt)
        fi, in_range = vt.flat_targets(actions, O, H, W)
        want_ce, want_ent, _, _ = vt.evaluate(l, legal, visits, fi, in_range)
        want_g = vt.gradient(l, legal, visits, fi, in_range, g_ce, g_h)
        has = legal.any(1)
        for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 2e-5)):
            x = torch.tensor(l, dtype=dtype, requires_grad=True)
            ce, ent = cross_entropy_torch(CFG, x, bits, torch.from_numpy(visits), torch.from_numpy(actions))
            assert ce.dtype == dtype and ce.shape == (10,)
            np.testing.assert_allclose(ce.detach().double().numpy(), want_ce, atol=tol, rtol=0)
            np.testing.assert_allclose(ent.detach().double().numpy(), want_ent, atol=tol, rtol=0)
            assert ce[0] == 0 and ent[0] == 0 and ce[1] == 0 and ent[1] > 0
            (ce * torch.from_numpy(g_ce).to(dtype) + ent * torch.from_numpy(g_h).to(dtype)).sum().backward()
            # a row without a legal action is zero by contract and untouched by the chain's `where`
            np.testing.assert_allclose(x.grad.double().numpy()[has], want_g[has], atol=tol, rtol=0)
            assert not x.grad[0].any()
