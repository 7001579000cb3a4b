"""The helpers of the logits edge tests (tests/logits_cases.py), on the CPU: the ragged configurations are valid and
select the template instantiations they are listed for, the synthetic bit rows hold the legal sets they claim and their
dirty twins the same ones, and the float64 contract itself is pinned in every logit regime."""
import numpy as np
import pytest

import evaluate_contract as ec
import logits_cases as lc
from pcbenv import named_config
from pcbenv.config import KIND_SQUARE

GEOMETRIES = {name: make for name, make in lc.RAGGED.items()}
GEOMETRIES.update({"c3": lambda: named_config("c3"), "c1": lambda: named_config("c1")})


@pytest.mark.parametrize("name", list(lc.RAGGED))
def test_ragged_configurations_are_valid_and_select_their_path(name):
    cfg = lc.RAGGED[name]()
    cfg.validate()
    cfg.check_device_limits()
    O, H, W, vec, nw = lc.EXPECTED[name]
    assert (cfg.num_orientations, cfg.height, cfg.width) == (O, H, W) and H != W
    assert lc.launch_path(cfg) == (vec, nw)
    assert lc.launch_path(cfg, aligned=False) == (False, nw)


def test_every_instantiation_is_reached():
    """(VEC, NW) over the ragged set and the named configurations, with aligned pointers: all four, so with two dtypes all
    eight <T, VEC, NW> of each kernel."""
    seen = {lc.launch_path(make()) for make in lc.RAGGED.values()} | {lc.launch_path(named_config(n)) for n in ("c1", "c3", "c5")}
    assert seen == {(True, 1), (True, 4), (False, 1), (False, 4)}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_bit_rows_hold_what_they_claim(name):
    cfg = GEOMETRIES[name]()
    O, H, W = cfg.num_orientations, cfg.height, cfg.width
    classes = lc.mask_classes(cfg.kind, O, H, W, np.random.RandomState(1))
    names = [n for n, _, _ in classes]
    assert {"density_0.02", "density_0.5", "density_0.98", "full", "none", "last_bit"} <= set(names)
    assert ("col63" in names) == (W > 63) and ("col64" in names) == ("word1_only" in names) == (W > 64)
    assert ("plane1_only" in names) == (cfg.kind != KIND_SQUARE)
    WW = (W + 63) // 64
    for cname, clean, count in classes:
        assert clean.dtype == np.uint64 and clean.shape[1:] == (2, H, WW)
        legal = ec.legal_rows(clean, O, H, W)
        assert np.array_equal(legal.sum(1), count), cname
        dirty = lc.dirty_twin(clean, cfg.kind, W, np.random.RandomState(2))
        assert np.array_equal(ec.legal_rows(dirty, O, H, W), legal), cname
        if W % 64 or cfg.kind == KIND_SQUARE:
            assert not np.array_equal(dirty.view(np.uint64), clean), cname  # the twin is dirty
        if W % 64:  # every padding bit is set
            assert ((dirty.view(np.uint64)[..., WW - 1] >> np.uint64(W % 64)) == (~np.uint64(0) >> np.uint64(W % 64))).all()
        reps = {1: 1, 2: 1, 4: 2}[O]
        if cname == "full":
            assert (count == O * H * W).all()
        if cname == "none":
            assert (count == 0).all()
        if cname in ("last_bit", "col63", "col64"):
            assert (count == (reps if cname == "last_bit" or O == 4 else 1)).all()
            o, x, y = {"last_bit": (O - 1, H - 1, W - 1), "col63": (0, H // 2, 63), "col64": (0, H // 2, 64)}[cname]
            assert legal[0, o * H * W + x * W + y]
        if cname == "word1_only":
            assert (count > 0).all() and not legal.reshape(-1, O * H, W)[:, :, :64].any()
        if cname == "plane1_only":
            assert (count > 0).all() and not legal.reshape(-1, O, H * W)[:, 0::2].any()
    all_rows = lc.bits(cfg.kind, O, H, W, np.random.RandomState(1))
    assert all_rows.dtype == np.int64 and all_rows.shape == (sum(len(c) for _, c, _ in classes), 2, H, WW)
    assert np.array_equal(all_rows.view(np.uint64), np.concatenate([c for _, c, _ in classes]))


def _random_legal(rng, N, A, p=0.3):
    legal = rng.rand(N, A) < p
    legal[:, 0] |= ~legal.any(1)
    return legal


@pytest.mark.parametrize("regime", list(lc.REGIMES) + ["offset", "offset_shifted", "offset_bf16", "offset_bf16_shifted"])
def test_contract_in_the_regimes(regime):
    """N = 64, A = 2 800, random 30 % masks: the float64 contract is finite with no error bit in every regime, and the
    float32 chain -- the source of e_ref -- is finite on every row, in huge_spread on at least a quarter of them."""
    import torch
    rng = np.random.RandomState(11)
    N, A = 64, 2800
    legal = _random_legal(rng, N, A)
    if regime.startswith("offset"):
        base, shifted, shift = lc.offset_pair(rng, legal, "bf16" in regime)
        assert np.array_equal(shifted - np.float32(shift), base)
        l32 = shifted if regime.endswith("shifted") else base
    else:
        l32 = lc.REGIMES[regime](rng, legal)
    assert l32.dtype == np.float32 and l32.shape == (N, A)
    for dtype in (torch.float32, torch.bfloat16):
        l = torch.from_numpy(l32).to(dtype).double().numpy()  # what a kernel would read
        if regime.startswith("offset") and ("bf16" in regime or dtype == torch.float32):
            assert np.array_equal(l, l32.astype(np.float64))  # exact in the dtype
        a = lc.stored_actions(rng, legal, l, peak_rows=regime.startswith("peaked"))
        assert legal[np.arange(N), a].all() and np.isfinite(l[np.arange(N), a]).all()
        g_lp, g_h = rng.randn(N), 0.01 * rng.randn(N)
        lp, ent, err, status = ec.evaluate(l, legal, a)
        g = ec.gradient(l, legal, a, g_lp, g_h)
        assert err == 0 and (status == ec.ROW_OK).all()
        assert np.isfinite(lp).all() and np.isfinite(ent).all() and np.isfinite(g).all() and not g[~legal].any()
        assert (ent >= -1e-12).all() and (lp <= 1e-12).all()
        _, _, _, finite = lc.chain32(l, legal, a, g_lp, g_h)
        if regime == "huge_spread":
            top = (legal & (l == l.max())).sum(1)
            assert (top >= 1).all() and (top < legal.sum(1)).all()
            np.testing.assert_allclose(ent, np.log(top), rtol=0, atol=1e-15)
            on_top = l[np.arange(N), a] > 0
            np.testing.assert_allclose(lp[on_top], -np.log(top[on_top]), rtol=0, atol=1e-15)
            with np.errstate(over="ignore"):
                assert (lp[~on_top].astype(np.float32) == -np.inf).all()  # -6e38 - log Z: -inf once it is a float32
            assert 4 * finite.sum() >= N and not finite.all()
        else:
            assert finite.all()
        if regime == "huge_equal":
            np.testing.assert_allclose(ent, np.log(legal.sum(1)), rtol=0, atol=1e-12)
        if regime == "peaked30" and dtype == torch.float32:
            assert (ent < 1e-6).all() and (lp[0::2] > -1e-7).all() and (lp[1::2] < -20).all()
        if regime == "underflow":
            assert (np.exp(l[legal] - 0.0).astype(np.float32) == 0).mean() > 0.4  # half the weights are 0 in float32


def test_ulp32():
    assert lc.ulp32(1.0) == 2.0 ** -23 and lc.ulp32(-1650.0) == 2.0 ** -13 and lc.ulp32(np.inf) == 0.0
    assert lc.ulp32(np.array([0.0]))[0] == np.spacing(np.float32(0))
