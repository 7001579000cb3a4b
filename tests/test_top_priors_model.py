"""csrc/pcb_topk.h -- the selection of pcbenv_top_priors as plain C++ -- against the float64 contract of
include/pcbenv_priors.h (tests/top_priors_cases.py:contract) on the CPU: tools/topk_model_check.cpp (AddressSanitizer +
UBSan, a program of its own, nothing preloaded) composes the header's pieces over every row of the case table in the
steps the kernel takes and dumps count, actions and priors.  Counts, actions, padding and error bits are exact; a prior is
within one float32 ulp of the correctly rounded float32 of the float64 value (the model sums Z in float64 in another
order than numpy, and its exp is the C library's).  tests/test_top_priors_gpu.py holds the kernel to the same contract."""
import shutil

import numpy as np
import pytest

import logits_cases as lc
import top_priors_cases as tc

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _check(label, l, legal, bits, O, H, W, Ks=tc.KS):
    got = tc.model(O, H, W, bits, l, Ks)
    for K in Ks:
        count, actions, prior, errors = tc.contract(l, legal, K, H, W)
        m_count, m_actions, m_prior, m_errors = got[K]
        assert np.array_equal(m_count, count), (label, K)
        assert np.array_equal(m_actions, actions), (label, K)
        assert int(np.bitwise_or.reduce(m_errors)) == errors, (label, K)
        want = prior.astype(np.float32)
        assert (np.abs(m_prior.astype(np.float64) - want.astype(np.float64)) <= lc.ulp32(want)).all(), (label, K)
        assert not m_prior[np.arange(K)[None, :] >= count[:, None]].any()
        bad = m_errors != 0
        assert np.array_equal(m_prior[bad], want[bad])  # float32(1.0 / n), exactly


@pytest.mark.parametrize("name", tc.GEOMETRIES)
def test_every_regime_on_the_synthetic_bit_rows(name):
    cfg, O, H, W = tc.geometry(name)
    legal, bits, names = tc.synthetic(name)
    regimes = list(tc.REGIMES)
    l = np.concatenate([tc.logits(name, regime, legal) for regime in regimes])
    _check(name, l, np.tile(legal, (len(regimes), 1)), np.tile(bits, (len(regimes), 1, 1, 1)), O, H, W)


@pytest.mark.parametrize("name", ["rect_33x65", "pin_40x48", "pin_100x9", "square_3x128"])
def test_bfloat16_values(name):
    cfg, O, H, W = tc.geometry(name)
    legal, bits, names = tc.synthetic(name)
    regimes = ["tame", "scale30", "near_uniform", "four_values", "denormals_mixed", "signed_zeros"]
    l = np.concatenate([tc.logits(name, regime, legal, bf16=True) for regime in regimes])
    _check(name + " bf16", l, np.tile(legal, (len(regimes), 1)), np.tile(bits, (len(regimes), 1, 1, 1)), O, H, W)


@pytest.mark.parametrize("name", tc.GEOMETRIES)
def test_legal_counts_around_K(name):
    cfg, O, H, W = tc.geometry(name)
    for K in tc.KS:
        legal, bits, targets = tc.counted(name, K)
        for regime in ("tame", "constant", "bad_rows"):
            _check(f"{name} counted {regime}", tc.logits(name, regime, legal), legal, bits, O, H, W, Ks=(K,))


def test_dirty_bit_rows_and_illegal_logits_change_nothing():
    for name in ("spatial_7x100", "square_3x128", "rect_9x70"):
        cfg, O, H, W = tc.geometry(name)
        legal, bits, names = tc.synthetic(name)
        l = tc.logits(name, "tame", legal)
        rng = tc.rng_for("dirty", name)
        twin = lc.dirty_twin(bits, cfg.kind, W, rng)
        poisoned = np.where(legal, l, rng.choice(np.array([np.nan, 3e38, -3e38], np.float32), size=l.shape))
        a, b, c = (tc.model(O, H, W, bb, ll, (3, 64)) for bb, ll in ((bits, l), (twin, l), (bits, poisoned)))
        for K in (3, 64):
            for x, y, z in zip(a[K], b[K], c[K]):
                assert x.tobytes() == y.tobytes() == z.tobytes(), (name, K)
