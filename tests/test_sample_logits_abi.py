"""pcbenv_sample_logits on the CPU side: the header declares it with both enums, libpcbenv.so exports it,
pcbenv/_lib.py binds it, and every argument check refuses what it must before anything touches a device.  Also the
float64 restatement of the contract (tests/sampling_contract.py) against the uniform pick.  No compute call is made."""
import ctypes as C
import re

import numpy as np
import pytest

import sampling_contract as sc
from abi_header import text as _header
from pcbenv import _lib


def test_header_declares_signature_and_enums():
    text = _header()
    sig = (r"\bint\s+pcbenv_sample_logits\s*\(\s*pcbenv\s*\*\s*env\s*,\s*const\s+void\s*\*\s*logits_dev\s*,\s*int32_t\s+logits_dtype\s*,"
           r"\s*int32_t\s+mode\s*,\s*int32_t\s*\*\s*actions_dev\s*,\s*int32_t\s+action_format\s*,\s*float\s*\*\s*log_prob_dev\s*,"
           r"\s*float\s*\*\s*entropy_dev\s*,\s*uint32_t\s*\*\s*errors_dev\s*,\s*uint64_t\s+seed\s*,\s*uint64_t\s+first_env_index\s*,"
           r"\s*uint64_t\s+step_index\s*,\s*void\s*\*\s*stream\s*\)\s*;")
    assert re.search(sig, text)
    assert re.search(r"enum\s+pcbenv_logits_dtype\s*\{\s*PCBENV_LOGITS_F32\s*=\s*0\s*,\s*PCBENV_LOGITS_BF16\s*=\s*1\s*\}", text)
    assert re.search(r"enum\s+pcbenv_draw_mode\s*\{\s*PCBENV_DRAW_SAMPLE\s*=\s*0\s*,\s*PCBENV_DRAW_GREEDY\s*=\s*1\s*\}", text)
    assert (_lib.LOGITS_F32, _lib.LOGITS_BF16, _lib.DRAW_SAMPLE, _lib.DRAW_GREEDY) == (0, 1, 0, 1)


def test_exported_and_bound():
    assert "pcbenv_sample_logits" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(L, "pcbenv_sample_logits")
    assert len(L.pcbenv_sample_logits.argtypes) == 13
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3  # an addition: the ABI version stays


def _call(env=None, logits=True, dtype=_lib.LOGITS_F32, mode=_lib.DRAW_SAMPLE, actions=True, fmt=_lib.ACTION_FLAT, offset=0):
    L = _lib.load()
    host = (C.c_uint64 * 8)()  # host memory: never dereferenced, every call below fails before a device is touched
    acts = (C.c_int32 * 4)()
    lp = C.c_void_p(C.addressof(host) + offset) if logits else None
    rc = L.pcbenv_sample_logits(env, lp, dtype, mode, C.cast(acts, C.c_void_p) if actions else None, fmt,
                                None, None, None, 1, 0, 0, None)
    return rc, L.pcbenv_last_error(None).decode()


@pytest.mark.parametrize("kw, msg", [
    ({}, "null handle"),
    ({"logits": False}, "null logits"),
    ({"actions": False}, "null actions"),
    ({"dtype": 2}, "unknown logits dtype"),
    ({"dtype": -1}, "unknown logits dtype"),
    ({"mode": 2}, "unknown draw mode"),
    ({"fmt": 7}, "unknown action format"),
    ({"offset": 1}, "not aligned"),
    ({"offset": 2}, "not aligned"),
    ({"offset": 1, "dtype": _lib.LOGITS_BF16}, "not aligned"),
    ({"offset": 2, "dtype": _lib.LOGITS_BF16}, "null handle"),  # 2-byte alignment is enough for bf16
    ({"mode": _lib.DRAW_GREEDY, "fmt": _lib.ACTION_TUPLE}, "null handle"),
])
def test_argument_checks_need_no_device(kw, msg):
    rc, err = _call(**kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err


def _random_legal(rng, O, H, W, p):
    bits = np.zeros((2, H, (W + 63) // 64), np.uint64)
    cells = rng.rand(2, H, W) < p
    for pl in range(2):
        for x in range(H):
            for y in np.flatnonzero(cells[pl, x]):
                bits[pl, x, y // 64] |= np.uint64(1) << np.uint64(y % 64)
    return bits, cells


@pytest.mark.parametrize("O, H, W", [(1, 8, 8), (2, 6, 6), (4, 10, 10), (4, 16, 64), (4, 5, 128)])
def test_restatement_constant_logits_is_the_uniform_pick(O, H, W):
    rng = np.random.RandomState(O * 1000 + H + W)
    for trial in range(40):
        bits, cells = _random_legal(rng, O, H, W, rng.choice([0.02, 0.3, 1.0]))
        legal = sc.legal_flat(bits, O, H, W)
        want = np.concatenate([cells[o & 1].reshape(-1) for o in range(O)]) if O > 1 else cells[0].reshape(-1)
        assert np.array_equal(legal, want)
        if not legal.any():
            continue
        const = np.full(O * H * W, rng.choice([0.0, 3.25, -7.5]))
        for step in range(5):
            h = sc.hi32(11, trial, step)
            a = sc.draw(const, legal, h / 2.0 ** 32)
            assert a == sc.uniform_pick(legal, h)
            lo, hi = sc.prefix_interval(const, legal, a)
            assert lo <= h / 2.0 ** 32 < hi
        n = int(legal.sum())
        assert sc.log_prob(const, legal, int(np.flatnonzero(legal)[0])) == pytest.approx(-np.log(n), rel=1e-12)
        assert sc.entropy(const, legal) == pytest.approx(np.log(n), rel=1e-12)


def test_restatement_greedy_takes_the_first_index_on_ties():
    legal = np.array([False, True, True, True, False, True])
    l = np.array([9.0, 1.0, 2.0, 2.0, 5.0, 2.0])
    assert sc.greedy(l, legal) == 2
    assert sc.greedy(np.zeros(6), legal) == 1
    assert sc.greedy(np.array([np.nan, -np.inf, -1.0, -np.inf, 0.0, -1.0]), legal) == 2


def test_restatement_hash_matches_the_sampler_definition():
    # the same constants test_sampler_definition restates: seed 5, global env 1000, step 3
    M = (1 << 64) - 1
    z = sc.mix64((sc.mix64((5 ^ ((0x9E3779B97F4A7C15 * 1001) & M)) & M) + 3) & M)
    assert sc.hi32(5, 1000, 3) == z >> 32
