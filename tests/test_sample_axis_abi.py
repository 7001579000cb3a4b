"""pcbenv_sample_axis / pcbenv_evaluate_axis / pcbenv_evaluate_axis_backward on the CPU side: the header declares them
with the axis enum, libpcbenv.so exports them, pcbenv/_lib.py binds them, and every argument check refuses what it must
before anything touches a device.  No compute call is made."""
import ctypes as C
import re

import pytest

from abi_header import raw as _raw, text as _header
from pcbenv import _lib


def _sig(ret, name, params):
    """A regex for `ret name(params);` with free whitespace; params are written as in the header."""
    def one(p):
        toks, out = re.findall(r"\w+|\*", p), ""
        for i, t in enumerate(toks):
            if i:
                out += r"\s*" if "*" in (t, toks[i - 1]) else r"\s+"
            out += re.escape(t)
        return out
    return r"\b" + ret + r"\s+" + name + r"\s*\(\s*" + r"\s*,\s*".join(one(p) for p in params) + r"\s*\)\s*;"


def test_header_declares_signatures_and_enum():
    text = _header()
    assert re.search(_sig("int", "pcbenv_sample_axis", [
        "pcbenv *env", "int32_t axis", "uint32_t given", "const void *logits_dev", "int32_t logits_dtype", "int32_t mode",
        "int32_t *actions_dev", "float *log_prob_dev", "float *entropy_dev", "uint32_t *errors_dev", "uint64_t seed",
        "uint64_t first_env_index", "uint64_t step_index", "void *stream"]), text)
    assert re.search(_sig("int", "pcbenv_evaluate_axis", [
        "const pcbenv *env", "int32_t axis", "uint32_t given", "const void *logits_dev", "int32_t logits_dtype",
        "const uint64_t *mask_bits_dev", "const int32_t *actions_dev", "int64_t num_rows", "float *log_prob_dev",
        "float *entropy_dev", "uint32_t *errors_dev", "void *stream"]), text)
    assert re.search(_sig("int", "pcbenv_evaluate_axis_backward", [
        "const pcbenv *env", "int32_t axis", "uint32_t given", "const void *logits_dev", "int32_t logits_dtype",
        "const uint64_t *mask_bits_dev", "const int32_t *actions_dev", "int64_t num_rows", "const float *grad_log_prob_dev",
        "const float *grad_entropy_dev", "void *grad_logits_dev", "void *stream"]), text)
    assert re.search(r"enum\s+pcbenv_axis\s*\{\s*PCBENV_AXIS_ORIENTATION\s*=\s*0\s*,\s*PCBENV_AXIS_X\s*=\s*1\s*,\s*PCBENV_AXIS_Y\s*=\s*2\s*\}", text)
    assert (_lib.AXIS_ORIENTATION, _lib.AXIS_X, _lib.AXIS_Y) == (0, 1, 2)
    assert re.search(r"#define\s+PCBENV_ABI_VERSION\s+3\b", text)
    # the "what each entry point replaces" block names the reference's lines
    assert re.search(r"pcbenv_sample_axis.*?factorized_action_distributions\.py:107-818",
                     _raw().split("#ifndef PCBENV_H")[0], flags=re.S)


def test_exported_and_bound():
    L = _lib.load()
    for name, nargs in (("pcbenv_sample_axis", 14), ("pcbenv_evaluate_axis", 12), ("pcbenv_evaluate_axis_backward", 12)):
        assert name in _lib.EXPORTS
        assert hasattr(L, name)
        assert len(getattr(L, name).argtypes) == nargs
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3  # additions: the ABI version stays


_HOST = (C.c_uint64 * 8)()  # host memory: never dereferenced, every call below fails before a device is touched
_ACTS = (C.c_int32 * 6)()


def _ptr(base, present=True, offset=0):
    return C.c_void_p(C.addressof(base) + offset) if present else None


def _sample(axis=0, given=0, logits=True, dtype=_lib.LOGITS_F32, mode=_lib.DRAW_SAMPLE, actions=True, offset=0):
    L = _lib.load()
    rc = L.pcbenv_sample_axis(None, axis, given, _ptr(_HOST, logits, offset), dtype, mode, _ptr(_ACTS, actions),
                              None, None, None, 1, 0, 0, None)
    return rc, L.pcbenv_last_error(None).decode()


def _evaluate(backward, axis=0, given=0, logits=True, dtype=_lib.LOGITS_F32, actions=True, offset=0, bits=True, bits_offset=0,
              rows=1, grad=True, grad_offset=0):
    L = _lib.load()
    if backward:
        rc = L.pcbenv_evaluate_axis_backward(None, axis, given, _ptr(_HOST, logits, offset), dtype, _ptr(_HOST, bits, bits_offset),
                                             _ptr(_ACTS, actions), rows, None, None, _ptr(_HOST, grad, grad_offset), None)
    else:
        rc = L.pcbenv_evaluate_axis(None, axis, given, _ptr(_HOST, logits, offset), dtype, _ptr(_HOST, bits, bits_offset),
                                    _ptr(_ACTS, actions), rows, None, None, None, None)
    return rc, L.pcbenv_last_error(None).decode()


COMMON = [
    ({}, "null handle"),
    ({"logits": False}, "null logits"),
    ({"actions": False}, "null actions"),
    ({"dtype": 2}, "unknown logits dtype"),
    ({"dtype": -1}, "unknown logits dtype"),
    ({"axis": 3}, "unknown axis"),
    ({"axis": -1}, "unknown axis"),
    ({"axis": 1, "given": 2}, "given contains the axis"),
    ({"axis": 0, "given": 7}, "given contains the axis"),
    ({"axis": 2, "given": 8}, "bit above 4"),
    ({"axis": 2, "given": 1 << 31}, "bit above 4"),
    ({"offset": 1}, "not aligned"),
    ({"offset": 2}, "not aligned"),
    ({"offset": 1, "dtype": _lib.LOGITS_BF16}, "not aligned"),
    ({"offset": 2, "dtype": _lib.LOGITS_BF16}, "null handle"),  # 2-byte alignment is enough for bf16
    ({"axis": 2, "given": 3}, "null handle"),
    ({"axis": 0, "given": 6}, "null handle"),
    ({"axis": 1, "given": 5}, "null handle"),
]


@pytest.mark.parametrize("kw, msg", COMMON + [
    ({"mode": 2}, "unknown draw mode"),
    ({"mode": -1}, "unknown draw mode"),
    ({"mode": _lib.DRAW_GREEDY, "axis": 1, "given": 1}, "null handle"),
])
def test_sampler_argument_checks_need_no_device(kw, msg):
    rc, err = _sample(**kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err


EVAL = COMMON + [
    ({"bits": False}, "null mask bits"),
    ({"bits_offset": 4}, "mask bits pointer not aligned"),
    ({"rows": -1}, "num_rows"),
    ({"rows": 0}, "null handle"),  # the null handle is refused before the no-op
]


@pytest.mark.parametrize("kw, msg", EVAL)
def test_evaluate_argument_checks_need_no_device(kw, msg):
    rc, err = _evaluate(False, **kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err


@pytest.mark.parametrize("kw, msg", EVAL + [
    ({"grad": False}, "null grad logits"),
    ({"grad_offset": 2}, "grad logits pointer not aligned"),
    ({"grad_offset": 2, "dtype": _lib.LOGITS_BF16}, "null handle"),
])
def test_backward_argument_checks_need_no_device(kw, msg):
    rc, err = _evaluate(True, **kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
