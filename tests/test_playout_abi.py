"""pcbenv_playout on the CPU side: the header declares it and states its contract, libpcbenv.so exports it,
pcbenv/_lib.py binds it, and every argument check refuses what it must before anything touches a device -- in the order
the header gives, the null handle last.  No compute call is made."""
import ctypes as C
import re

import pytest

from abi_header import raw as _raw, text as _text
from pcbenv import _lib

PARAMS = ["const pcbenv *env", "const int32_t *root_index_dev", "int64_t num_playouts", "const int32_t *first_actions_dev",
          "int32_t action_format", "int32_t max_steps", "double *reward_dev", "uint8_t *done_dev", "int32_t *length_dev",
          "double *info_dev", "int32_t *actions_out_dev", "int32_t actions_steps", "uint32_t *errors_dev", "uint64_t seed",
          "uint64_t first_env_index", "uint64_t step_index0", "void *stream"]


def _sig(ret, name, params):
    def one(p):
        toks, out = re.findall(r"\w+|\*", p), ""
        for i, t in enumerate(toks):
            if i:
                out += r"\s*" if "*" in (t, toks[i - 1]) else r"\s+"
            out += re.escape(t)
        return out
    return r"\b" + ret + r"\s+" + name + r"\s*\(\s*" + r"\s*,\s*".join(one(p) for p in params) + r"\s*\)\s*;"


def test_header_declares_the_signature_and_the_contract():
    raw = _raw()
    text = _text()
    assert re.search(_sig("int", "pcbenv_playout", PARAMS), text)
    assert re.search(r"#define\s+PCBENV_ABI_VERSION\s+3\b", text)  # an addition: the version stays
    # the "what each entry point replaces" block names the reference's lines
    assert re.search(r"pcbenv_playout\s+copy\.deepcopy\(env\).*?random_policy_square\.py:25-58", raw.split("#ifndef PCBENV_H")[0], flags=re.S)
    # the comment block in front of the declaration states the contract
    block = raw[:raw.index("int pcbenv_playout(")].rsplit("/*", 1)[1]
    for phrase in ("The identity", "pcbenv_step_sampled(seed, first_env_index, step_index0 + t)", "pcbenv_gather", "bit for",
                   "root_index_dev", "first_actions_dev", "worst-case", "reward_dev[i]", "Not a sum", "done_dev[i]", "length_dev[i]",
                   "info_dev[i, 2]", "actions_out_dev", "untouched", "length = 0", "Writes nothing the library owns",
                   "PCBENV_FLAG_AUTO_RESET is ignored", "PCBENV_EINVAL (checked before any device call, in this order)",
                   "num_playouts == 0 is a no-op success", "PCBENV_ESTATE", "hipGraph"):
        assert phrase in block, phrase


def test_exported_and_bound():
    L = _lib.load()
    assert "pcbenv_playout" in _lib.EXPORTS and hasattr(L, "pcbenv_playout")
    assert len(L.pcbenv_playout.argtypes) == len(PARAMS) == 17
    assert L.pcbenv_playout.argtypes[2] is C.c_int64 and L.pcbenv_playout.argtypes[13:16] == [C.c_uint64] * 3
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3


_HOST = (C.c_uint64 * 8)()  # host memory: never dereferenced, every call below fails before a device is touched


def _call(reward=True, fmt=_lib.ACTION_TUPLE, max_steps=4, actions_steps=0, actions=False, n=8, index=True):
    L = _lib.load()
    p = lambda present: C.c_void_p(C.addressof(_HOST)) if present else None
    rc = L.pcbenv_playout(None, p(index), n, None, fmt, max_steps, p(reward), None, None, None, p(actions), actions_steps, None,
                          1, 0, 0, None)
    return rc, L.pcbenv_last_error(None).decode()


@pytest.mark.parametrize("kw, msg", [
    ({"reward": False}, "null reward"),
    ({"reward": False, "fmt": 7, "max_steps": 0}, "null reward"),          # the order: reward first
    ({"fmt": 2}, "unknown action format"),
    ({"fmt": -1, "max_steps": 0}, "unknown action format"),              # ... then the format
    ({"max_steps": 0}, "max_steps"),
    ({"max_steps": -3, "actions_steps": -1}, "max_steps"),
    ({"actions_steps": -1}, "actions_steps must be in"),
    ({"actions_steps": 5, "actions": True}, "actions_steps must be in"),
    ({"actions_steps": 2}, "null actions_out"),
    ({"actions_steps": 2, "n": -1}, "null actions_out"),
    ({"n": -1}, "num_playouts"),
    ({"n": -1, "index": False}, "num_playouts"),
    ({}, "null handle"),
    ({"actions_steps": 4, "actions": True}, "null handle"),
    ({"fmt": _lib.ACTION_FLAT, "index": False}, "null handle"),          # (the multiple-of-num_envs check needs a handle)
    ({"n": 0}, "null handle"),                                            # the null handle is refused before the no-op
])
def test_argument_checks_need_no_device(kw, msg):
    rc, err = _call(**kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
