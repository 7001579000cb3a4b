"""pcbenv_playout_paths on the CPU side: the header declares it and its request struct and states the contract,
libpcbenv.so exports it, pcbenv/_lib.py binds it, and every argument check refuses what it must before anything touches a
device -- in the order the header gives, the null handle last.  No compute call is made."""
import ctypes as C
import re

import pytest

from abi_header import raw as _raw, structs as _structs, text as _text
from pcbenv import _lib

FIELDS = [("uint32_t", "struct_size"), ("int32_t", "action_format"), ("const int32_t *", "root_index_dev"), ("int64_t", "num_playouts"),
          ("const int32_t *", "path_actions_dev"), ("const int32_t *", "path_len_dev"), ("int32_t", "path_steps"), ("int32_t", "max_steps"),
          ("double *", "reward_dev"), ("uint8_t *", "done_dev"), ("int32_t *", "length_dev"), ("double *", "info_dev"),
          ("int32_t *", "actions_out_dev"), ("int32_t", "actions_steps"), ("uint64_t *", "leaf_mask_bits_dev"), ("uint32_t *", "errors_dev"),
          ("uint64_t", "seed"), ("uint64_t", "first_env_index"), ("uint64_t", "step_index0"), ("void *", "stream")]
CTYPES = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}


def test_header_declares_the_function_the_struct_and_the_contract():
    raw = _raw()
    text = _text()
    assert re.search(r"\bint\s+pcbenv_playout_paths\s*\(\s*const\s+pcbenv\s*\*\s*env\s*,\s*const\s+pcbenv_playout_request\s*\*\s*req\s*\)\s*;", text)
    assert _structs()["pcbenv_playout_request"] == FIELDS
    assert re.search(r"#define\s+PCBENV_ABI_VERSION\s+3\b", text)  # an addition: the version stays
    assert raw.index("int pcbenv_playout(") < raw.index("int pcbenv_playout_paths(")  # the old declaration comes first
    top = raw.split("#ifndef PCBENV_H")[0]
    assert re.search(r"pcbenv_playout_paths\s+copy\.deepcopy\(env\), env\.step\(a\) for every action of the path.*?simulate\(\)", top, flags=re.S)
    # its stream class: a sentence of its own at the end of the Streams paragraph, behind the pcbenv_set_option sentence
    para = re.sub(r"\s*\n \*\s*", " ", top[top.index(" * Streams."):top.index("What each entry point replaces")])
    assert para.index("pcbenv_set_option") < para.index("pcbenv_playout_paths") and "only enqueues" in para[para.index("pcbenv_playout_paths"):]
    block = raw[:raw.index("typedef struct pcbenv_playout_request")].rsplit("/*", 1)[1]
    for phrase in ("The identity", "t < path_len[i]", "(seed, first_env_index + i, step_index0 + t)", "bit for bit",
                   "The draw key depends on t, not on the path", "path_steps == 1 equals pcbenv_playout", "for every d",
                   "A bad path action is data", "worst-case", "not read for effect", "recorded as given", "untouched",
                   "leaf_mask_bits_dev", "min(path_len[i], length[i]) - 1", "the root's own", "columns >= W", "plane 1 of the square kind",
                   "unspecified", "pcbenv_evaluate_logits / pcbenv_evaluate_axis", "bit 1 (value 2)", "still sets bit 0", "all-zero leaf mask",
                   "length = 0", "Writes nothing the library owns", "PCBENV_FLAG_AUTO_RESET is ignored", "hipGraph",
                   "PCBENV_EINVAL (checked before any device call, in this order)", "num_playouts == 0 is a no-op success", "PCBENV_ESTATE"):
        assert phrase in block, phrase


def test_exported_and_bound():
    L = _lib.load()
    assert "pcbenv_playout_paths" in _lib.EXPORTS and hasattr(L, "pcbenv_playout_paths")
    assert len(L.pcbenv_playout_paths.argtypes) == 2
    R = _lib.PcbenvPlayoutRequest
    assert [n for n, _ in R._fields_] == [n for _, n in FIELDS]
    for (n, t), (ct, _) in zip(R._fields_, FIELDS):
        assert t is (C.c_void_p if ct.endswith("*") else CTYPES[ct]), n
    assert C.sizeof(R) == 144 and R.stream.offset == 136  # no padding surprises: 8-byte members on 8-byte offsets
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3


_HOST = (C.c_uint64 * 8)()  # host memory: never dereferenced, every call below fails before a device is touched


def _call(request=True, size=None, reward=True, fmt=_lib.ACTION_TUPLE, max_steps=4, path_steps=0, paths=False, actions_steps=0,
          actions=False, leaf=0, n=8, index=True):
    L = _lib.load()
    p = lambda present: C.addressof(_HOST) if present else None
    R = _lib.PcbenvPlayoutRequest
    req = R(struct_size=C.sizeof(R) if size is None else size, action_format=fmt, root_index_dev=p(index), num_playouts=n,
            path_actions_dev=p(paths), path_steps=path_steps, max_steps=max_steps, reward_dev=p(reward), actions_out_dev=p(actions),
            actions_steps=actions_steps, leaf_mask_bits_dev=(C.addressof(_HOST) + leaf) if leaf else None, seed=1)
    rc = L.pcbenv_playout_paths(None, C.byref(req) if request else None)
    return rc, L.pcbenv_last_error(None).decode()


@pytest.mark.parametrize("kw, msg", [
    ({"request": False}, "null request"),
    ({"size": 0}, "struct_size"),
    ({"size": 140, "reward": False}, "struct_size"),                      # the order: the size before any field is believed
    ({"size": 152, "fmt": 9}, "struct_size"),
    ({"reward": False}, "null reward"),
    ({"reward": False, "fmt": 7, "max_steps": 0}, "null reward"),
    ({"fmt": 2}, "unknown action format"),
    ({"fmt": -1, "max_steps": 0}, "unknown action format"),
    ({"max_steps": 0}, "max_steps must be"),
    ({"max_steps": -3, "path_steps": -1}, "max_steps must be"),
    ({"path_steps": -1}, "path_steps must be in"),
    ({"path_steps": 5, "paths": True}, "path_steps must be in"),
    ({"path_steps": 5, "actions_steps": -1}, "path_steps must be in"),
    ({"path_steps": 2}, "null path_actions"),
    ({"path_steps": 2, "actions_steps": 9}, "null path_actions"),
    ({"actions_steps": -1}, "actions_steps must be in"),
    ({"actions_steps": 5, "actions": True}, "actions_steps must be in"),
    ({"actions_steps": 2}, "null actions_out"),
    ({"actions_steps": 2, "leaf": 4}, "null actions_out"),
    ({"leaf": 4}, "leaf_mask_bits must be 8-byte aligned"),
    ({"leaf": 1, "n": -1}, "leaf_mask_bits must be 8-byte aligned"),
    ({"n": -1}, "num_playouts"),
    ({"n": -1, "index": False}, "num_playouts"),
    ({}, "null handle"),
    ({"path_steps": 4, "paths": True, "actions_steps": 4, "actions": True, "leaf": 8}, "null handle"),
    ({"fmt": _lib.ACTION_FLAT, "index": False}, "null handle"),          # (the multiple-of-num_envs check needs a handle)
    ({"n": 0}, "null handle"),                                            # the null handle is refused before the no-op
])
def test_argument_checks_need_no_device(kw, msg):
    rc, err = _call(**kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
