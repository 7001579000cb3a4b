"""pcbenv_gather_paths on the CPU side: the header declares the function and its request with exactly the fields of the
contract, libpcbenv.so exports it, pcbenv/_lib.py binds it, the stream travels in the request, and every argument check
refuses what it must before anything touches a device -- in the order the header gives, the null handle behind the
request's own fields.  (The last check of that order, two handles of different definitions or devices, needs two handles
and so a device: tests/test_gather_paths_gpu.py makes it.)  No compute call is made."""
import ctypes as C
import re

import pytest

from abi_header import raw as _raw, structs as _structs, text as _text
from pcbenv import _lib
FIELDS = [("uint32_t", "struct_size"), ("int32_t", "action_format"), ("const pcbenv *", "src"), ("const int32_t *", "src_index_dev"),
          ("const int32_t *", "path_actions_dev"), ("const int32_t *", "path_len_dev"), ("int32_t", "path_steps"),
          ("int32_t *", "length_dev"), ("uint32_t *", "errors_dev"), ("void *", "stream")]


def test_header_declares_the_function_the_struct_and_the_contract():
    raw, text = _raw(), _text()
    assert re.search(r"\bint\s+pcbenv_gather_paths\s*\(\s*pcbenv\s*\*\s*dst\s*,\s*const\s+pcbenv_gather_paths_request\s*\*\s*req\s*\)\s*;", text)
    assert "pcbenv_gather_paths_request" in _structs(), "the request struct is not declared"
    fields = _structs()["pcbenv_gather_paths_request"]
    norm = lambda t: re.sub(r"\s*\*\s*", " *", t).strip()
    assert [(norm(t), n) for t, n in fields] == [(norm(t), n) for t, n in FIELDS], fields
    assert re.search(r"#define\s+PCBENV_ABI_VERSION\s+3\b", text)  # an addition: the version stays
    # the comment block in front of the struct states the contract
    block = raw[:raw.index("typedef struct pcbenv_gather_paths_request")].rsplit("/*", 1)[1]
    for phrase in ("ONE kernel", "The identity", "pcbenv_gather(dst, src, src_index)", "ALONE", "without PCBENV_FLAG_AUTO_RESET",
                   "first one that", "written whole", "last transition applied", "the source row's", "length_dev[i]",
                   "path_steps == 0: the call is pcbenv_gather, bit for bit", "worst-case", "no done latch", "never resets",
                   "never consumes an instance", "src_index[i] == -1", "bit 0", "bit 1 (value 2)", "before it addresses",
                   "Enqueue-only", "no host synchronisation", "hipGraph", "works in place",
                   "PCBENV_EINVAL (checked before any device call, in this order)", "PCBENV_ESTATE"):
        assert phrase in block, phrase
    assert re.search(r"pcbenv_gather_paths\s+copy\.deepcopy\(env\) followed by env\.step\(a\)", raw.split("#ifndef PCBENV_H")[0])


def test_the_stream_is_a_field_not_a_parameter():
    decl = re.search(r"\bpcbenv_gather_paths\s*\(([^;{]*)\)\s*;", _text()).group(1)
    assert not re.search(r"\bstream\b", decl)
    # ... and the "Streams" paragraph says so behind the pcbenv_set_option sentence, not in the two lists before it
    raw = _raw()
    para = re.sub(r"\s*\n \*\s*", " ", raw[raw.index(" * Streams."):raw.index("What each entry point replaces")])
    assert "pcbenv_gather_paths" not in para[:para.index("pcbenv_set_option")]
    tail = para[para.index("pcbenv_set_option"):]
    assert "pcbenv_gather_paths takes its stream as a field of its request" in tail
    assert tail.index("pcbenv_tree_advance") < tail.index("pcbenv_gather_paths")


def test_exported_and_bound():
    L = _lib.load()
    assert "pcbenv_gather_paths" in _lib.EXPORTS and hasattr(L, "pcbenv_gather_paths")
    assert L.pcbenv_gather_paths.argtypes == [C.c_void_p, C.POINTER(_lib.PcbenvGatherPathsRequest)]
    R = _lib.PcbenvGatherPathsRequest
    assert [n for n, _ in R._fields_] == [n for _, n in FIELDS]
    # the layout a C compiler gives the struct on this ABI: 4 + 4, four pointers, 4 + 4 padding, three pointers
    assert C.sizeof(R) == 72 and R.path_steps.offset == 40 and R.length_dev.offset == 48 and R.stream.offset == 64
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3


_HOST = (C.c_uint64 * 8)()  # host memory: never dereferenced, every call below fails before a device is touched


def _call(request=True, size=None, fmt=_lib.ACTION_TUPLE, path_steps=2, actions=True, index=True):
    L = _lib.load()
    R = _lib.PcbenvGatherPathsRequest
    p = lambda present: C.addressof(_HOST) if present else None
    req = R(struct_size=C.sizeof(R) if size is None else size, action_format=fmt, src=None, src_index_dev=p(index),
            path_actions_dev=p(actions), path_len_dev=None, path_steps=path_steps, length_dev=None, errors_dev=None, stream=None)
    rc = L.pcbenv_gather_paths(None, C.byref(req) if request else None)
    return rc, L.pcbenv_last_error(None).decode()


@pytest.mark.parametrize("kw, msg", [
    ({"request": False}, "null request"),
    ({"size": 0}, "struct_size"),
    ({"size": 64, "fmt": 9, "path_steps": -1, "actions": False, "index": False}, "struct_size"),  # the order: the size first
    ({"size": 80}, "struct_size"),
    ({"fmt": 2}, "unknown action format"),
    ({"fmt": -1, "path_steps": -1, "actions": False, "index": False}, "unknown action format"),  # ... then the format
    ({"path_steps": -1}, "path_steps must not be negative"),
    ({"path_steps": -5, "actions": False, "index": False}, "path_steps must not be negative"),
    ({"actions": False}, "null path_actions"),
    ({"actions": False, "index": False}, "null path_actions"),
    ({"index": False}, "null src_index"),
    ({"index": False, "path_steps": 0, "actions": False}, "null src_index"),
    ({}, "null handle"),
    ({"fmt": _lib.ACTION_FLAT, "path_steps": 0, "actions": False}, "null handle"),  # no path at all: null path_actions with path_steps == 0
    ({"path_steps": 0}, "null handle"),
])
def test_argument_checks_need_no_device(kw, msg):
    rc, err = _call(**kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
