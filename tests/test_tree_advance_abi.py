"""pcbenv_tree_advance on the CPU side: the header declares it, its request struct and its contract, libpcbenv.so exports
it, pcbenv/_lib.py binds it with a structure of the C struct's size, and every argument check refuses what it must before
anything touches a device -- in the order the header gives, the null handle last.  No compute call is made."""
import ctypes as C
import re
import shutil

import pytest

from abi_header import REPO, raw as _raw, structs as _structs, text as _text
import model_harness
from pcbenv import _lib

POINTERS = ("ln_dev",) + _lib.TREE_TENSORS + ("selected", "path_len", "paths", "reward", "length", "actions", "errors_dev", "stream")
MEMBERS = ("struct_size", "phases", "num_roots", "capacity", "max_children", "max_steps", "c_uct") + POINTERS


def test_header_declares_the_function_the_struct_and_the_contract():
    raw = _raw()
    text = _text()
    assert re.search(r"\bint\s+pcbenv_tree_advance\s*\(\s*const\s+pcbenv\s*\*\s*env\s*,\s*const\s+pcbenv_tree_request\s*\*\s*req\s*\)\s*;", text)
    names = [n for _, n in _structs()["pcbenv_tree_request"]]
    assert tuple(names) == MEMBERS
    for name, value in (("PCBENV_TREE_INIT", 1), ("PCBENV_TREE_ABSORB", 2), ("PCBENV_TREE_SELECT", 4), ("PCBENV_MAX_TREE_CHILDREN", 64)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name
    assert (_lib.TREE_INIT, _lib.TREE_ABSORB, _lib.TREE_SELECT, _lib.MAX_TREE_CHILDREN) == (1, 2, 4, 64)
    assert re.search(r"#define\s+PCBENV_ABI_VERSION\s+3\b", text)  # an addition: the version stays
    assert not re.search(r"pcbenv_tree_advance\s*\([^;]*\bstream\b", text)  # the stream travels in the request
    top = raw.split("#ifndef PCBENV_H")[0]
    assert re.search(r"pcbenv_tree_advance\s+no counterpart", top)
    para = re.sub(r"\s*\n \*\s*", " ", top[top.index(" * Streams."):top.index("What each entry point replaces")])
    assert para.index("pcbenv_playout_paths") < para.index("pcbenv_tree_advance") and "only enqueues" in para[para.index("pcbenv_tree_advance"):]
    block = re.sub(r"\s*\n \*\s*", " ", raw[:raw.index("#define PCBENV_TREE_INIT")].rsplit("/*", 1)[1])
    for phrase in ("one kernel launch on req->stream", "nothing the library owns is read or written", "no bound buffers",
                   "Enqueue only, no allocation, no synchronisation", "hipGraph", "in the order INIT, ABSORB, SELECT",
                   "ties go to the lowest child slot", "ln_dev[min(n, N)]", "never computes a logarithm", "path_len[p] = depth(selected)",
                   "are untouched", "At most max_steps levels", "drew = length > depth(node) && !terminal(node)", "the first such child",
                   "num_nodes < N", "bit 0 (value 1)", "bit 1 (value 2)", "for t < length", "best_actions is not written",
                   "PCBENV_EINVAL (checked before any device call, in this order)", "num_roots == 0 is a no-op success"):
        assert phrase in block, phrase


def test_exported_and_bound():
    L = _lib.load()
    assert "pcbenv_tree_advance" in _lib.EXPORTS and hasattr(L, "pcbenv_tree_advance")
    assert len(L.pcbenv_tree_advance.argtypes) == 2
    R = _lib.PcbenvTreeRequest
    assert tuple(n for n, _ in R._fields_) == MEMBERS
    kinds = dict(struct_size=C.c_uint32, c_uct=C.c_double, **{n: C.c_void_p for n in POINTERS})
    for n, t in R._fields_:
        assert t is kinds.get(n, C.c_int32), n
    # csrc/pcb_tree.hip static_asserts the same two figures of the struct as the library compiled it
    assert C.sizeof(R) == 224 and R.stream.offset == 216 and R.c_uct.offset == 24
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_ctypes_structure_has_the_c_layout():
    """A compiled probe: sizeof and every member's offset as a C compiler lays include/pcbenv.h out."""
    offsets, size = model_harness.layout("pcbenv.h", "pcbenv_tree_request", MEMBERS)
    R = _lib.PcbenvTreeRequest
    assert size == C.sizeof(R)
    assert offsets == {n: getattr(R, n).offset for n in MEMBERS}


_HOST = (C.c_uint64 * 8)()  # host memory: never dereferenced, every call below fails before a device is touched
TREE = ("num_nodes", "parent", "depth", "visits", "num_children", "node_action", "children", "value_sum", "value_max", "terminal",
        "reward_lo", "reward_hi")


def _call(request=True, size=None, phases=_lib.TREE_ABSORB | _lib.TREE_SELECT, P=8, N=5, Cc=3, T=4, null=(), odd=()):
    L = _lib.load()
    R = _lib.PcbenvTreeRequest
    req = R(struct_size=C.sizeof(R) if size is None else size, phases=phases, num_roots=P, capacity=N, max_children=Cc, max_steps=T, c_uct=1.0)
    for n in POINTERS[:-2]:  # errors_dev and stream stay null: both are optional
        if n not in null:
            setattr(req, n, C.addressof(_HOST) + (4 if n in odd else 0))
    rc = L.pcbenv_tree_advance(None, C.byref(req) if request else None)
    return rc, L.pcbenv_last_error(None).decode()


I, A, S = _lib.TREE_INIT, _lib.TREE_ABSORB, _lib.TREE_SELECT


@pytest.mark.parametrize("kw, msg", [
    ({"request": False}, "null request"),
    ({"size": 0}, "struct_size"),
    ({"size": 216, "phases": 0}, "struct_size"),                            # the order: the size before any field is believed
    ({"size": 232, "P": -1}, "struct_size"),
    ({"phases": 0}, "phases must be"),
    ({"phases": 8, "P": -1}, "phases must be"),
    ({"phases": 15}, "phases must be"),
    ({"phases": -1}, "phases must be"),
    ({"phases": I | A}, "INIT cannot be combined with ABSORB"),
    ({"phases": I | A | S, "N": 0}, "INIT cannot be combined with ABSORB"),
    ({"P": -1}, "num_roots"),
    ({"P": -1, "N": 0}, "num_roots"),
    ({"N": 0}, "capacity"),
    ({"N": -4, "Cc": 0}, "capacity"),
    ({"Cc": 0}, "max_children"),
    ({"Cc": 65, "T": 0}, "max_children"),
    ({"Cc": -1}, "max_children"),
    ({"T": 0}, "max_steps"),
    ({"T": -2, "null": ("parent",)}, "max_steps"),
    *[({"null": (n,), "phases": ph}, "null tree tensor") for n in TREE for ph in (I, A, S)],
    ({"null": ("best_reward",), "phases": I}, "null tree tensor"),
    ({"null": ("best_length",), "phases": A}, "null tree tensor"),
    ({"null": ("best_actions",), "phases": A | S}, "null tree tensor"),
    ({"null": ("best_actions", "selected"), "phases": A}, "null tree tensor"),
    ({"null": ("selected",), "phases": A}, "null selected"),
    ({"null": ("selected", "paths"), "phases": S}, "null selected"),
    ({"null": ("path_len",), "phases": I | S}, "null path_len or paths"),
    ({"null": ("paths", "ln_dev"), "phases": S}, "null path_len or paths"),
    ({"null": ("ln_dev",), "phases": S}, "null ln"),
    ({"null": ("ln_dev", "reward"), "phases": A | S}, "null ln"),
    ({"null": ("reward",), "phases": A}, "null reward, length or actions"),
    ({"null": ("length",), "phases": A | S}, "null reward, length or actions"),
    ({"null": ("actions",), "odd": ("value_sum",), "phases": A}, "null reward, length or actions"),
    *[({"odd": (n,), "phases": ph}, "8-byte aligned") for n in ("ln_dev", "value_sum", "value_max", "reward_lo", "reward_hi", "best_reward", "reward")
      for ph in (A | S,)],
    ({"odd": ("ln_dev",), "phases": I | S}, "8-byte aligned"),
    ({}, "null handle"),
    ({"phases": I}, "null handle"),
    ({"phases": I | S}, "null handle"),
    ({"phases": S, "null": ("best_reward", "best_length", "best_actions", "reward", "length", "actions")}, "null handle"),  # what SELECT does not touch
    ({"phases": I, "null": ("best_actions", "selected", "path_len", "paths", "ln_dev", "reward", "length", "actions")}, "null handle"),
    ({"phases": A, "null": ("path_len", "paths", "ln_dev")}, "null handle"),
    ({"odd": ("parent", "paths", "actions")}, "null handle"),              # int32 tensors need 4 bytes only
    ({"Cc": 64, "N": 1, "T": 1}, "null handle"),
    ({"P": 0}, "null handle"),                                              # the null handle is refused before the no-op
])
def test_argument_checks_need_no_device(kw, msg):
    rc, err = _call(**kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
