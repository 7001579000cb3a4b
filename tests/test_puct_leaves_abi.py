"""pcbenv_puct_advance_leaves on the CPU side: include/pcbenv_leaves.h declares it, its request struct and its contract,
libpcbenv.so exports it, pcbenv/_leaves_lib.py binds it with a structure of the C struct's layout -- next to
include/pcbenv.h, include/pcbenv_search.h and their bindings, which stay as they are -- and every argument check refuses
what it must before anything touches a device, in the order the header gives, the null handle last.  No compute call is
made."""
import ctypes as C
import os
import re
import shutil

import pytest

from abi_header import REPO, _STRUCT, _declarator
import model_harness
from pcbenv import _leaves_lib, _lib, _search_lib

PATH = os.path.join(REPO, "include", "pcbenv_leaves.h")
TREE = _leaves_lib.LEAVES_TREE_TENSORS
INPUTS = _search_lib.PUCT_INPUTS
POINTERS = TREE + ("selected", "path_len", "paths") + INPUTS + ("errors_dev", "stream")
INTS = ("phases", "num_roots", "capacity", "max_children", "max_steps", "num_candidates", "reserved")
MEMBERS = ("struct_size",) + INTS + ("c_puct", "num_leaves", "reserved2") + POINTERS
CTYPES = {"struct_size": "uint32_t", "c_puct": "double", "node_action": "int32_t *", "terminal": "uint8_t *", "value": "const double *",
          "leaf_terminal": "const uint8_t *", "cand_count": "const int32_t *", "cand_actions": "const int32_t *", "cand_prior": "const float *",
          "errors_dev": "uint32_t *", "stream": "void *", "num_leaves": "int32_t", "reserved2": "int32_t",
          **{n: "int32_t" for n in INTS}, **{n: "double *" for n in ("prior", "value_sum", "value_max", "reward_lo", "reward_hi")},
          **{n: "int32_t *" for n in ("num_nodes", "parent", "depth", "visits", "num_children", "first_child", "pending", "selected", "path_len", "paths")}}


def _raw():
    with open(PATH) as f:
        return f.read()


def _text():
    return re.sub(r"/\*.*?\*/", "", _raw(), flags=re.S)


def _members(text, struct):
    (name, body), = re.findall(_STRUCT, text, flags=re.S)
    assert name == struct
    out = []
    for decl in filter(str.strip, body.split(";")):
        base = re.match(r"\s*((?:const\s+)?\w+)", decl)
        out += [_declarator(base.group(1) + " " + item) for item in decl[base.end():].split(",")]
    return out


def test_header_declares_the_function_the_struct_and_the_contract():
    raw, text = _raw(), _text()
    assert re.search(r'#include\s+"pcbenv_search.h"', text) and "PCBENV_ABI_VERSION" not in text  # the version is pcbenv.h's, and stays 3
    assert re.search(r"\bint\s+pcbenv_puct_advance_leaves\s*\(\s*const\s+pcbenv\s*\*\s*env\s*,\s*const\s+pcbenv_puct_leaves_request\s*\*\s*req\s*\)\s*;", text)
    assert len(re.findall(r"\b\w+\s*\([^()]*\)\s*;", text)) == 1  # one prototype
    assert re.search(r"#define\s+PCBENV_MAX_PUCT_LEAVES\s+64\b", text) and _leaves_lib.MAX_PUCT_LEAVES == 64
    members = _members(text, "pcbenv_puct_leaves_request")
    assert tuple(n for _, n in members) == MEMBERS
    assert {n: t for t, n in members} == CTYPES
    # it carries the members of pcbenv_puct_request, in their order
    with open(os.path.join(REPO, "include", "pcbenv_search.h")) as f:
        base = [n for _, n in _members(re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S), "pcbenv_puct_request")]
    assert [n for n in MEMBERS if n in base] == base and set(MEMBERS) - set(base) == {"num_leaves", "reserved2", "pending"}
    assert not re.search(r"#define\s+PCBENV_TREE_", text)  # the phases are pcbenv.h's
    block = re.sub(r"\s*\n \*\s*", " ", raw[:raw.index("typedef struct pcbenv_puct_leaves_request")].rsplit("/*", 1)[1])
    for phrase in ("one kernel launch on req->stream", "nothing the library owns is read or written", "no bound buffers",
                   "Enqueue only, no allocation, no synchronisation", "hipGraph", "in the order INIT, ABSORB, SELECT",
                   "first_child .. first_child + k - 1", "ties go to the lowest c", "No logarithm is computed", "are untouched",
                   "At most max_steps levels", "which is never cleared", "clamp(cand_count, 0, min(K, C))", "all or nothing", "bit 0 (value 1)",
                   "bit 1 (value 2)", "at most max_steps + 1 nodes", "row r = p * L + l", "pending = 0 in every slot",
                   "n_c = (double)(visits(ch) + pending(ch))", "((double)visits(ch) / n_c)",
                   "u = c_puct * prior(ch) * sqrt((double)max(visits(node) + pending(node), 1)) / (1.0 + n_c)",
                   "counts as a visit that returned reward_lo", "is exactly 1.0", "bit for bit", "selected[r] = path_len[r] = -1",
                   "adds no pending visit", "may be selected more than once", "none of that row's inputs is read", "pending -= 1",
                   "pending is zero everywhere", "adds to the pending visits that are there", "the caller pairs", "it never addresses anything",
                   "PCBENV_EINVAL (checked before any device call, in this order)", "num_roots == 0 is a no-op success"):
        assert phrase in block, phrase
    assert "only enqueues" in raw.split("#ifndef PCBENV_LEAVES_H")[0]


def test_exported_and_bound():
    L = _leaves_lib.bind(_lib.load())
    assert _leaves_lib.EXPORTS == ("pcbenv_puct_advance_leaves",) and hasattr(L, "pcbenv_puct_advance_leaves")
    assert len(L.pcbenv_puct_advance_leaves.argtypes) == 2 and L.pcbenv_puct_advance_leaves.restype is C.c_int
    assert "pcbenv_puct_advance_leaves" not in _lib.EXPORTS and "pcbenv_puct_advance_leaves" not in _search_lib.EXPORTS
    R = _leaves_lib.PcbenvPuctLeavesRequest
    assert tuple(n for n, _ in R._fields_) == MEMBERS
    kinds = dict(struct_size=C.c_uint32, c_puct=C.c_double, **{n: C.c_void_p for n in POINTERS})
    for n, t in R._fields_:
        assert t is kinds.get(n, C.c_int32), n
    # csrc/pcb_puct_leaves.hip static_asserts the same figures of the struct as the library compiled it
    assert C.sizeof(R) == 240 and R.stream.offset == 232 and R.num_leaves.offset == 40 and R.c_puct.offset == 32
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_ctypes_structure_has_the_c_layout():
    """A compiled probe: sizeof and every member's offset as a C compiler lays include/pcbenv_leaves.h out."""
    offsets, size = model_harness.layout("pcbenv_leaves.h", "pcbenv_puct_leaves_request", MEMBERS)
    R = _leaves_lib.PcbenvPuctLeavesRequest
    assert size == C.sizeof(R)
    assert offsets == {n: getattr(R, n).offset for n in MEMBERS}


_HOST = (C.c_uint64 * 8)()  # host memory: never dereferenced, every call below fails before a device is touched


def _call(request=True, size=None, phases=_lib.TREE_ABSORB | _lib.TREE_SELECT, P=8, N=5, Cc=3, T=4, K=2, Lv=4, reserved=0, reserved2=0, null=(), odd=(),
          odd2=()):
    L = _leaves_lib.bind(_lib.load())
    R = _leaves_lib.PcbenvPuctLeavesRequest
    req = R(struct_size=C.sizeof(R) if size is None else size, phases=phases, num_roots=P, capacity=N, max_children=Cc, max_steps=T,
            num_candidates=K, reserved=reserved, c_puct=1.0, num_leaves=Lv, reserved2=reserved2)
    for n in POINTERS[:-2]:  # errors_dev and stream stay null: both are optional
        if n not in null:
            setattr(req, n, C.addressof(_HOST) + (4 if n in odd else 2 if n in odd2 else 0))
    rc = L.pcbenv_puct_advance_leaves(None, C.byref(req) if request else None)
    return rc, L.pcbenv_last_error(None).decode()


I, A, S = _lib.TREE_INIT, _lib.TREE_ABSORB, _lib.TREE_SELECT
DOUBLES = ("prior", "value_sum", "value_max", "reward_lo", "reward_hi")


@pytest.mark.parametrize("kw, msg", [
    ({"request": False}, "null request"),                                   # 1
    ({"size": 0}, "struct_size"),                                           # 2
    ({"size": 224, "phases": 0}, "struct_size"),                            # pcbenv_puct_request's size is not this struct's
    ({"size": 248, "P": -1}, "struct_size"),
    ({"phases": 0}, "phases must be"),                                      # 3
    ({"phases": 8, "P": -1}, "phases must be"),
    ({"phases": -1}, "phases must be"),
    ({"phases": I | A}, "INIT cannot be combined with ABSORB"),
    ({"phases": I | A | S, "P": -1}, "INIT cannot be combined with ABSORB"),
    ({"P": -1}, "num_roots"),                                               # 4
    ({"P": -1, "N": 0}, "num_roots must not be negative"),
    ({"N": 0}, "capacity"),                                                 # 5
    ({"N": -4, "Cc": 0}, "capacity"),
    ({"Cc": 0}, "max_children"),                                            # 6
    ({"Cc": 65, "T": 0}, "max_children"),
    ({"T": 0}, "max_steps"),                                                # 7
    ({"T": -2, "Lv": 0}, "max_steps"),
    ({"Lv": 0}, "num_leaves must be in [1, 64]"),                           # 8
    ({"Lv": 65, "K": 0}, "num_leaves must be in [1, 64]"),
    ({"Lv": -1, "phases": I}, "num_leaves must be in [1, 64]"),
    ({"P": 2 ** 31 - 1, "Lv": 2, "K": 0}, "num_roots * num_leaves"),        # 9
    ({"P": 2 ** 25, "Lv": 64, "phases": S}, "num_roots * num_leaves"),
    ({"K": 0}, "num_candidates"),                                           # 10
    ({"K": -1, "phases": A, "reserved": 1}, "num_candidates"),
    ({"reserved": 1}, "reserved"),                                          # 11
    ({"reserved2": 1, "phases": S, "null": ("parent",)}, "reserved"),
    *[({"null": (n,), "phases": ph}, "null tree tensor") for n in TREE for ph in (I, A, S)],   # 12
    ({"null": ("pending", "selected"), "phases": A}, "null tree tensor"),
    ({"null": ("selected",), "phases": A}, "null selected"),                # 13
    ({"null": ("selected", "paths"), "phases": S}, "null selected"),
    ({"null": ("path_len",), "phases": I | S}, "null path_len or paths"),   # 14
    ({"null": ("paths", "value"), "phases": A | S}, "null path_len or paths"),
    *[({"null": (n,), "phases": ph}, "null value, leaf_terminal, cand_count, cand_actions or cand_prior") for n in INPUTS for ph in (A, A | S)],  # 15
    ({"null": ("cand_prior",), "odd": ("value_sum",), "phases": A}, "null value, leaf_terminal"),
    *[({"odd": (n,), "phases": ph}, "8-byte aligned") for n in DOUBLES for ph in (I, A | S)],   # 16
    ({"odd": ("value",), "phases": A}, "8-byte aligned"),
    ({"odd2": ("cand_prior",), "phases": A | S}, "cand_prior must be 4-byte aligned"),
    ({"odd": ("value",), "odd2": ("cand_prior",), "phases": A}, "8-byte aligned"),
    ({}, "null handle"),                                                    # 17
    ({"phases": I}, "null handle"),
    ({"phases": I | S, "Lv": 64}, "null handle"),
    ({"phases": S, "null": INPUTS, "Lv": 1}, "null handle"),                # what SELECT does not touch
    ({"phases": S, "K": 0, "null": INPUTS}, "null handle"),                 # num_candidates counts with ABSORB only
    ({"phases": I, "K": -3, "null": ("selected", "path_len", "paths") + INPUTS}, "null handle"),
    ({"phases": A, "null": ("path_len", "paths")}, "null handle"),
    ({"phases": S, "odd": ("value",), "odd2": ("cand_prior",)}, "null handle"),  # inputs are looked at with ABSORB only
    ({"odd": ("parent", "pending", "paths", "cand_actions", "cand_prior")}, "null handle"),  # int32 and float32 tensors need 4 bytes only
    ({"P": 2 ** 25 - 1, "Lv": 64}, "null handle"),                          # the largest row count of 64 leaves
    ({"P": 0}, "null handle"),                                              # the null handle is refused before the no-op
])
def test_argument_checks_need_no_device(kw, msg):
    rc, err = _call(**kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
