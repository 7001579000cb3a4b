"""pcbenv_puct_advance on the CPU side: include/pcbenv_search.h declares it, its request struct and its contract,
libpcbenv.so exports it, pcbenv/_search_lib.py binds it with a structure of the C struct's layout -- next to
include/pcbenv.h and pcbenv/_lib.py, which stay as they are -- and every argument check refuses what it must before
anything touches a device, in the order the header gives, the null handle last.  No compute call is made."""
import ctypes as C
import os
import re
import shutil

import pytest

import abi_header
from abi_header import REPO, _STRUCT, _declarator
import model_harness
from pcbenv import _lib, _search_lib

PATH = os.path.join(REPO, "include", "pcbenv_search.h")
TREE = _search_lib.PUCT_TREE_TENSORS
INPUTS = _search_lib.PUCT_INPUTS
POINTERS = TREE + ("selected", "path_len", "paths") + INPUTS + ("errors_dev", "stream")
INTS = ("phases", "num_roots", "capacity", "max_children", "max_steps", "num_candidates", "reserved")
MEMBERS = ("struct_size",) + INTS + ("c_puct",) + POINTERS
CTYPES = {"struct_size": "uint32_t", "c_puct": "double", "node_action": "int32_t *", "terminal": "uint8_t *", "value": "const double *",
          "leaf_terminal": "const uint8_t *", "cand_count": "const int32_t *", "cand_actions": "const int32_t *", "cand_prior": "const float *",
          "errors_dev": "uint32_t *", "stream": "void *",
          **{n: "int32_t" for n in INTS}, **{n: "double *" for n in ("prior", "value_sum", "value_max", "reward_lo", "reward_hi")},
          **{n: "int32_t *" for n in ("num_nodes", "parent", "depth", "visits", "num_children", "first_child", "selected", "path_len", "paths")}}


def _raw():
    with open(PATH) as f:
        return f.read()


def _text():
    return re.sub(r"/\*.*?\*/", "", _raw(), flags=re.S)


def _members():
    (name, body), = re.findall(_STRUCT, _text(), flags=re.S)
    assert name == "pcbenv_puct_request"
    out = []
    for decl in filter(str.strip, body.split(";")):
        base = re.match(r"\s*((?:const\s+)?\w+)", decl)
        out += [_declarator(base.group(1) + " " + item) for item in decl[base.end():].split(",")]
    return out


def test_header_declares_the_function_the_struct_and_the_contract():
    raw, text = _raw(), _text()
    assert re.search(r'#include\s+"pcbenv.h"', text) and "PCBENV_ABI_VERSION" not in text  # the version is pcbenv.h's, and stays 3
    assert re.search(r"\bint\s+pcbenv_puct_advance\s*\(\s*const\s+pcbenv\s*\*\s*env\s*,\s*const\s+pcbenv_puct_request\s*\*\s*req\s*\)\s*;", text)
    assert len(re.findall(r"\b\w+\s*\([^()]*\)\s*;", text)) == 1  # one prototype
    members = _members()
    assert tuple(n for _, n in members) == MEMBERS
    assert {n: t for t, n in members} == CTYPES
    assert not re.search(r"#define\s+PCBENV_TREE_", text)  # the phases are pcbenv.h's
    block = re.sub(r"\s*\n \*\s*", " ", raw[:raw.index("typedef struct pcbenv_puct_request")].rsplit("/*", 1)[1])
    for phrase in ("one kernel launch on req->stream", "nothing the library owns is read or written", "no bound buffers",
                   "Enqueue only, no allocation, no synchronisation", "hipGraph", "in the order INIT, ABSORB, SELECT",
                   "first_child .. first_child + k - 1", "ties go to the lowest c", "No logarithm is computed", "are untouched",
                   "At most max_steps levels", "it is never cleared", "clamp(cand_count, 0, min(K, C))", "is data, not an error",
                   "all or nothing", "bit 0 (value 1)", "bit 1 (value 2)", "not renormalised", "at most max_steps + 1 nodes",
                   "u = c_puct * prior(ch) * sqrt((double)max(visits(node), 1)) / (1.0 + n_c)",
                   "PCBENV_EINVAL (checked before any device call, in this order)", "num_roots == 0 is a no-op success"):
        assert phrase in block, phrase
    assert "only enqueues" in raw.split("#ifndef PCBENV_SEARCH_H")[0]


def test_pcbenv_h_and_lib_are_as_they_were():
    assert len(abi_header.prototypes()) == 40 and len(abi_header.structs()) == 6
    assert "pcbenv_puct" not in abi_header.raw()
    assert len(_lib.EXPORTS) == 40 and "pcbenv_puct_advance" not in _lib.EXPORTS
    assert not [n for n in vars(_lib) if "puct" in n.lower()]
    assert re.search(r"#define\s+PCBENV_ABI_VERSION\s+3\b", abi_header.text())


def test_exported_and_bound():
    L = _search_lib.bind(_lib.load())
    assert _search_lib.EXPORTS == ("pcbenv_puct_advance",) and hasattr(L, "pcbenv_puct_advance")
    assert len(L.pcbenv_puct_advance.argtypes) == 2 and L.pcbenv_puct_advance.restype is C.c_int
    R = _search_lib.PcbenvPuctRequest
    assert tuple(n for n, _ in R._fields_) == MEMBERS
    kinds = dict(struct_size=C.c_uint32, c_puct=C.c_double, **{n: C.c_void_p for n in POINTERS})
    for n, t in R._fields_:
        assert t is kinds.get(n, C.c_int32), n
    # csrc/pcb_puct.hip static_asserts the same two figures of the struct as the library compiled it
    assert C.sizeof(R) == 224 and R.stream.offset == 216 and R.c_puct.offset == 32
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_ctypes_structure_has_the_c_layout():
    """A compiled probe: sizeof and every member's offset as a C compiler lays include/pcbenv_search.h out."""
    offsets, size = model_harness.layout("pcbenv_search.h", "pcbenv_puct_request", MEMBERS)
    R = _search_lib.PcbenvPuctRequest
    assert size == C.sizeof(R)
    assert offsets == {n: getattr(R, n).offset for n in MEMBERS}


_HOST = (C.c_uint64 * 8)()  # host memory: never dereferenced, every call below fails before a device is touched


def _call(request=True, size=None, phases=_lib.TREE_ABSORB | _lib.TREE_SELECT, P=8, N=5, Cc=3, T=4, K=2, reserved=0, null=(), odd=(), odd2=()):
    L = _search_lib.bind(_lib.load())
    R = _search_lib.PcbenvPuctRequest
    req = R(struct_size=C.sizeof(R) if size is None else size, phases=phases, num_roots=P, capacity=N, max_children=Cc, max_steps=T,
            num_candidates=K, reserved=reserved, c_puct=1.0)
    for n in POINTERS[:-2]:  # errors_dev and stream stay null: both are optional
        if n not in null:
            setattr(req, n, C.addressof(_HOST) + (4 if n in odd else 2 if n in odd2 else 0))
    rc = L.pcbenv_puct_advance(None, C.byref(req) if request else None)
    return rc, L.pcbenv_last_error(None).decode()


I, A, S = _lib.TREE_INIT, _lib.TREE_ABSORB, _lib.TREE_SELECT
DOUBLES = ("prior", "value_sum", "value_max", "reward_lo", "reward_hi")


@pytest.mark.parametrize("kw, msg", [
    ({"request": False}, "null request"),                                   # 1
    ({"size": 0}, "struct_size"),                                           # 2
    ({"size": 216, "phases": 0}, "struct_size"),                            # the order: the size before any field is believed
    ({"size": 232, "P": -1}, "struct_size"),
    ({"phases": 0}, "phases must be"),                                      # 3
    ({"phases": 8, "P": -1}, "phases must be"),
    ({"phases": 15}, "phases must be"),
    ({"phases": -1}, "phases must be"),
    ({"phases": I | A}, "INIT cannot be combined with ABSORB"),
    ({"phases": I | A | S, "P": -1}, "INIT cannot be combined with ABSORB"),
    ({"P": -1}, "num_roots"),                                               # 4
    ({"P": -1, "N": 0}, "num_roots"),
    ({"N": 0}, "capacity"),                                                 # 5
    ({"N": -4, "Cc": 0}, "capacity"),
    ({"Cc": 0}, "max_children"),                                            # 6
    ({"Cc": 65, "T": 0}, "max_children"),
    ({"Cc": -1}, "max_children"),
    ({"T": 0}, "max_steps"),                                                # 7
    ({"T": -2, "K": 0}, "max_steps"),
    ({"K": 0}, "num_candidates"),                                           # 8
    ({"K": -1, "phases": A, "reserved": 1}, "num_candidates"),
    ({"reserved": 1}, "reserved"),                                          # 9
    ({"reserved": -1, "phases": S, "null": ("parent",)}, "reserved"),
    *[({"null": (n,), "phases": ph}, "null tree tensor") for n in TREE for ph in (I, A, S)],   # 10
    ({"null": ("prior", "selected"), "phases": A}, "null tree tensor"),
    ({"null": ("selected",), "phases": A}, "null selected"),                # 11
    ({"null": ("selected", "paths"), "phases": S}, "null selected"),
    ({"null": ("path_len",), "phases": I | S}, "null path_len or paths"),   # 12
    ({"null": ("paths", "value"), "phases": A | S}, "null path_len or paths"),
    *[({"null": (n,), "phases": ph}, "null value, leaf_terminal, cand_count, cand_actions or cand_prior") for n in INPUTS for ph in (A, A | S)],  # 13
    ({"null": ("cand_prior",), "odd": ("value_sum",), "phases": A}, "null value, leaf_terminal"),
    *[({"odd": (n,), "phases": ph}, "8-byte aligned") for n in DOUBLES for ph in (I, A | S)],   # 14
    ({"odd": ("value",), "phases": A}, "8-byte aligned"),
    ({"odd2": ("cand_prior",), "phases": A | S}, "cand_prior must be 4-byte aligned"),
    ({"odd": ("value",), "odd2": ("cand_prior",), "phases": A}, "8-byte aligned"),
    ({}, "null handle"),                                                    # 15
    ({"phases": I}, "null handle"),
    ({"phases": I | S}, "null handle"),
    ({"phases": S, "null": INPUTS}, "null handle"),                         # what SELECT does not touch
    ({"phases": S, "K": 0, "null": INPUTS}, "null handle"),                 # num_candidates counts with ABSORB only
    ({"phases": I, "K": -3, "null": ("selected", "path_len", "paths") + INPUTS}, "null handle"),
    ({"phases": A, "null": ("path_len", "paths")}, "null handle"),
    ({"phases": S, "odd": ("value",), "odd2": ("cand_prior",)}, "null handle"),  # inputs are looked at with ABSORB only
    ({"odd": ("parent", "paths", "cand_actions", "cand_prior")}, "null handle"),  # int32 and float32 tensors need 4 bytes only
    ({"Cc": 64, "N": 1, "T": 1, "K": 1}, "null handle"),
    ({"P": 0}, "null handle"),                                              # the null handle is refused before the no-op
])
def test_argument_checks_need_no_device(kw, msg):
    rc, err = _call(**kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
