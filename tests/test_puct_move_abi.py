"""pcbenv_puct_move on the CPU side: include/pcbenv_move.h declares it, its request struct and its contract,
libpcbenv.so exports it, pcbenv/_move_lib.py binds it with a structure of the C struct's layout -- next to
include/pcbenv.h, include/pcbenv_search.h, include/pcbenv_priors.h and their binding modules, which stay as they are -- and
every argument check refuses what it must before anything touches a device, in the order the header gives, the null handle
last.  No compute call is made."""
import ctypes as C
import os
import re
import shutil

import pytest

import abi_header
from abi_header import REPO, _STRUCT, _declarator
import model_harness
from pcbenv import _lib, _move_lib, _priors_lib, _search_lib

PATH = os.path.join(REPO, "include", "pcbenv_move.h")
TREE = ("num_nodes", "parent", "depth", "visits", "num_children", "first_child", "node_action", "prior", "value_sum", "value_max", "terminal",
        "reward_lo", "reward_hi")
MOVE = ("move_slot", "move_action", "child_visits", "child_actions", "root_value", "remap")
POINTERS = TREE + MOVE + ("reset", "errors_dev", "stream")
SCALARS = ("struct_size", "phases", "num_roots", "capacity", "max_children", "mode", "first_root", "reserved", "seed", "step_index")
MEMBERS = SCALARS + POINTERS
CTYPES = {"struct_size": "uint32_t", "seed": "uint64_t", "step_index": "uint64_t", "reset": "const uint8_t *", "errors_dev": "uint32_t *",
          "stream": "void *", "terminal": "uint8_t *", **{n: "int32_t" for n in SCALARS[1:8]},
          **{n: "double *" for n in ("prior", "value_sum", "value_max", "reward_lo", "reward_hi", "root_value")},
          **{n: "int32_t *" for n in ("num_nodes", "parent", "depth", "visits", "num_children", "first_child", "node_action", "move_slot",
                                      "move_action", "child_visits", "child_actions", "remap")}}


def _raw():
    with open(PATH) as f:
        return f.read()


def _text():
    return re.sub(r"/\*.*?\*/", "", _raw(), flags=re.S)


def _members():
    (name, body), = re.findall(_STRUCT, _text(), flags=re.S)
    assert name == "pcbenv_puct_move_request"
    out = []
    for decl in filter(str.strip, body.split(";")):
        base = re.match(r"\s*((?:const\s+)?\w+)", decl)
        out += [_declarator(base.group(1) + " " + item) for item in decl[base.end():].split(",")]
    return out


def test_header_declares_the_function_the_struct_and_the_contract():
    raw, text = _raw(), _text()
    assert re.search(r'#include\s+"pcbenv_search.h"', text) and "PCBENV_ABI_VERSION" not in raw  # the version is pcbenv.h's, and stays 3
    assert re.search(r"\bint\s+pcbenv_puct_move\s*\(\s*const\s+pcbenv\s*\*\s*env\s*,\s*const\s+pcbenv_puct_move_request\s*\*\s*req\s*\)\s*;", text)
    assert len(re.findall(r"\b\w+\s*\([^()]*\)\s*;", text)) == 1  # one prototype
    members = _members()
    assert tuple(n for _, n in members) == MEMBERS
    assert {n: t for t, n in members} == CTYPES
    defines = dict(re.findall(r"#define\s+(PCBENV_MOVE_\w+)\s+(\d+)", text))
    assert defines == {"PCBENV_MOVE_CHOOSE": "1", "PCBENV_MOVE_REROOT": "2", "PCBENV_MOVE_GREEDY": "0", "PCBENV_MOVE_PROPORTIONAL": "1"}
    assert (_move_lib.MOVE_CHOOSE, _move_lib.MOVE_REROOT, _move_lib.MOVE_GREEDY, _move_lib.MOVE_PROPORTIONAL) == (1, 2, 0, 1)
    block = re.sub(r"\s*\n \*\s*", " ", raw[:raw.index("typedef struct pcbenv_puct_move_request")].rsplit("/*", 1)[1])
    for phrase in ("Enqueue only, no allocation, no synchronisation, one kernel on req->stream", "hipGraph",
                   "the handle supplies the device and pcbenv_last_error only", "in the order CHOOSE, REROOT",
                   "are checked (1 <= k <= C, 1 <= fc <= N - k) before they address anything", "entries behind k are zero",
                   "one IEEE division, NaN for an unvisited root", "ties to the lowest c", "the int64 sum of the children's visits",
                   "hi32(mix64(mix64(seed ^ 0x9E3779B97F4A7C15 * (first_root + p + 1)) + step_index))", "r = (h * total) >> 32",
                   "the least c whose inclusive prefix sum of visits exceeds r", "falls back to greedy",
                   "no floating-point operations in the choice", "move_slot = -1 and action (0, 0, 0)",
                   "exactly what PCBENV_TREE_INIT leaves", "remap[p, :] = -1", "the identity on [0, n) and -1 behind",
                   "the rank of s among the kept slots, in slot order", "go through remap", "its depth drops by depth(m)",
                   "parent = -1, depth = 0, node_action = 0 and prior = 0", "reward_lo and reward_hi are kept", "in place",
                   "is compared before it addresses anything", "0 <= parent(s) < s for every used s >= 1", "num_children in [0, C]",
                   "with every slot of that range kept", "leaves that root's tree tensors untouched", "all or nothing",
                   "sets its remap row to -1", "ORs bit 1 (value 2) into *errors_dev", "reset uint8 [P], may be NULL", "errors_dev may be NULL",
                   "PCBENV_EINVAL (checked before any device call, in this order)", "[1, PCBENV_MAX_TREE_CHILDREN]",
                   "num_roots == 0 is a no-op success"):
        assert phrase in block, phrase
    assert "only enqueues" in raw.split("#ifndef PCBENV_MOVE_H")[0]


def test_the_other_headers_and_bindings_are_as_they_were():
    assert len(abi_header.prototypes()) == 40 and len(abi_header.structs()) == 6
    assert "puct_move" not in abi_header.raw()
    for h in ("pcbenv_search.h", "pcbenv_priors.h"):
        with open(os.path.join(REPO, "include", h)) as f:
            assert "_move" not in f.read()
    assert len(_lib.EXPORTS) == 40 and _search_lib.EXPORTS == ("pcbenv_puct_advance",) and _priors_lib.EXPORTS == ("pcbenv_top_priors",)
    assert not [n for n in list(vars(_lib)) + list(vars(_search_lib)) + list(vars(_priors_lib)) if "move" in n.lower()]
    assert re.search(r"#define\s+PCBENV_ABI_VERSION\s+3\b", abi_header.text())


def test_exported_and_bound():
    L = _move_lib.bind(_priors_lib.bind(_search_lib.bind(_lib.load())))
    assert _move_lib.EXPORTS == ("pcbenv_puct_move",) and hasattr(L, "pcbenv_puct_move")
    assert len(L.pcbenv_puct_move.argtypes) == 2 and L.pcbenv_puct_move.restype is C.c_int
    R = _move_lib.PcbenvPuctMoveRequest
    assert tuple(n for n, _ in R._fields_) == MEMBERS
    kinds = dict(struct_size=C.c_uint32, seed=C.c_uint64, step_index=C.c_uint64, **{n: C.c_void_p for n in POINTERS})
    for n, t in R._fields_:
        assert t is kinds.get(n, C.c_int32), n
    # csrc/pcb_puct_move.hip static_asserts the same figures of the struct as the library compiled it
    assert C.sizeof(R) == 224 and R.stream.offset == 216 and R.seed.offset == 32
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3


def test_bind_refuses_a_library_without_the_symbol():
    class Without:
        pass
    with pytest.raises(ImportError, match="pcbenv_puct_move"):
        _move_lib.bind(Without())


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_ctypes_structure_has_the_c_layout():
    """A compiled probe: sizeof and every member's offset as a C compiler lays include/pcbenv_move.h out."""
    offsets, size = model_harness.layout("pcbenv_move.h", "pcbenv_puct_move_request", MEMBERS)
    R = _move_lib.PcbenvPuctMoveRequest
    assert size == C.sizeof(R)
    assert offsets == {n: getattr(R, n).offset for n in MEMBERS}


_HOST = (C.c_uint64 * 8)()  # host memory: never dereferenced, every call below fails before a device is touched
BOTH = _move_lib.MOVE_CHOOSE | _move_lib.MOVE_REROOT
CHOSEN = ("move_action", "child_visits", "child_actions", "root_value")
DOUBLES = ("prior", "value_sum", "value_max", "reward_lo", "reward_hi")


def _call(request=True, size=None, phases=BOTH, mode=0, roots=8, capacity=31, C_=16, reserved=0, null=(), off=None):
    """off: {member: byte offset from an 8-byte boundary}.  reset, errors_dev and stream stay null: all are optional."""
    L = _move_lib.bind(_lib.load())
    R = _move_lib.PcbenvPuctMoveRequest
    req = R(struct_size=C.sizeof(R) if size is None else size, phases=phases, mode=mode, num_roots=roots, capacity=capacity, max_children=C_,
            reserved=reserved)
    for n in TREE + MOVE:
        if n not in null:
            setattr(req, n, C.addressof(_HOST) + (off or {}).get(n, 0))
    rc = L.pcbenv_puct_move(None, C.byref(req) if request else None)
    return rc, L.pcbenv_last_error(None).decode()


@pytest.mark.parametrize("kw, msg", [
    ({"request": False}, "null request"),                                               # 1
    ({"size": 0}, "struct_size"),                                                       # 2
    ({"size": 216, "phases": 0}, "struct_size"),                                        # the order: the size before any field is believed
    ({"size": 232, "mode": 7}, "struct_size"),
    ({"phases": 0}, "phases"),                                                          # 3
    ({"phases": 4, "mode": 7}, "phases"),
    ({"phases": 7, "roots": -1}, "phases"),
    ({"phases": -1}, "phases"),
    ({"mode": 2}, "unknown mode"),                                                      # 4
    ({"mode": -1, "roots": -1}, "unknown mode"),
    ({"mode": 2, "phases": 1, "capacity": 0}, "unknown mode"),
    ({"roots": -1}, "num_roots"),                                                       # 5
    ({"roots": -1, "capacity": 0}, "num_roots"),
    ({"mode": 2, "phases": 2, "roots": -3}, "num_roots"),                               # REROOT alone does not read the mode
    ({"capacity": 0}, "capacity"),                                                      # 6
    ({"capacity": -4, "C_": 0}, "capacity"),
    ({"C_": 0}, "max_children"),                                                        # 7
    ({"C_": 65, "reserved": 1}, "max_children"),
    ({"C_": -1}, "max_children"),
    ({"reserved": 1}, "reserved"),                                                      # 8
    ({"reserved": -1, "null": ("parent",)}, "reserved"),
    *[({"null": (n,)}, "null tree tensor") for n in TREE],                              # 9
    ({"null": ("terminal", "move_slot")}, "null tree tensor"),
    ({"null": ("move_slot",)}, "null move_slot"),                                       # 10
    ({"null": ("move_slot", "remap"), "phases": 2}, "null move_slot"),
    ({"null": ("move_slot", "move_action")}, "null move_slot"),
    *[({"null": (n,)}, "null move_action, child_visits, child_actions or root_value") for n in CHOSEN],   # 11
    *[({"null": (n, "remap"), "phases": 1}, "null move_action, child_visits, child_actions or root_value") for n in CHOSEN],
    ({"null": ("root_value", "remap")}, "null move_action, child_visits"),
    ({"null": ("remap",)}, "null remap"),                                               # 12
    ({"null": ("remap",) + CHOSEN, "phases": 2}, "null remap"),
    ({"null": ("remap",), "off": {"prior": 4}}, "null remap"),
    *[({"off": {n: 4}}, "8-byte aligned") for n in DOUBLES + ("root_value",)],          # 13
    ({"off": {"value_max": 1}, "phases": 2}, "8-byte aligned"),
    ({}, "null handle"),                                                                # 14
    ({"phases": 1, "null": ("remap",)}, "null handle"),                                 # CHOOSE alone needs no remap
    ({"phases": 2, "null": CHOSEN}, "null handle"),                                     # REROOT alone none of CHOOSE's outputs
    ({"phases": 2, "mode": 9, "off": {"root_value": 4}}, "null handle"),                # nor its mode, nor root_value's alignment
    ({"mode": 1}, "null handle"),
    ({"off": {n: 4 for n in ("parent", "visits", "move_slot", "remap", "child_visits")}}, "null handle"),  # int32 needs 4
    ({"C_": 1}, "null handle"),
    ({"C_": 64}, "null handle"),
    ({"roots": 0}, "null handle"),                                                      # the null handle is refused before the no-op
])
def test_argument_checks_need_no_device(kw, msg):
    rc, err = _call(**kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
