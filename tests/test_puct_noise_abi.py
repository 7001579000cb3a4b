"""pcbenv_puct_root_noise on the CPU side: include/pcbenv_noise.h declares it, its request struct and its contract,
libpcbenv.so exports it, pcbenv/_noise_lib.py binds it with a structure of the C struct's layout -- next to
include/pcbenv.h, include/pcbenv_search.h and their bindings, which stay as they are -- and every argument check refuses
what it must before anything touches a device, in the order the header gives, the null handle last.  No compute call is
made."""
import ctypes as C
import math
import os
import re
import shutil

import pytest

from abi_header import REPO, _STRUCT, _declarator
import model_harness
from pcbenv import _lib, _move_lib, _noise_lib, _search_lib

PATH = os.path.join(REPO, "include", "pcbenv_noise.h")
TENSORS = _noise_lib.NOISE_TENSORS
POINTERS = TENSORS + ("errors_dev", "stream")
INTS = ("num_roots", "capacity", "max_children", "first_root", "reserved")
MEMBERS = ("struct_size",) + INTS + ("seed", "step_index", "alpha", "eps") + POINTERS
CTYPES = {"struct_size": "uint32_t", "seed": "uint64_t", "step_index": "uint64_t", "alpha": "double", "eps": "double",
          "num_children": "int32_t *", "first_child": "int32_t *", "prior": "double *", "noised": "int32_t *", "errors_dev": "uint32_t *",
          "stream": "void *", **{n: "int32_t" for n in INTS}}


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
    assert re.search(r"\bint\s+pcbenv_puct_root_noise\s*\(\s*const\s+pcbenv\s*\*\s*env\s*,\s*const\s+pcbenv_puct_noise_request\s*\*\s*req\s*\)\s*;", text)
    assert len(re.findall(r"\b\w+\s*\([^()]*\)\s*;", text)) == 1  # one prototype
    members = _members(text, "pcbenv_puct_noise_request")
    assert tuple(n for _, n in members) == MEMBERS
    assert {n: t for t, n in members} == CTYPES
    # the tree pointers it uses have pcbenv_puct_request's names and types
    with open(os.path.join(REPO, "include", "pcbenv_search.h")) as f:
        base = {n: t for t, n in _members(re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S), "pcbenv_puct_request")}
    assert all(base[n] == CTYPES[n] for n in ("num_children", "first_child", "prior", "errors_dev", "stream"))
    block = re.sub(r"\s*\n \*\s*", " ", raw[:raw.index("typedef struct pcbenv_puct_noise_request")].rsplit("/*", 1)[1])
    for phrase in ("one kernel launch on req->stream", "nothing the library owns is read or written", "no bound buffers",
                   "Enqueue only, no allocation, no synchronisation", "hipGraph", "noised[p] == 0 and k >= 1", "before they address anything",
                   "bit 1 (value 2)", "keeps noised[p] = 0", "a later call finds it", "is a no-op",
                   "Nothing but prior of the k children and noised[p] is ever stored",
                   "mix64(mix64(seed ^ 0x9E3779B97F4A7C15 * (first_root + p + 1)) + step_index)", "(64 t + c + 1)", "((w >> 12) + 0.5) * 2^-52",
                   "never on P, on C or on the other children", "d = a - 1/3", "cc = (1/3) / sqrt(d)", "Attempt t = 0 .. 31", "3 t, 3 t + 1, 3 t + 2",
                   "fails if s >= 1", "fails if v <= 0", "ln u3 < ((0.5 (x x) + d) - d v) + d ln v", "g = d v", "If all 32 attempts fail, g = d",
                   "draw number 96", "IEEE + - * / alone", "summed in that order", "or 1 / k if S is not a finite number greater than 0",
                   "(double)(float)((1 - eps) * prior(fc + c) + eps * eta_c)", "unchanged bit for bit",
                   "PCBENV_EINVAL (checked before any device call, in this order)", "num_roots == 0 is a no-op success"):
        assert phrase in block, phrase
    assert "only enqueues" in raw.split("#ifndef PCBENV_NOISE_H")[0]


def test_exported_and_bound():
    L = _noise_lib.bind(_lib.load())
    assert _noise_lib.EXPORTS == ("pcbenv_puct_root_noise",) and hasattr(L, "pcbenv_puct_root_noise")
    assert len(L.pcbenv_puct_root_noise.argtypes) == 2 and L.pcbenv_puct_root_noise.restype is C.c_int
    assert all("pcbenv_puct_root_noise" not in m.EXPORTS for m in (_lib, _search_lib, _move_lib))
    R = _noise_lib.PcbenvPuctNoiseRequest
    assert tuple(n for n, _ in R._fields_) == MEMBERS
    kinds = dict(struct_size=C.c_uint32, seed=C.c_uint64, step_index=C.c_uint64, alpha=C.c_double, eps=C.c_double, **{n: C.c_void_p for n in POINTERS})
    for n, t in R._fields_:
        assert t is kinds.get(n, C.c_int32), n
    # csrc/pcb_puct_noise.hip static_asserts the same figures of the struct as the library compiled it
    assert C.sizeof(R) == 104 and R.stream.offset == 96 and R.seed.offset == 24 and R.alpha.offset == 40
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_ctypes_structure_has_the_c_layout():
    """A compiled probe: sizeof and every member's offset as a C compiler lays include/pcbenv_noise.h out."""
    offsets, size = model_harness.layout("pcbenv_noise.h", "pcbenv_puct_noise_request", MEMBERS)
    R = _noise_lib.PcbenvPuctNoiseRequest
    assert size == C.sizeof(R)
    assert offsets == {n: getattr(R, n).offset for n in MEMBERS}


_HOST = (C.c_uint64 * 8)()  # host memory: never dereferenced, every call below fails before a device is touched


def _call(request=True, size=None, P=8, N=5, Cc=3, reserved=0, alpha=0.3, eps=0.25, null=(), odd=()):
    L = _noise_lib.bind(_lib.load())
    R = _noise_lib.PcbenvPuctNoiseRequest
    req = R(struct_size=C.sizeof(R) if size is None else size, num_roots=P, capacity=N, max_children=Cc, reserved=reserved, alpha=alpha, eps=eps)
    for n in TENSORS:  # errors_dev and stream stay null: both are optional
        if n not in null:
            setattr(req, n, C.addressof(_HOST) + (4 if n in odd else 0))
    rc = L.pcbenv_puct_root_noise(None, C.byref(req) if request else None)
    return rc, L.pcbenv_last_error(None).decode()


NAN, INF = math.nan, math.inf


@pytest.mark.parametrize("kw, msg", [
    ({"request": False}, "null request"),                                   # 1
    ({"size": 0}, "struct_size"),                                           # 2
    ({"size": 224, "P": -1}, "struct_size"),                                # pcbenv_puct_move_request's size is not this struct's
    ({"size": 112, "N": 0}, "struct_size"),
    ({"P": -1}, "num_roots"),                                               # 3
    ({"P": -1, "N": 0}, "num_roots must not be negative"),
    ({"N": 0}, "capacity"),                                                 # 4
    ({"N": -4, "Cc": 0}, "capacity"),
    ({"Cc": 0}, "max_children"),                                            # 5
    ({"Cc": 65, "reserved": 1}, "max_children"),
    ({"reserved": 1}, "reserved"),                                          # 6
    ({"reserved": -1, "alpha": NAN}, "reserved"),
    ({"alpha": NAN}, "alpha must be in [0.01, 100]"),                       # 7
    ({"alpha": INF}, "alpha must be in"),
    ({"alpha": 0.0099}, "alpha must be in"),
    ({"alpha": 100.5, "eps": 2.0}, "alpha must be in"),
    ({"alpha": -1.0}, "alpha must be in"),
    ({"eps": NAN}, "eps must be in [0, 1]"),                                # 8
    ({"eps": -1e-9}, "eps must be in"),
    ({"eps": 1.0000001, "null": ("prior",)}, "eps must be in"),
    ({"eps": INF}, "eps must be in"),
    *[({"null": (n,)}, "null tree tensor") for n in TENSORS],               # 9
    ({"null": ("noised",), "odd": ("prior",)}, "null tree tensor"),
    ({"odd": ("prior",)}, "8-byte aligned"),                                # 10
    ({}, "null handle"),                                                    # 11
    ({"alpha": 0.01, "eps": 0.0}, "null handle"),                           # the ends of the ranges are in
    ({"alpha": 100.0, "eps": 1.0, "Cc": 64}, "null handle"),
    ({"odd": ("num_children", "first_child", "noised")}, "null handle"),    # int32 tensors need 4 bytes only
    ({"P": 0}, "null handle"),                                              # the null handle is refused before the no-op
])
def test_argument_checks_need_no_device(kw, msg):
    rc, err = _call(**kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
