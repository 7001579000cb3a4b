"""pcbenv_top_priors on the CPU side: include/pcbenv_priors.h declares it, its request struct and its contract,
libpcbenv.so exports it, pcbenv/_priors_lib.py binds it with a structure of the C struct's layout -- next to
include/pcbenv.h, include/pcbenv_search.h and their binding modules, which stay as they are -- and every argument check
refuses what it must before anything touches a device, in the order the header gives, the null handle last of those that
need no handle.  No compute call is made."""
import ctypes as C
import os
import re
import shutil

import pytest

import abi_header
from abi_header import REPO, _STRUCT, _declarator
import model_harness
from pcbenv import _lib, _priors_lib, _search_lib

PATH = os.path.join(REPO, "include", "pcbenv_priors.h")
POINTERS = ("logits", "mask_bits", "cand_count", "cand_actions", "cand_prior", "errors_dev", "stream")
MEMBERS = ("struct_size", "logits_dtype", "num_candidates", "reserved", "num_rows") + POINTERS
CTYPES = {"struct_size": "uint32_t", "logits_dtype": "int32_t", "num_candidates": "int32_t", "reserved": "int32_t", "num_rows": "int64_t",
          "logits": "const void *", "mask_bits": "const uint64_t *", "cand_count": "int32_t *", "cand_actions": "int32_t *",
          "cand_prior": "float *", "errors_dev": "uint32_t *", "stream": "void *"}


def _raw():
    with open(PATH) as f:
        return f.read()


def _text():
    return re.sub(r"/\*.*?\*/", "", _raw(), flags=re.S)


def _members():
    (name, body), = re.findall(_STRUCT, _text(), flags=re.S)
    assert name == "pcbenv_top_priors_request"
    out = []
    for decl in filter(str.strip, body.split(";")):
        base = re.match(r"\s*((?:const\s+)?\w+)", decl)
        out += [_declarator(base.group(1) + " " + item) for item in decl[base.end():].split(",")]
    return out


def test_header_declares_the_function_the_struct_and_the_contract():
    raw, text = _raw(), _text()
    assert re.search(r'#include\s+"pcbenv.h"', text) and "PCBENV_ABI_VERSION" not in raw  # the version is pcbenv.h's, and stays 3
    assert re.search(r"\bint\s+pcbenv_top_priors\s*\(\s*const\s+pcbenv\s*\*\s*env\s*,\s*const\s+pcbenv_top_priors_request\s*\*\s*req\s*\)\s*;", text)
    assert len(re.findall(r"\b\w+\s*\([^()]*\)\s*;", text)) == 1  # one prototype
    members = _members()
    assert tuple(n for _, n in members) == MEMBERS
    assert {n: t for t, n in members} == CTYPES
    assert not re.search(r"#define\s+PCBENV_", text.replace("#define PCBENV_PRIORS_H", ""))  # dtypes and the limit of K are pcbenv.h's
    block = re.sub(r"\s*\n \*\s*", " ", raw[:raw.index("typedef struct pcbenv_top_priors_request")].rsplit("/*", 1)[1])
    for phrase in ("one kernel launch on req->stream", "Enqueue only, no allocation, no synchronisation", "hipGraph",
                   "exactly the layouts pcbenv_puct_request reads", "orientation o reads plane o & 1", "the square kind reads plane 0 only",
                   "bits of columns >= W are ignored", "no bound buffers are needed", "mask_bits == NULL: row e is environment e",
                   "exactly as pcbenv_sample_logits reads them", "no mask is copied", "has no influence", "widened exactly to float32",
                   "-0.0 equals +0.0", "ties go to the lower flat index", "come last, in index order", "k = min(K, n)",
                   "float32(exp(v - M) / Z)", "not renormalised over the k kept", "A -inf logit has prior 0",
                   "Entries c >= k are action (0, 0, 0) and prior 0", "Every element of the three outputs is written",
                   "two launches give the same bits", "no floating-point atomics", "No legal action: count 0", "bit 0 (value 1)",
                   "bit 1 (value 2)", "the first k legal actions in flat order, each with prior float32(1.0 / n)",
                   "PCBENV_EINVAL (checked before any device call, in this order)", "[1, PCBENV_MAX_TREE_CHILDREN]",
                   "PCBENV_ESTATE (mask_bits == NULL only)", "num_rows == 0 is a no-op success"):
        assert phrase in block, phrase
    assert "only enqueues" in raw.split("#ifndef PCBENV_PRIORS_H")[0]


def test_the_other_headers_and_bindings_are_as_they_were():
    assert len(abi_header.prototypes()) == 40 and len(abi_header.structs()) == 6
    assert "top_priors" not in abi_header.raw()
    with open(os.path.join(REPO, "include", "pcbenv_search.h")) as f:
        assert "top_priors" not in f.read()
    assert len(_lib.EXPORTS) == 40 and _search_lib.EXPORTS == ("pcbenv_puct_advance",)
    assert not [n for n in list(vars(_lib)) + list(vars(_search_lib)) if "priors" in n.lower()]
    assert re.search(r"#define\s+PCBENV_ABI_VERSION\s+3\b", abi_header.text())


def test_exported_and_bound():
    L = _priors_lib.bind(_search_lib.bind(_lib.load()))
    assert _priors_lib.EXPORTS == ("pcbenv_top_priors",) and hasattr(L, "pcbenv_top_priors")
    assert len(L.pcbenv_top_priors.argtypes) == 2 and L.pcbenv_top_priors.restype is C.c_int
    R = _priors_lib.PcbenvTopPriorsRequest
    assert tuple(n for n, _ in R._fields_) == MEMBERS
    kinds = dict(struct_size=C.c_uint32, num_rows=C.c_int64, **{n: C.c_void_p for n in POINTERS})
    for n, t in R._fields_:
        assert t is kinds.get(n, C.c_int32), n
    # csrc/pcb_top_priors.hip static_asserts the same two figures of the struct as the library compiled it
    assert C.sizeof(R) == 80 and R.stream.offset == 72 and R.num_rows.offset == 16
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3


def test_bind_refuses_a_library_without_the_symbol():
    class Without:
        pass
    with pytest.raises(ImportError, match="pcbenv_top_priors"):
        _priors_lib.bind(Without())


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_ctypes_structure_has_the_c_layout():
    """A compiled probe: sizeof and every member's offset as a C compiler lays include/pcbenv_priors.h out."""
    offsets, size = model_harness.layout("pcbenv_priors.h", "pcbenv_top_priors_request", MEMBERS)
    R = _priors_lib.PcbenvTopPriorsRequest
    assert size == C.sizeof(R)
    assert offsets == {n: getattr(R, n).offset for n in MEMBERS}


_HOST = (C.c_uint64 * 8)()  # host memory: never dereferenced, every call below fails before a device is touched
F32, BF16 = _lib.LOGITS_F32, _lib.LOGITS_BF16


def _call(request=True, size=None, dtype=F32, K=16, reserved=0, rows=8, null=(), off=None):
    """off: {member: byte offset from an 8-byte boundary}.  mask_bits is given unless it is in `null`."""
    L = _priors_lib.bind(_lib.load())
    R = _priors_lib.PcbenvTopPriorsRequest
    req = R(struct_size=C.sizeof(R) if size is None else size, logits_dtype=dtype, num_candidates=K, reserved=reserved, num_rows=rows)
    for n in POINTERS[:-2]:  # errors_dev and stream stay null: both are optional
        if n not in null:
            setattr(req, n, C.addressof(_HOST) + (off or {}).get(n, 0))
    rc = L.pcbenv_top_priors(None, C.byref(req) if request else None)
    return rc, L.pcbenv_last_error(None).decode()


OUTPUTS = ("cand_count", "cand_actions", "cand_prior")


@pytest.mark.parametrize("kw, msg", [
    ({"request": False}, "null request"),                                               # 1
    ({"size": 0}, "struct_size"),                                                       # 2
    ({"size": 72, "dtype": 9}, "struct_size"),                                          # the order: the size before any field is believed
    ({"size": 88, "K": 0}, "struct_size"),
    ({"dtype": 2}, "unknown logits dtype"),                                             # 3
    ({"dtype": -1, "K": 0}, "unknown logits dtype"),
    ({"K": 0}, "num_candidates"),                                                       # 4
    ({"K": 65, "reserved": 1}, "num_candidates"),
    ({"K": -1}, "num_candidates"),
    ({"reserved": 1}, "reserved"),                                                      # 5
    ({"reserved": -1, "rows": -1}, "reserved"),
    ({"rows": -1}, "num_rows"),                                                         # 6
    ({"rows": -5, "null": ("logits",)}, "num_rows"),
    ({"rows": 2 ** 31}, "num_rows"),
    *[({"null": (n,)}, "null logits, cand_count, cand_actions or cand_prior") for n in ("logits",) + OUTPUTS],   # 7
    ({"null": ("cand_prior",), "off": {"logits": 2}}, "null logits, cand_count"),
    ({"off": {"logits": 2}}, "logits pointer not aligned"),                             # 8
    ({"off": {"logits": 1}, "dtype": BF16}, "logits pointer not aligned"),
    ({"off": {"logits": 6, "mask_bits": 4}}, "logits pointer not aligned"),
    ({"off": {"mask_bits": 4}}, "mask bits pointer not aligned"),                       # 9
    ({"off": {"mask_bits": 1, "cand_count": 2}}, "mask bits pointer not aligned"),
    *[({"off": {n: 2}}, "must be 4-byte aligned") for n in OUTPUTS],                    # 10
    ({"off": {"cand_prior": 1}, "null": ("mask_bits",)}, "must be 4-byte aligned"),
    ({}, "null handle"),                                                                # 11
    ({"dtype": BF16, "off": {"logits": 2}}, "null handle"),                             # a bf16 needs 2 bytes only
    ({"off": {"logits": 4, "cand_count": 4, "cand_actions": 4, "cand_prior": 4}}, "null handle"),  # float32 and int32 need 4
    ({"K": 1}, "null handle"),
    ({"K": 64}, "null handle"),
    ({"null": ("mask_bits",)}, "null handle"),                                          # 12 needs a handle: the null one is refused first
    ({"rows": 0}, "null handle"),                                                       # the null handle is refused before the no-op
    ({"rows": 2 ** 31 - 1}, "null handle"),
])
def test_argument_checks_need_no_device(kw, msg):
    rc, err = _call(**kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
