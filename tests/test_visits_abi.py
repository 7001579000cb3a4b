"""pcbenv_evaluate_visits / pcbenv_evaluate_visits_backward on the CPU side: include/pcbenv_train.h declares them, their
request struct and their contract, libpcbenv.so exports them, pcbenv/_train_lib.py binds them with a structure of the C
struct's layout -- next to include/pcbenv.h, pcbenv_search.h, pcbenv_priors.h, pcbenv_move.h and their binding modules,
which stay as they are -- and every argument check refuses what it must before anything touches a device, in the order the
header gives, the null handle last.  No compute call is made."""
import ctypes as C
import os
import re
import shutil

import pytest

import abi_header
from abi_header import REPO, _STRUCT, _declarator
import model_harness
from pcbenv import _lib, _move_lib, _priors_lib, _search_lib, _train_lib

PATH = os.path.join(REPO, "include", "pcbenv_train.h")
INPUTS = ("logits", "mask_bits", "visits", "target_actions")
POINTERS = INPUTS + ("cross_entropy", "entropy", "stats", "errors_dev", "grad_cross_entropy", "grad_entropy", "grad_logits", "stream")
MEMBERS = ("struct_size", "logits_dtype", "action_format", "num_targets", "num_rows", "reserved") + POINTERS
CTYPES = {"struct_size": "uint32_t", "logits_dtype": "int32_t", "action_format": "int32_t", "num_targets": "int32_t", "num_rows": "int64_t",
          "reserved": "int64_t", "logits": "const void *", "mask_bits": "const uint64_t *", "visits": "const int32_t *",
          "target_actions": "const int32_t *", "cross_entropy": "float *", "entropy": "float *", "stats": "float *", "errors_dev": "uint32_t *",
          "grad_cross_entropy": "const float *", "grad_entropy": "const float *", "grad_logits": "void *", "stream": "void *"}
CALLS = ("pcbenv_evaluate_visits", "pcbenv_evaluate_visits_backward")


def _raw():
    with open(PATH) as f:
        return f.read()


def _text():
    return re.sub(r"/\*.*?\*/", "", _raw(), flags=re.S)


def _members():
    (name, body), = re.findall(_STRUCT, _text(), flags=re.S)
    assert name == "pcbenv_visits_request"
    out = []
    for decl in filter(str.strip, body.split(";")):
        base = re.match(r"\s*((?:const\s+)?\w+)", decl)
        out += [_declarator(base.group(1) + " " + item) for item in decl[base.end():].split(",")]
    return out


def test_header_declares_the_functions_the_struct_and_the_contract():
    raw, text = _raw(), _text()
    assert re.search(r'#include\s+"pcbenv.h"', text) and "PCBENV_ABI_VERSION" not in raw  # the version is pcbenv.h's, and stays 3
    for name in CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*const\s+pcbenv\s*\*\s*env\s*,\s*const\s+pcbenv_visits_request\s*\*\s*req\s*\)\s*;", text)
    assert len(re.findall(r"\b\w+\s*\([^()]*\)\s*;", text)) == 2  # two prototypes
    members = _members()
    assert tuple(n for _, n in members) == MEMBERS
    assert {n: t for t, n in members} == CTYPES
    assert not re.search(r"#define\s+PCBENV_", text.replace("#define PCBENV_TRAIN_H", ""))  # dtypes, formats and the limit of C are pcbenv.h's
    block = re.sub(r"\s*\n \*\s*", " ", raw[:raw.index("typedef struct pcbenv_visits_request")].rsplit("/*", 1)[1])
    for phrase in ("one kernel launch on req->stream each", "Enqueue only, no allocation, no synchronisation", "hipGraph",
                   "Rows are independent and num_rows is arbitrary", "no bound buffers are needed", "orientation o reads plane o & 1",
                   "the square kind reads plane 0 only", "bits of columns >= W are ignored", "An illegal logit is never read",
                   "exactly the tensors pcbenv_puct_move CHOOSE writes", "valid if visits[c] > 0, its action is in range and its bit is set",
                   "T is the int64 sum of the valid visits", "pi_c = (double)visits[c] / (double)T",
                   "cross_entropy = log Z - sum over the valid entries of pi_c (l_c - M)", "formed in float64, rounded once to float32",
                   "Entries with the same action add up", "makes the cross entropy +inf", "(M, log Z, entropy, row status), 16-byte aligned",
                   "0 (ROW_OK), 1 (ROW_ZERO", "2 (ROW_NO_TARGET", "may be NULL", "Writes every element of grad_logits",
                   "round to nearest even", "each exactly once", "g_i = g_ce (p_i - pi_i) - g_H p_i (log p_i + Hrow)", "either may be NULL, which means zero",
                   "no legal action:", "a legal NaN or +inf:", "bit 0 (value 1)", "every legal logit -inf:", "bit 1 (value 2)", "visits[c] == 0:",
                   "bit 2 (value 4)", "T == 0:", "the g_ce term dropped", "The forward call ORs the bits into *errors_dev",
                   "PCBENV_EINVAL (checked before any device call, in this order)", "[1, PCBENV_MAX_TREE_CHILDREN]", "num_rows == 0 is a no-op success"):
        assert phrase in block, phrase
    assert "only enqueues" in raw.split("#ifndef PCBENV_TRAIN_H")[0]


def test_the_other_headers_and_bindings_are_as_they_were():
    assert len(abi_header.prototypes()) == 40 and len(abi_header.structs()) == 6
    for header in ("pcbenv.h", "pcbenv_search.h", "pcbenv_priors.h", "pcbenv_move.h"):
        with open(os.path.join(REPO, "include", header)) as f:
            assert "evaluate_visits" not in f.read(), header
    assert len(_lib.EXPORTS) == 40 and _search_lib.EXPORTS == ("pcbenv_puct_advance",)
    assert _priors_lib.EXPORTS == ("pcbenv_top_priors",) and _move_lib.EXPORTS == ("pcbenv_puct_move",)
    assert not [n for m in (_lib, _search_lib, _priors_lib, _move_lib) for n in vars(m) if "visits" in n.lower() and n != "MOVE_OUTPUTS"]
    assert re.search(r"#define\s+PCBENV_ABI_VERSION\s+3\b", abi_header.text())


def test_exported_and_bound():
    L = _train_lib.bind(_lib.load())
    assert _train_lib.EXPORTS == CALLS
    R = _train_lib.PcbenvVisitsRequest
    for name in CALLS:
        f = getattr(L, name)
        assert len(f.argtypes) == 2 and f.restype is C.c_int
    assert tuple(n for n, _ in R._fields_) == MEMBERS
    kinds = dict(struct_size=C.c_uint32, num_rows=C.c_int64, reserved=C.c_int64, **{n: C.c_void_p for n in POINTERS})
    for n, t in R._fields_:
        assert t is kinds.get(n, C.c_int32), n
    # csrc/pcb_policy_visits.hip static_asserts the same two figures of the struct as the library compiled it
    assert C.sizeof(R) == 128 and R.stream.offset == 120 and R.num_rows.offset == 16
    assert (_train_lib.ROW_OK, _train_lib.ROW_ZERO, _train_lib.ROW_NO_TARGET) == (0, 1, 2)
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3


def test_bind_refuses_a_library_without_the_symbols():
    class Without:
        pass
    with pytest.raises(ImportError, match="pcbenv_evaluate_visits"):
        _train_lib.bind(Without())


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_ctypes_structure_has_the_c_layout():
    """A compiled probe: sizeof and every member's offset as a C compiler lays include/pcbenv_train.h out."""
    offsets, size = model_harness.layout("pcbenv_train.h", "pcbenv_visits_request", MEMBERS)
    R = _train_lib.PcbenvVisitsRequest
    assert size == C.sizeof(R)
    assert offsets == {n: getattr(R, n).offset for n in MEMBERS}


_HOST = (C.c_uint64 * 8)()  # host memory: never dereferenced, every call below fails before a device is touched
F32, BF16 = _lib.LOGITS_F32, _lib.LOGITS_BF16
GIVEN = INPUTS + ("stats", "grad_logits")


def _call(backward, request=True, size=None, dtype=F32, fmt=_lib.ACTION_TUPLE, C_=16, reserved=0, rows=8, null=(), off=None):
    """off: {member: byte offset from a 16-byte boundary}.  The inputs, stats and grad_logits are given unless in `null`;
    every other pointer stays null: all of them are optional."""
    L = _train_lib.bind(_lib.load())
    R = _train_lib.PcbenvVisitsRequest
    req = R(struct_size=C.sizeof(R) if size is None else size, logits_dtype=dtype, action_format=fmt, num_targets=C_, num_rows=rows, reserved=reserved)
    base = (C.addressof(_HOST) + 15) & ~15
    for n in GIVEN:
        if n not in null:
            setattr(req, n, base + (off or {}).get(n, 0))
    f = L.pcbenv_evaluate_visits_backward if backward else L.pcbenv_evaluate_visits
    rc = f(None, C.byref(req) if request else None)
    return rc, L.pcbenv_last_error(None).decode()


BOTH = [
    ({"request": False}, "null request"),                                               # 1
    ({"size": 0}, "struct_size"),                                                       # 2
    ({"size": 120, "dtype": 9}, "struct_size"),                                         # the order: the size before any field is believed
    ({"size": 136, "C_": 0}, "struct_size"),
    ({"dtype": 2}, "unknown logits dtype"),                                             # 3
    ({"dtype": -1, "fmt": 7}, "unknown logits dtype"),
    ({"fmt": 2}, "unknown action format"),                                              # 4
    ({"fmt": -1, "C_": 0}, "unknown action format"),
    ({"C_": 0}, "num_targets"),                                                         # 5
    ({"C_": 65, "rows": -1}, "num_targets"),
    ({"C_": -1}, "num_targets"),
    ({"rows": -1}, "num_rows"),                                                         # 6
    ({"rows": -5, "reserved": 1}, "num_rows"),
    ({"rows": 2 ** 31}, "num_rows"),
    ({"reserved": 1}, "reserved"),                                                      # 7
    ({"reserved": -1, "null": ("logits",)}, "reserved"),
    *[({"null": (n,)}, "null logits, mask_bits, visits or target_actions") for n in INPUTS],   # 8
    ({"null": ("visits",), "off": {"logits": 2}}, "null logits, mask_bits"),
    ({"off": {"logits": 2}}, "logits pointer not aligned"),                             # 10
    ({"off": {"logits": 1}, "dtype": BF16}, "logits pointer not aligned"),
    ({"off": {"logits": 6, "mask_bits": 4}}, "logits pointer not aligned"),
    ({"off": {"mask_bits": 4}}, "mask bits pointer not aligned"),                       # 11
    ({"off": {"mask_bits": 1, "visits": 2}}, "mask bits pointer not aligned"),
    ({"off": {"visits": 2}}, "must be 4-byte aligned"),                                 # 12
    ({"off": {"target_actions": 1, "stats": 4}}, "must be 4-byte aligned"),
    ({"off": {"stats": 8}}, "stats pointer not aligned"),                               # 13
    ({"off": {"stats": 4, "grad_logits": 1}}, "stats pointer not aligned"),
    ({}, "null handle"),                                                                # 15
    ({"dtype": BF16, "off": {"logits": 2}}, "null handle"),                             # a bf16 needs 2 bytes only
    ({"off": {"logits": 4, "visits": 4, "target_actions": 12, "mask_bits": 8}}, "null handle"),
    ({"C_": 1}, "null handle"),
    ({"C_": 64, "fmt": _lib.ACTION_FLAT}, "null handle"),
    ({"rows": 0}, "null handle"),                                                       # the null handle is refused before the no-op
    ({"rows": 2 ** 31 - 1}, "null handle"),
]
FORWARD_ONLY = [
    ({"null": ("stats",)}, "null handle"),                                              # optional in the forward call
    ({"null": ("grad_logits",)}, "null handle"),                                        # not read by it
    ({"off": {"grad_logits": 1}}, "null handle"),
]
BACKWARD_ONLY = [
    ({"null": ("stats",)}, "null stats or grad_logits"),                                # 9
    ({"null": ("grad_logits",), "off": {"logits": 2}}, "null stats or grad_logits"),
    ({"null": ("stats", "logits")}, "null logits, mask_bits"),
    ({"off": {"grad_logits": 2}}, "grad logits pointer not aligned"),                   # 14
    ({"off": {"grad_logits": 1}, "dtype": BF16}, "grad logits pointer not aligned"),
    ({"off": {"grad_logits": 2}, "dtype": BF16}, "null handle"),
]


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("kw, msg", BOTH)
def test_argument_checks_need_no_device(kw, msg, backward):
    rc, err = _call(backward, **kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err


@pytest.mark.parametrize("backward, kw, msg", [(False, k, m) for k, m in FORWARD_ONLY] + [(True, k, m) for k, m in BACKWARD_ONLY])
def test_argument_checks_of_one_call(backward, kw, msg):
    rc, err = _call(backward, **kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
