"""pcbenv_frontier_sample on the CPU side: include/pcbenv_frontier_sample.h declares it, its request struct and its contract,
libpcbenv.so exports it, pcbenv/_frontier_sample_lib.py binds it with a structure of the C struct's layout -- next to the
earlier headers and their bindings, which stay as they are -- and every argument check refuses what it must before anything
touches a device, in the order the header gives, the null handle last.  No compute call is made."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from abi_header import REPO, _STRUCT, _declarator
import model_harness
from pcbenv import _frontier_lib, _frontier_sample_lib, _lib, _search_lib

PATH = os.path.join(REPO, "include", "pcbenv_frontier_sample.h")
NAME = "pcbenv_frontier_sample"
SET_IN, SET_OUT = tuple(n + "_in" for n in _frontier_sample_lib.SAMPLE_SET), tuple(n + "_out" for n in _frontier_sample_lib.SAMPLE_SET)
OWN, SAMPLE, INPUTS = _frontier_lib.FRONTIER_OWN, _frontier_sample_lib.SAMPLE_OWN, _search_lib.PUCT_INPUTS
POINTERS = SET_IN + SET_OUT + OWN + SAMPLE + INPUTS + ("errors_dev", "stream")
INTS = ("phases", "num_roots", "width", "num_candidates", "max_steps", "first_root", "reserved")
MEMBERS = ("struct_size", "phases", "num_roots", "width", "num_candidates", "max_steps", "seed", "step_index", "first_root", "reserved") + POINTERS
INIT, ADVANCE = 1, 2


def _raw():
    with open(PATH) as f:
        return f.read()


def test_header_declares_the_function_the_struct_and_the_contract():
    raw = _raw()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r'#include\s+"pcbenv_frontier.h"', text) and "PCBENV_ABI_VERSION" not in text
    assert not re.findall(r"#define\s+(PCBENV_\w+)\s+(\d+)", text)  # the phases and the bounds are pcbenv_frontier.h's
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*const\s+pcbenv\s*\*\s*env\s*,\s*const\s+pcbenv_frontier_sample_request\s*\*\s*req\s*\)\s*;", text)
    assert len(re.findall(r"\b\w+\s*\([^()]*\)\s*;", text)) == 1  # one prototype
    (name, body), = re.findall(_STRUCT, text, flags=re.S)
    members = []
    for decl in filter(str.strip, body.split(";")):
        base = re.match(r"\s*((?:const\s+)?\w+)", decl)
        members += [_declarator(base.group(1) + " " + item) for item in decl[base.end():].split(",")]
    assert name == "pcbenv_frontier_sample_request" and tuple(n for _, n in members) == MEMBERS
    types = dict((n, t) for t, n in members)
    assert types["gumbel_in"] == "const double *" and types["gumbel_out"] == types["set_gumbel"] == types["set_logp"] == types["set_value"] == "double *"
    assert types["set_len"] == types["set_path"] == "int32_t *" and types["seed"] == types["step_index"] == "uint64_t" and types["first_root"] == "int32_t"
    block = re.sub(r"\s*\n \*\s*", " ", raw[:raw.index("typedef struct pcbenv_frontier_sample_request")].rsplit("/*", 1)[1])
    for phrase in ("one kernel launch on req->stream", "Enqueue only, no allocation, no synchronisation", "hipGraph", "both in one request is PCBENV_EINVAL",
                   "gumbel_out of slot 0 = 0.0 and set_len = -1 everywhere", "ORs bit 1 (value 2) into *errors_dev", "ORs bit 2 (value 4) into *errors_dev",
                   "the value is never read into a key", "a NaN counted as -inf", "-0.0 ties with +0.0", "on equal keys a set entry goes before a row",
                   "The first min(W, contenders) are the winners", "get set_len = -1 and nothing else", "the m-th lowest slot that is not a surviving entry",
                   "the last three copied as data", "draw number 256 + i_w of child c", "256 lies above every draw number", "Z the largest G_c over the children with finite phi_c",
                   "(G_S - max(v, 0)) - ln(1 + exp(-|v|))", "one IEEE operation per written operator", "no further guard is needed", "Exact maximum", "Final set",
                   "Dropped entries stay out", "Batch independence", "PCBENV_EINVAL (checked before any device call, in this order)",
                   "overlapping those of its out twin", "num_roots == 0 is a no-op success"):
        assert phrase in block, phrase
    assert "only enqueues" in raw.split("#ifndef PCBENV_FRONTIER_SAMPLE_H")[0] and "ABI version is pcbenv.h's and is unchanged" in re.sub(r"\s*\n \*\s*", " ", raw)


def test_exported_and_bound():
    L = _frontier_sample_lib.bind(_lib.load())
    assert _frontier_sample_lib.EXPORTS == (NAME,) and hasattr(L, NAME)
    assert len(getattr(L, NAME).argtypes) == 2 and getattr(L, NAME).restype is C.c_int
    assert all(NAME not in m.EXPORTS for m in (_lib, _search_lib, _frontier_lib))
    R = _frontier_sample_lib.PcbenvFrontierSampleRequest
    assert tuple(n for n, _ in R._fields_) == MEMBERS
    kinds = dict(struct_size=C.c_uint32, seed=C.c_uint64, step_index=C.c_uint64, **{n: C.c_void_p for n in POINTERS})
    for n, t in R._fields_:
        assert t is kinds.get(n, C.c_int32), n
    # csrc/pcb_frontier_sample.hip static_asserts the same figures of the struct as the library compiled it
    assert C.sizeof(R) == 248 and R.stream.offset == 240 and R.paths_in.offset == 48 and R.seed.offset == 24 and R.first_root.offset == 40
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3  # the ABI version is unchanged


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_header_compiles_as_c_and_the_ctypes_structure_has_its_layout():
    offsets, size = model_harness.layout("pcbenv_frontier_sample.h", "pcbenv_frontier_sample_request", MEMBERS)
    R = _frontier_sample_lib.PcbenvFrontierSampleRequest
    assert size == C.sizeof(R)
    assert offsets == {n: getattr(R, n).offset for n in MEMBERS}


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_rule_compiles_alone_for_the_host():
    """csrc/pcb_frontier_sample.h is plain C++17: a translation unit that holds nothing else compiles with every warning an error."""
    tmp = tempfile.mkdtemp(prefix="frontier_sample_alone_")
    src = os.path.join(tmp, "alone.cpp")
    with open(src, "w") as f:
        f.write('#include "pcb_frontier_sample.h"\nint main() { return pcb_frontier_sample::truncated(0.0, 0.0, 0.0) == 0.0 ? 0 : 1; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", model_harness.CSRC, "-o", os.path.join(tmp, "alone"), src], check=True)


# host memory, never dereferenced: every call below fails before a device is touched.  Every tensor has a region of its own,
# SPAN bytes apart, larger than any tensor of the default sizes (paths: T * P * W * K * 12 = 192 bytes).
SPAN = 1024
_HOST = (C.c_uint64 * (SPAN // 8 * (len(POINTERS) + 1)))()


def _address(name):
    return C.addressof(_HOST) + SPAN * POINTERS.index(name)


def _call(request=True, size=None, phases=ADVANCE, P=2, W=2, K=2, T=2, first_root=0, reserved=0, null=(), odd=(), at=None):
    L = _frontier_sample_lib.bind(_lib.load())
    R = _frontier_sample_lib.PcbenvFrontierSampleRequest
    req = R(struct_size=C.sizeof(R) if size is None else size, phases=phases, num_roots=P, width=W, num_candidates=K, max_steps=T, seed=1, step_index=2,
            first_root=first_root, reserved=reserved)
    for name in SET_IN + SET_OUT + OWN + SAMPLE + INPUTS:  # errors_dev and stream stay null: both are optional
        if name not in null:
            setattr(req, name, _address(name) + (4 if name in odd else 2 if name + "/2" in odd else 0))
    for name, (other, offset) in (at or {}).items():
        setattr(req, name, _address(other) + offset)
    rc = getattr(L, NAME)(None, C.byref(req) if request else None)
    return rc, L.pcbenv_last_error(None).decode()


OUT_NULL = "null paths_out, path_len_out, cum_logp_out, gumbel_out, parent_row, live, best_value, best_len, set_len, set_gumbel, set_logp, set_value or set_path"
IN_NULL = "null paths_in, path_len_in, cum_logp_in, gumbel_in, best_path, value, leaf_terminal, cand_count, cand_actions or cand_prior with ADVANCE"
FIRST_ROOT = "first_root must not be negative and first_root + num_roots must not exceed 2^31 - 1"
TWIN = "an in tensor overlaps its out twin"
ALIGNED = "the float64 tensors must be 8-byte aligned"
# every check, in the order the header gives: each row is refused with its message although everything behind it in the
# order is wrong as well where that can be arranged (the null handle always is)
CHECKS = [
    (dict(request=False), "null request"),
    (dict(size=244, phases=0), "struct_size"),
    (dict(size=184), "struct_size"),  # pcbenv_frontier_request's
    (dict(phases=0, P=-1), "phases must be INIT or ADVANCE"),
    (dict(phases=4), "phases must be INIT or ADVANCE"),
    (dict(phases=INIT | ADVANCE | 8), "phases must be INIT or ADVANCE"),
    (dict(phases=INIT | ADVANCE, P=-1), "INIT cannot be combined with ADVANCE"),
    (dict(P=-1, W=0), "num_roots must not be negative"),
    (dict(W=0, K=0), "width must be in [1, 64]"),
    (dict(W=65), "width must be in [1, 64]"),
    (dict(K=0, T=0), "num_candidates must be in [1, 64]"),
    (dict(K=65), "num_candidates must be in [1, 64]"),
    (dict(W=17, K=61, T=0), "width * num_candidates must not exceed 1024"),
    (dict(T=0, first_root=-1), "max_steps must be at least 1"),
    (dict(P=2 ** 21, W=32, K=32, first_root=-1), "num_roots * width * num_candidates must not exceed 2^31 - 1"),
    (dict(first_root=-1, reserved=1), FIRST_ROOT),
    (dict(first_root=2 ** 31 - 2, P=2), FIRST_ROOT),
    (dict(reserved=1, null=("live",)), "reserved must be 0"),
    (dict(reserved=-1), "reserved must be 0"),
] + [(dict(null=(n, "value"), phases=ph), OUT_NULL) for n in SET_OUT + OWN[:4] + SAMPLE for ph in (INIT, ADVANCE)] + [
    (dict(null=(n,), odd=("value",)), IN_NULL) for n in SET_IN + ("best_path",) + INPUTS
] + [
    (dict(odd=(n,), at={"paths_in": ("paths_out", 0)}), ALIGNED) for n in ("cum_logp_in", "gumbel_in", "cum_logp_out", "gumbel_out", "best_value", "set_gumbel", "set_logp", "set_value", "value")
] + [(dict(odd=(n,), phases=INIT), ALIGNED) for n in ("cum_logp_out", "gumbel_out", "best_value", "set_gumbel", "set_logp", "set_value")] + [
    (dict(odd=("cand_prior/2",), at={"paths_in": ("paths_out", 0)}), "cand_prior must be 4-byte aligned"),
    # the twins: the same address, the in tensor ending inside the out tensor, and beginning inside it (paths: 192 bytes, path_len 32, cum_logp and gumbel 64)
    (dict(at={"paths_in": ("paths_out", 0)}), TWIN),
    (dict(at={"paths_in": ("paths_out", -188)}), TWIN),
    (dict(at={"path_len_in": ("path_len_out", 28)}), TWIN),
    (dict(at={"cum_logp_in": ("cum_logp_out", 56)}), TWIN),
    (dict(at={"gumbel_in": ("gumbel_out", 0)}), TWIN),
    (dict(at={"gumbel_in": ("gumbel_out", -56)}), TWIN),
    (dict(at={"gumbel_out": ("gumbel_in", 56)}), TWIN),
    # the last of the order: everything is right but the handle -- and tensors that only touch do not overlap
    (dict(), "null handle"),
    (dict(phases=INIT), "null handle"),
    (dict(phases=INIT, null=SET_IN + ("best_path",) + INPUTS), "null handle"),   # INIT needs the out set and the sample set alone
    (dict(phases=INIT, odd=("cum_logp_in", "gumbel_in", "value", "cand_prior/2")), "null handle"),  # and looks at nothing else
    (dict(phases=INIT, at={"gumbel_in": ("gumbel_out", 0), "paths_in": ("paths_out", 0)}), "null handle"),
    (dict(at={"gumbel_in": ("gumbel_out", 64)}), "null handle"),
    (dict(at={"gumbel_in": ("gumbel_out", -64)}), "null handle"),
    (dict(P=0, null=("set_len",)), OUT_NULL),   # num_roots == 0 is a success only behind every check
    (dict(P=0), "null handle"),
    (dict(W=64, K=16, P=1, T=1, phases=INIT), "null handle"),  # the limits themselves are in range
    (dict(first_root=2 ** 31 - 3, P=2), "null handle"),
]


def test_the_table_is_the_whole_of_it():
    messages = {msg for _, msg in CHECKS}
    raw = re.sub(r"\s*\n \*\s*", " ", _raw())
    order = raw[raw.index("PCBENV_EINVAL (checked before any device call, in this order)"):]
    steps = ("null request", "struct_size not", "phases 0 or with unknown bits", "INIT together with ADVANCE", "num_roots < 0", "width outside", "num_candidates outside",
             "width * num_candidates above", "max_steps < 1", "num_roots * width * num_candidates above", "first_root < 0 or first_root + num_roots above", "reserved != 0",
             "a null tensor among paths_out", "a null tensor among paths_in", "not 8-byte aligned", "not 4-byte aligned", "overlapping those of its out twin", "null handle")
    at = [order.index(s) for s in steps]
    assert at == sorted(at)  # the header states the order the table walks
    assert len(messages) == 18 and len(CHECKS) >= 80


@pytest.mark.parametrize("kw, msg", CHECKS)
def test_argument_checks_need_no_device(kw, msg):
    rc, err = _call(**kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
