"""pcbenv_gumbel_advance on the CPU side: include/pcbenv_gumbel.h declares it, its request struct and its contract,
libpcbenv.so exports it, pcbenv/_gumbel_lib.py binds it with a structure of the C struct's layout -- next to
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
from pcbenv import _gumbel_lib, _lib, _move_lib, _noise_lib, _search_lib

PATH = os.path.join(REPO, "include", "pcbenv_gumbel.h")
TREE, EXCHANGE, INPUTS = _search_lib.PUCT_TREE_TENSORS, _search_lib.PUCT_EXCHANGE, _search_lib.PUCT_INPUTS
BUDGET, OUTPUTS = _gumbel_lib.GUMBEL_BUDGET, _gumbel_lib.GUMBEL_OUTPUTS
POINTERS = TREE + EXCHANGE + INPUTS + BUDGET + OUTPUTS + ("errors_dev", "stream")
INTS = ("phases", "num_roots", "capacity", "max_children", "max_steps", "num_candidates", "num_simulations", "max_considered", "first_root", "reserved")
DOUBLES = ("c_puct", "c_visit", "c_scale")
MEMBERS = ("struct_size",) + INTS + DOUBLES + ("seed", "step_index") + POINTERS
OWN = {"sim_index": "int32_t *", "sim_visits": "int32_t *", "considered": "const int32_t *", "move_slot": "int32_t *", "move_action": "int32_t *",
       "child_weights": "int32_t *", "child_policy": "float *", "child_actions": "int32_t *", "root_value": "double *"}
BEGIN, ABSORB, SELECT, CHOOSE = 1, 2, 4, 8


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
    assert re.search(r"\bint\s+pcbenv_gumbel_advance\s*\(\s*const\s+pcbenv\s*\*\s*env\s*,\s*const\s+pcbenv_gumbel_request\s*\*\s*req\s*\)\s*;", text)
    assert len(re.findall(r"\b\w+\s*\([^()]*\)\s*;", text)) == 1  # one prototype
    for name, bit in (("BEGIN", 1), ("ABSORB", 2), ("SELECT", 4), ("CHOOSE", 8)):
        assert re.search(rf"#define\s+PCBENV_GUMBEL_{name}\s+{bit}\b", text)
    assert (_gumbel_lib.GUMBEL_BEGIN, _gumbel_lib.GUMBEL_ABSORB, _gumbel_lib.GUMBEL_SELECT, _gumbel_lib.GUMBEL_CHOOSE) == (1, 2, 4, 8)
    members = _members(text, "pcbenv_gumbel_request")
    assert tuple(n for _, n in members) == MEMBERS
    # the tree and exchange tensors have pcbenv_puct_request's names and types, in its order
    with open(os.path.join(REPO, "include", "pcbenv_search.h")) as f:
        base = _members(re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S), "pcbenv_puct_request")
    shared = [(t, n) for t, n in base if n in TREE + EXCHANGE + INPUTS]
    assert [(t, n) for t, n in members if n in TREE + EXCHANGE + INPUTS] == shared and len(shared) == 21
    types = {n: t for t, n in members}
    assert {n: types[n] for n in OWN} == OWN
    assert types["struct_size"] == "uint32_t" and all(types[n] == "int32_t" for n in INTS) and all(types[n] == "double" for n in DOUBLES)
    assert types["seed"] == types["step_index"] == "uint64_t" and types["errors_dev"] == "uint32_t *" and types["stream"] == "void *"
    block = re.sub(r"\s*\n \*\s*", " ", raw[:raw.index("typedef struct pcbenv_gumbel_request")].rsplit("/*", 1)[1])
    for phrase in ("one kernel launch on req->stream", "nothing the library owns is read or written", "no bound buffers",
                   "Enqueue only, no allocation, no synchronisation", "hipGraph", "runs them in that order", "before they address anything",
                   "mix64(mix64(seed ^ 0x9E3779B97F4A7C15 * (first_root + p + 1)) + step_index)", "(64 * 128 + c + 1)", "((w >> 12) + 0.5) * 2^-52",
                   "g_c = -ln(-ln u)", "use the numbers 0 .. 96", "never on P, on C or on the other children",
                   "prior(ch) > 2^-149 ? (prior(ch) < 1 ? prior(ch) : 1) : 2^-149", "vbar = visits(0) > 0 ? value_sum(0) / visits(0) : reward_lo",
                   "qhat_c = range ? ((n_c > 0 ? value_sum(ch) / n_c : vbar) - reward_lo) / (reward_hi - reward_lo) : 0",
                   "sigma_c = ((c_visit + (double)max_b n_b) * c_scale) * qhat_c", "score_c = (g_c + logit_c) + sigma_c", "IEEE + - * / alone",
                   "exp only sees arguments <= 0", "sim_index[p] = 0 and sim_visits[p, :] = 0", "word for word", "consumes no simulation",
                   "t < 0: bit 1 is ORed", "nothing else is stored", "t >= n: level 0 is chosen by pcbenv_puct_advance's rule",
                   "v = considered[m * n + t]", "or all k children if there is none", "ties to the lowest c", "sim_visits[p, c*] += 1, sim_index[p] = t + 1",
                   "it never stores to the tree", "extra = max(1, n / (e * nc))", "nc = max(2, nc / 2)", "0 0 0 0 1 1 2 2", "it never addresses with one",
                   "move_slot = -1, move_action = 0", "vmax = max_c sim_visits[p, c]", "summed in that order", "pi_c = e_c / Z",
                   "(int32)(pi_c * 16777216.0 + 0.5)", "Every element of the six outputs is written", "because it divides by the integer sum",
                   "PCBENV_EINVAL (checked before any device call, in this order)", "CHOOSE together with SELECT", "num_roots == 0 is a no-op success"):
        assert phrase in block, phrase
    assert "only enqueues" in raw.split("#ifndef PCBENV_GUMBEL_H")[0]


def test_exported_and_bound():
    L = _gumbel_lib.bind(_lib.load())
    assert _gumbel_lib.EXPORTS == ("pcbenv_gumbel_advance",) and hasattr(L, "pcbenv_gumbel_advance")
    assert len(L.pcbenv_gumbel_advance.argtypes) == 2 and L.pcbenv_gumbel_advance.restype is C.c_int
    assert all("pcbenv_gumbel_advance" not in m.EXPORTS for m in (_lib, _search_lib, _move_lib, _noise_lib))
    R = _gumbel_lib.PcbenvGumbelRequest
    assert tuple(n for n, _ in R._fields_) == MEMBERS
    kinds = dict(struct_size=C.c_uint32, seed=C.c_uint64, step_index=C.c_uint64, **{n: C.c_double for n in DOUBLES}, **{n: C.c_void_p for n in POINTERS})
    for n, t in R._fields_:
        assert t is kinds.get(n, C.c_int32), n
    # csrc/pcb_gumbel.hip static_asserts the same figures of the struct as the library compiled it
    assert C.sizeof(R) == 344 and R.stream.offset == 336 and R.c_puct.offset == 48 and R.seed.offset == 72 and R.num_nodes.offset == 88
    assert R.sim_index.offset == 256 and R.move_slot.offset == 280
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_ctypes_structure_has_the_c_layout():
    """A compiled probe: sizeof and every member's offset as a C compiler lays include/pcbenv_gumbel.h out."""
    offsets, size = model_harness.layout("pcbenv_gumbel.h", "pcbenv_gumbel_request", MEMBERS)
    R = _gumbel_lib.PcbenvGumbelRequest
    assert size == C.sizeof(R)
    assert offsets == {n: getattr(R, n).offset for n in MEMBERS}


_HOST = (C.c_uint64 * 8)()  # host memory: never dereferenced, every call below fails before a device is touched
ALL = BEGIN | ABSORB | SELECT


def _call(request=True, size=None, phases=ALL, P=8, N=5, Cc=3, T=4, K=2, n=8, Mc=4, reserved=0, c_visit=50.0, c_scale=1.0, null=(), odd=()):
    L = _gumbel_lib.bind(_lib.load())
    R = _gumbel_lib.PcbenvGumbelRequest
    req = R(struct_size=C.sizeof(R) if size is None else size, phases=phases, num_roots=P, capacity=N, max_children=Cc, max_steps=T, num_candidates=K,
            num_simulations=n, max_considered=Mc, reserved=reserved, c_puct=1.0, c_visit=c_visit, c_scale=c_scale)
    for name in TREE + EXCHANGE + INPUTS + BUDGET + OUTPUTS:  # errors_dev and stream stay null: both are optional
        if name not in null:
            setattr(req, name, C.addressof(_HOST) + (4 if name in odd else 2 if name + "/2" in odd else 0))
    rc = L.pcbenv_gumbel_advance(None, C.byref(req) if request else None)
    return rc, L.pcbenv_last_error(None).decode()


NAN, INF = math.nan, math.inf


@pytest.mark.parametrize("kw, msg", [
    ({"request": False}, "null request"),                                                   # 1
    ({"size": 0}, "struct_size"),                                                           # 2
    ({"size": 224, "phases": 0}, "struct_size"),                                            # pcbenv_puct_request's size is not this struct's
    ({"phases": 0}, "phases must be a non-empty set of BEGIN, ABSORB, SELECT, CHOOSE"),     # 3
    ({"phases": 16, "P": -1}, "phases must be"),
    ({"phases": -1}, "phases must be"),
    ({"phases": SELECT | CHOOSE, "P": -1}, "CHOOSE cannot be combined with SELECT"),
    ({"phases": 15}, "CHOOSE cannot be combined with SELECT"),
    ({"P": -1, "N": 0}, "num_roots must not be negative"),                                  # 4
    ({"N": 0, "Cc": 0}, "capacity"),                                                        # 5
    ({"Cc": 0, "T": 0}, "max_children"),                                                    # 6
    ({"Cc": 65}, "max_children"),
    ({"T": 0, "K": 0}, "max_steps"),                                                        # 7
    ({"K": 0, "n": 0}, "num_candidates must be at least 1 with ABSORB"),                    # 8
    ({"phases": BEGIN | SELECT, "K": 0, "n": 0}, "num_simulations"),                        # only with ABSORB
    ({"n": 0, "Mc": 0}, "num_simulations must be at least 1"),                              # 9
    ({"n": -3}, "num_simulations"),
    ({"Mc": 0, "reserved": 1}, "max_considered must be in [1, 64]"),                        # 10
    ({"Mc": 65}, "max_considered"),
    ({"reserved": 1, "c_visit": NAN}, "reserved"),                                          # 11
    ({"c_visit": NAN}, "c_visit and c_scale must be finite and not negative"),              # 12
    ({"c_visit": -1e-9}, "c_visit and c_scale"),
    ({"c_visit": INF}, "c_visit and c_scale"),
    ({"c_scale": NAN, "null": ("prior",)}, "c_visit and c_scale"),
    ({"c_scale": -1.0}, "c_visit and c_scale"),
    ({"c_scale": INF}, "c_visit and c_scale"),
    *[({"null": (name,), "phases": ph}, "null tree tensor") for name in TREE for ph in (BEGIN, CHOOSE)],   # 13
    ({"null": ("prior", "sim_index")}, "null tree tensor"),
    *[({"null": (name,), "phases": ph}, "null sim_index or sim_visits") for name in ("sim_index", "sim_visits") for ph in (BEGIN, SELECT, CHOOSE)],  # 14
    ({"null": ("sim_index", "selected")}, "null sim_index or sim_visits"),
    ({"null": ("selected",), "phases": ABSORB}, "null selected"),                           # 15
    ({"null": ("selected", "paths"), "phases": SELECT}, "null selected"),
    *[({"null": (name,), "phases": SELECT}, "null path_len, paths or considered with SELECT") for name in ("path_len", "paths", "considered")],  # 16
    ({"null": ("considered", "value")}, "null path_len, paths or considered"),
    *[({"null": (name,), "phases": ABSORB}, "null value, leaf_terminal, cand_count, cand_actions or cand_prior with ABSORB") for name in INPUTS],  # 17
    *[({"null": (name,), "phases": CHOOSE}, "null move_slot, move_action, child_weights, child_policy, child_actions or root_value with CHOOSE")
      for name in OUTPUTS],                                                                 # 18
    ({"null": ("root_value",), "phases": CHOOSE, "odd": ("prior",)}, "null move_slot"),
    *[({"odd": (name,), "phases": BEGIN}, "8-byte aligned") for name in ("prior", "value_sum", "value_max", "reward_lo", "reward_hi")],  # 19
    ({"odd": ("value", "cand_prior/2")}, "8-byte aligned"),
    ({"odd": ("root_value", "child_policy/2"), "phases": CHOOSE}, "8-byte aligned"),
    ({"odd": ("cand_prior/2",)}, "cand_prior must be 4-byte aligned"),                       # 20
    ({"odd": ("child_policy/2",), "phases": CHOOSE | ABSORB}, "child_policy must be 4-byte aligned"),
    ({}, "null handle"),                                                                    # 21
    ({"phases": CHOOSE | BEGIN | ABSORB}, "null handle"),
    ({"c_visit": 0.0, "c_scale": 0.0, "Mc": 64, "Cc": 64, "n": 1}, "null handle"),          # the ends of the ranges are in
    ({"phases": BEGIN, "null": EXCHANGE + INPUTS + OUTPUTS + ("considered",), "K": 0}, "null handle"),  # what a phase does not use may be null
    ({"phases": ABSORB, "null": ("path_len", "paths") + BUDGET + OUTPUTS}, "null handle"),
    ({"phases": SELECT, "null": INPUTS + OUTPUTS, "K": 0}, "null handle"),
    ({"phases": CHOOSE, "null": EXCHANGE + INPUTS + ("considered",), "K": 0}, "null handle"),
    ({"odd": ("value",), "phases": SELECT}, "null handle"),                                 # value is not read without ABSORB
    ({"odd": ("root_value", "child_policy/2"), "phases": SELECT}, "null handle"),
    ({"odd": ("num_nodes", "parent", "sim_index", "sim_visits", "considered", "selected", "cand_prior", "child_policy")}, "null handle"),  # 4 bytes suffice
    ({"P": 0}, "null handle"),                                                              # the null handle is refused before the no-op
])
def test_argument_checks_need_no_device(kw, msg):
    rc, err = _call(**kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
