"""pcbenv_gumbel_advance_leaves on the CPU side: include/pcbenv_gumbel_leaves.h declares it, its request struct and its
contract, libpcbenv.so exports it, pcbenv/_gumbel_leaves_lib.py binds it with a structure of the C struct's layout -- next to
the earlier headers and their bindings, which stay as they are -- and every argument check refuses what it must before
anything touches a device, in the order the header gives, the null handle last.  No compute call is made."""
import ctypes as C
import math
import os
import re
import shutil

import pytest

from abi_header import REPO, _STRUCT, _declarator
import model_harness
from pcbenv import _gumbel_leaves_lib, _gumbel_lib, _leaves_lib, _lib, _move_lib, _noise_lib, _search_lib

PATH = os.path.join(REPO, "include", "pcbenv_gumbel_leaves.h")
TREE, EXCHANGE, INPUTS = _leaves_lib.LEAVES_TREE_TENSORS, _search_lib.PUCT_EXCHANGE, _search_lib.PUCT_INPUTS
BUDGET, OUTPUTS = _gumbel_lib.GUMBEL_BUDGET, _gumbel_lib.GUMBEL_OUTPUTS
POINTERS = TREE + EXCHANGE + INPUTS + BUDGET + OUTPUTS + ("errors_dev", "stream")
INTS = ("phases", "num_roots", "capacity", "max_children", "max_steps", "num_candidates", "num_simulations", "max_considered", "first_root", "reserved")
DOUBLES = ("c_puct", "c_visit", "c_scale")
MEMBERS = ("struct_size",) + INTS + DOUBLES + ("seed", "step_index", "num_leaves", "reserved2") + POINTERS
BEGIN, ABSORB, SELECT, CHOOSE = 1, 2, 4, 8


def _raw():
    with open(PATH) as f:
        return f.read()


def _members(path, struct):
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    (name, body), = re.findall(_STRUCT, text, flags=re.S)
    assert name == struct
    out = []
    for decl in filter(str.strip, body.split(";")):
        base = re.match(r"\s*((?:const\s+)?\w+)", decl)
        out += [_declarator(base.group(1) + " " + item) for item in decl[base.end():].split(",")]
    return out


def test_header_declares_the_function_the_struct_and_the_contract():
    raw = _raw()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r'#include\s+"pcbenv_gumbel.h"', text) and re.search(r'#include\s+"pcbenv_leaves.h"', text) and "PCBENV_ABI_VERSION" not in text
    assert "#define" not in text.replace("#define PCBENV_GUMBEL_LEAVES_H", "")  # the phases and the bound on L are the earlier headers'
    assert re.search(r"\bint\s+pcbenv_gumbel_advance_leaves\s*\(\s*const\s+pcbenv\s*\*\s*env\s*,\s*const\s+pcbenv_gumbel_leaves_request\s*\*\s*req\s*\)\s*;", text)
    assert len(re.findall(r"\b\w+\s*\([^()]*\)\s*;", text)) == 1  # one prototype
    members = _members(PATH, "pcbenv_gumbel_leaves_request")
    assert tuple(n for _, n in members) == MEMBERS
    # pcbenv_gumbel_request's members with their types, in its order, plus num_leaves, reserved2 and pending as pcbenv_puct_leaves_request has them
    base = _members(os.path.join(REPO, "include", "pcbenv_gumbel.h"), "pcbenv_gumbel_request")
    leaves = {n: t for t, n in _members(os.path.join(REPO, "include", "pcbenv_leaves.h"), "pcbenv_puct_leaves_request")}
    more = ("num_leaves", "reserved2", "pending")
    assert [(t, n) for t, n in members if n not in more] == base
    assert {n: t for t, n in members if n in more} == {n: leaves[n] for n in more}
    block = re.sub(r"\s*\n \*\s*", " ", raw[:raw.index("typedef struct pcbenv_gumbel_leaves_request")].rsplit("/*", 1)[1])
    for phrase in ("One kernel launch on req->stream", "Enqueue only, no allocation, no synchronisation", "hipGraph", "runs them in that order",
                   "row r = p * L + l is leaf l of root p", "word for word and bit for bit", "BEGIN does not touch pending and CHOOSE does not read it",
                   "a row with selected == -1 skipped and none of its inputs read", "pending -= 1 on every node of each backup chain",
                   "never pending", "they are the same for every leaf of a launch", "leaf 0 gets selected = 0, path_len = 0 and pending(0) += 1",
                   "every later leaf selected = path_len = -1", "no simulation is consumed", "The last two conditions OR bit 1 into *errors_dev",
                   "v = considered[m * n + t]", "or all k if there is none", "ties to the lowest c", "pending(0) += 1, paths[0, r, :] = node_action(fc + c*)",
                   "at most T levels in all", "out of budget, t >= n", "the counters are untouched", "add no pending visit",
                   "takes its pending visits back, the root's included", "consumes no simulation", "The repeat's own path rows hold what it passed",
                   "sim_visits[p, c*] += 1, sim_index[p] = t + 1", "With num_leaves == 1 and pending all zero every tensor pcbenv_gumbel_advance writes gets the same bits",
                   "PCBENV_EINVAL (checked before any device call, in this order)", "CHOOSE together with SELECT", "num_leaves outside [1, PCBENV_MAX_PUCT_LEAVES]",
                   "num_roots * num_leaves above 2^31 - 1", "reserved or reserved2 != 0", "num_nodes ... reward_hi and pending (every phase)",
                   "num_roots == 0 is a no-op success"):
        assert phrase in block, phrase
    assert "only enqueues" in raw.split("#ifndef PCBENV_GUMBEL_LEAVES_H")[0]


def test_exported_and_bound():
    L = _gumbel_leaves_lib.bind(_lib.load())
    assert _gumbel_leaves_lib.EXPORTS == ("pcbenv_gumbel_advance_leaves",) and hasattr(L, "pcbenv_gumbel_advance_leaves")
    assert len(L.pcbenv_gumbel_advance_leaves.argtypes) == 2 and L.pcbenv_gumbel_advance_leaves.restype is C.c_int
    assert all("pcbenv_gumbel_advance_leaves" not in m.EXPORTS for m in (_lib, _search_lib, _move_lib, _noise_lib, _leaves_lib, _gumbel_lib))
    R = _gumbel_leaves_lib.PcbenvGumbelLeavesRequest
    assert tuple(n for n, _ in R._fields_) == MEMBERS
    kinds = dict(struct_size=C.c_uint32, seed=C.c_uint64, step_index=C.c_uint64, **{n: C.c_double for n in DOUBLES}, **{n: C.c_void_p for n in POINTERS})
    for n, t in R._fields_:
        assert t is kinds.get(n, C.c_int32), n
    # csrc/pcb_gumbel_leaves.hip static_asserts the same figures of the struct as the library compiled it
    assert C.sizeof(R) == 360 and R.stream.offset == 352 and R.c_puct.offset == 48 and R.seed.offset == 72 and R.num_leaves.offset == 88
    assert R.num_nodes.offset == 96 and R.pending.offset == 200 and R.sim_index.offset == 272 and R.move_slot.offset == 296
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3  # the ABI version is unchanged


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_ctypes_structure_has_the_c_layout():
    """A compiled probe: sizeof and every member's offset as a C compiler lays include/pcbenv_gumbel_leaves.h out."""
    offsets, size = model_harness.layout("pcbenv_gumbel_leaves.h", "pcbenv_gumbel_leaves_request", MEMBERS)
    R = _gumbel_leaves_lib.PcbenvGumbelLeavesRequest
    assert size == C.sizeof(R)
    assert offsets == {n: getattr(R, n).offset for n in MEMBERS}


_HOST = (C.c_uint64 * 8)()  # host memory: never dereferenced, every call below fails before a device is touched
ALL = BEGIN | ABSORB | SELECT


def _call(request=True, size=None, phases=ALL, P=8, N=5, Cc=3, T=4, K=2, n=8, Mc=4, Lv=3, reserved=0, reserved2=0, c_visit=50.0, c_scale=1.0, null=(), odd=()):
    L = _gumbel_leaves_lib.bind(_lib.load())
    R = _gumbel_leaves_lib.PcbenvGumbelLeavesRequest
    req = R(struct_size=C.sizeof(R) if size is None else size, phases=phases, num_roots=P, capacity=N, max_children=Cc, max_steps=T, num_candidates=K,
            num_simulations=n, max_considered=Mc, reserved=reserved, c_puct=1.0, c_visit=c_visit, c_scale=c_scale, num_leaves=Lv, reserved2=reserved2)
    for name in TREE + EXCHANGE + INPUTS + BUDGET + OUTPUTS:  # errors_dev and stream stay null: both are optional
        if name not in null:
            setattr(req, name, C.addressof(_HOST) + (4 if name in odd else 2 if name + "/2" in odd else 0))
    rc = L.pcbenv_gumbel_advance_leaves(None, C.byref(req) if request else None)
    return rc, L.pcbenv_last_error(None).decode()


NAN, INF = math.nan, math.inf


@pytest.mark.parametrize("kw, msg", [
    ({"request": False}, "null request"),                                                   # 1
    ({"size": 0}, "struct_size"),                                                           # 2
    ({"size": 344, "phases": 0}, "struct_size"),                                            # pcbenv_gumbel_request's size is not this struct's
    ({"phases": 0}, "phases must be a non-empty set of BEGIN, ABSORB, SELECT, CHOOSE"),     # 3
    ({"phases": 16, "P": -1}, "phases must be"),
    ({"phases": -1}, "phases must be"),
    ({"phases": SELECT | CHOOSE, "P": -1}, "CHOOSE cannot be combined with SELECT"),
    ({"phases": 15}, "CHOOSE cannot be combined with SELECT"),
    ({"P": -1, "N": 0}, "num_roots must not be negative"),                                  # 4
    ({"N": 0, "Cc": 0}, "capacity"),                                                        # 5
    ({"Cc": 0, "T": 0}, "max_children"),                                                    # 6
    ({"Cc": 65}, "max_children"),
    ({"T": 0, "Lv": 0}, "max_steps"),                                                       # 7
    ({"Lv": 0, "K": 0}, "num_leaves must be in [1, 64]"),                                   # 8
    ({"Lv": 65, "P": 2 ** 31 - 1}, "num_leaves must be in [1, 64]"),
    ({"Lv": -1, "phases": CHOOSE}, "num_leaves must be in [1, 64]"),                        # in every phase
    ({"P": 2 ** 30, "Lv": 2, "K": 0}, "num_roots * num_leaves must not exceed 2^31 - 1"),   # 9
    ({"P": 2 ** 31 - 1, "Lv": 64, "phases": BEGIN}, "num_roots * num_leaves"),
    ({"K": 0, "n": 0}, "num_candidates must be at least 1 with ABSORB"),                    # 10
    ({"phases": BEGIN | SELECT, "K": 0, "n": 0}, "num_simulations"),                        # only with ABSORB
    ({"n": 0, "Mc": 0}, "num_simulations must be at least 1"),                              # 11
    ({"Mc": 0, "reserved": 1}, "max_considered must be in [1, 64]"),                        # 12
    ({"Mc": 65}, "max_considered"),
    ({"reserved": 1, "c_visit": NAN}, "reserved and reserved2 must be 0"),                  # 13
    ({"reserved2": -1, "c_scale": NAN}, "reserved and reserved2 must be 0"),
    ({"c_visit": NAN}, "c_visit and c_scale must be finite and not negative"),              # 14
    ({"c_visit": -1e-9}, "c_visit and c_scale"),
    ({"c_scale": INF, "null": ("prior",)}, "c_visit and c_scale"),
    *[({"null": (name,), "phases": ph}, "null tree tensor") for name in TREE for ph in (BEGIN, CHOOSE)],   # 15: pending among them, in every phase
    ({"null": ("pending", "sim_index")}, "null tree tensor"),
    *[({"null": (name,), "phases": ph}, "null sim_index or sim_visits") for name in ("sim_index", "sim_visits") for ph in (BEGIN, SELECT, CHOOSE)],  # 16
    ({"null": ("sim_index", "selected")}, "null sim_index or sim_visits"),
    ({"null": ("selected",), "phases": ABSORB}, "null selected"),                           # 17
    ({"null": ("selected", "paths"), "phases": SELECT}, "null selected"),
    *[({"null": (name,), "phases": SELECT}, "null path_len, paths or considered with SELECT") for name in ("path_len", "paths", "considered")],  # 18
    ({"null": ("considered", "value")}, "null path_len, paths or considered"),
    *[({"null": (name,), "phases": ABSORB}, "null value, leaf_terminal, cand_count, cand_actions or cand_prior with ABSORB") for name in INPUTS],  # 19
    *[({"null": (name,), "phases": CHOOSE}, "null move_slot, move_action, child_weights, child_policy, child_actions or root_value with CHOOSE")
      for name in OUTPUTS],                                                                 # 20
    ({"null": ("root_value",), "phases": CHOOSE, "odd": ("prior",)}, "null move_slot"),
    *[({"odd": (name,), "phases": BEGIN}, "8-byte aligned") for name in ("prior", "value_sum", "value_max", "reward_lo", "reward_hi")],  # 21
    ({"odd": ("value", "cand_prior/2")}, "8-byte aligned"),
    ({"odd": ("root_value", "child_policy/2"), "phases": CHOOSE}, "8-byte aligned"),
    ({"odd": ("cand_prior/2",)}, "cand_prior must be 4-byte aligned"),                       # 22
    ({"odd": ("child_policy/2",), "phases": CHOOSE | ABSORB}, "child_policy must be 4-byte aligned"),
    ({}, "null handle"),                                                                    # 23
    ({"phases": CHOOSE | BEGIN | ABSORB}, "null handle"),
    ({"c_visit": 0.0, "c_scale": 0.0, "Mc": 64, "Cc": 64, "n": 1, "Lv": 64}, "null handle"),  # the ends of the ranges are in
    ({"Lv": 1}, "null handle"),
    ({"P": (2 ** 31 - 1) // 64, "Lv": 64}, "null handle"),
    ({"phases": BEGIN, "null": EXCHANGE + INPUTS + OUTPUTS + ("considered",), "K": 0}, "null handle"),  # what a phase does not use may be null
    ({"phases": ABSORB, "null": ("path_len", "paths") + BUDGET + OUTPUTS}, "null handle"),
    ({"phases": SELECT, "null": INPUTS + OUTPUTS, "K": 0}, "null handle"),
    ({"phases": CHOOSE, "null": EXCHANGE + INPUTS + ("considered",), "K": 0}, "null handle"),
    ({"odd": ("value",), "phases": SELECT}, "null handle"),                                 # value is not read without ABSORB
    ({"odd": ("num_nodes", "parent", "pending", "sim_index", "sim_visits", "considered", "selected", "cand_prior", "child_policy")}, "null handle"),  # 4 bytes suffice
    ({"P": 0}, "null handle"),                                                              # the null handle is refused before the no-op
])
def test_argument_checks_need_no_device(kw, msg):
    rc, err = _call(**kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
