"""pcbenv_gumbel_tree_advance on the CPU side: include/pcbenv_gumbel_tree.h declares it over pcbenv_gumbel.h's request, which
stays as it is, libpcbenv.so exports it, pcbenv/_gumbel_tree_lib.py binds it with `_gumbel_lib`'s structure, and every
argument check refuses what it must before anything touches a device, in pcbenv_gumbel_advance's order and words, the null
handle last.  No compute call is made."""
import ctypes as C
import math
import os
import re

import pytest

from abi_header import REPO
from pcbenv import _gumbel_leaves_lib, _gumbel_lib, _gumbel_tree_lib, _lib, _move_lib, _noise_lib, _search_lib

PATH = os.path.join(REPO, "include", "pcbenv_gumbel_tree.h")
TREE, EXCHANGE, INPUTS = _search_lib.PUCT_TREE_TENSORS, _search_lib.PUCT_EXCHANGE, _search_lib.PUCT_INPUTS
BUDGET, OUTPUTS = _gumbel_lib.GUMBEL_BUDGET, _gumbel_lib.GUMBEL_OUTPUTS
BEGIN, ABSORB, SELECT, CHOOSE = 1, 2, 4, 8


def _raw():
    with open(PATH) as f:
        return f.read()


def test_header_declares_the_function_over_the_request_of_the_root_rule():
    raw = _raw()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r'#include\s+"pcbenv_gumbel.h"', text) and "PCBENV_ABI_VERSION" not in text and "typedef" not in text and "#define PCBENV_GUMBEL_BEGIN" not in text
    assert re.search(r"\bint\s+pcbenv_gumbel_tree_advance\s*\(\s*const\s+pcbenv\s*\*\s*env\s*,\s*const\s+pcbenv_gumbel_request\s*\*\s*req\s*\)\s*;", text)
    assert len(re.findall(r"\b\w+\s*\([^()]*\)\s*;", text)) == 1  # one prototype
    block = re.sub(r"\s*\n \*\s*", " ", raw[:raw.index("int pcbenv_gumbel_tree_advance")].rsplit("/*", 1)[1])
    for phrase in ("one kernel launch on req->stream", "nothing the library owns is read or written", "no bound buffers",
                   "Enqueue only, no allocation, no synchronisation", "hipGraph", "c_puct is never read", "before it addresses anything",
                   "pr_c    = prior(ch) > 2^-149 ? (prior(ch) < 1 ? prior(ch) : 1) : 2^-149", "Nsum    = sum_c n_c", "S       = sum_c value_sum(ch)",
                   "Wv      = sum_{c: n_c > 0} pr_c ;  Qv = sum_{c: n_c > 0} pr_c * q_c", "own     = visits(a) - Nsum",
                   "vhat    = own > 0 ? (value_sum(a) - S) / (double)own : (visits(a) > 0 ? value_sum(a) / visits(a) : lo)",
                   "vmix    = (Nsum > 0 && Wv > 0.0) ? (vhat + ((double)Nsum / Wv) * Qv) / (1.0 + (double)Nsum) : vhat",
                   "qhat_c  = hi > lo ? ((n_c > 0 ? q_c : vmix) - lo) / (hi - lo) : 0.0", "sigma_c = ((c_visit + (double)max_b n_b) * c_scale) * qhat_c",
                   "t_c     = pi_c - (double)n_c / (1.0 + (double)Nsum)", "in child order from 0.0", "data, not an error", "PCBENV_MOVE_REROOT",
                   "Two deliberate departures from the paper", "not per node", "derived as above rather than stored", "word for word",
                   "ties to the lowest c", "SELECT never stores to the tree", "With c_scale == 0", "all have n_c > 0", "num_roots == 0 is a no-op success"):
        assert phrase in block, phrase
    assert "only enqueues" in raw.split("#ifndef PCBENV_GUMBEL_TREE_H")[0]


def test_exported_and_bound():
    L = _gumbel_tree_lib.bind(_lib.load())
    assert _gumbel_tree_lib.EXPORTS == ("pcbenv_gumbel_tree_advance",) and hasattr(L, "pcbenv_gumbel_tree_advance")
    fn = L.pcbenv_gumbel_tree_advance
    assert len(fn.argtypes) == 2 and fn.restype is C.c_int and fn.argtypes[1]._type_ is _gumbel_lib.PcbenvGumbelRequest
    assert all("pcbenv_gumbel_tree_advance" not in m.EXPORTS for m in (_lib, _search_lib, _move_lib, _noise_lib, _gumbel_lib, _gumbel_leaves_lib))
    assert C.sizeof(_gumbel_lib.PcbenvGumbelRequest) == 344  # csrc/pcb_gumbel_tree.hip static_asserts the same
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3


_HOST = (C.c_uint64 * 8)()  # host memory: never dereferenced, every call below fails before a device is touched
ALL = BEGIN | ABSORB | SELECT


def _call(request=True, size=None, phases=ALL, P=8, N=5, Cc=3, T=4, K=2, n=8, Mc=4, reserved=0, c_puct=1.0, c_visit=50.0, c_scale=1.0, null=(), odd=()):
    L = _gumbel_tree_lib.bind(_lib.load())
    R = _gumbel_lib.PcbenvGumbelRequest
    req = R(struct_size=C.sizeof(R) if size is None else size, phases=phases, num_roots=P, capacity=N, max_children=Cc, max_steps=T, num_candidates=K,
            num_simulations=n, max_considered=Mc, reserved=reserved, c_puct=c_puct, c_visit=c_visit, c_scale=c_scale)
    for name in TREE + EXCHANGE + INPUTS + BUDGET + OUTPUTS:  # errors_dev and stream stay null: both are optional
        if name not in null:
            setattr(req, name, C.addressof(_HOST) + (4 if name in odd else 2 if name + "/2" in odd else 0))
    rc = L.pcbenv_gumbel_tree_advance(None, C.byref(req) if request else None)
    return rc, L.pcbenv_last_error(None).decode()


NAN, INF = math.nan, math.inf


# every check of include/pcbenv_gumbel.h's list, in its order: each case also breaks the check behind it, which must not be the one reported
@pytest.mark.parametrize("kw, msg", [
    ({"request": False}, "null request"),                                                   # 1
    ({"size": 0, "phases": 0}, "struct_size"),                                              # 2
    ({"phases": 0, "P": -1}, "phases must be a non-empty set of BEGIN, ABSORB, SELECT, CHOOSE"),  # 3
    ({"phases": 16, "P": -1}, "phases must be"),
    ({"phases": SELECT | CHOOSE, "P": -1}, "CHOOSE cannot be combined with SELECT"),
    ({"P": -1, "N": 0}, "num_roots must not be negative"),                                  # 4
    ({"N": 0, "Cc": 0}, "capacity"),                                                        # 5
    ({"Cc": 0, "T": 0}, "max_children"),                                                    # 6
    ({"Cc": 65, "T": 0}, "max_children"),
    ({"T": 0, "K": 0}, "max_steps"),                                                        # 7
    ({"K": 0, "n": 0}, "num_candidates must be at least 1 with ABSORB"),                    # 8
    ({"phases": BEGIN | SELECT, "K": 0, "n": 0}, "num_simulations"),                        # only with ABSORB
    ({"n": 0, "Mc": 0}, "num_simulations must be at least 1"),                              # 9
    ({"Mc": 0, "reserved": 1}, "max_considered must be in [1, 64]"),                        # 10
    ({"Mc": 65, "reserved": 1}, "max_considered"),
    ({"reserved": 1, "c_visit": NAN}, "reserved"),                                          # 11
    ({"c_visit": NAN, "null": ("prior",)}, "c_visit and c_scale must be finite and not negative"),  # 12
    ({"c_visit": -1e-9}, "c_visit and c_scale"),
    ({"c_scale": INF, "null": ("prior",)}, "c_visit and c_scale"),
    *[({"null": (name, "sim_index"), "phases": ph}, "null tree tensor") for name in TREE for ph in (BEGIN, CHOOSE)],   # 13
    *[({"null": (name, "selected"), "phases": ph}, "null sim_index or sim_visits") for name in ("sim_index", "sim_visits") for ph in (BEGIN, SELECT, CHOOSE)],  # 14
    ({"null": ("selected", "paths"), "phases": SELECT}, "null selected"),                   # 15
    ({"null": ("selected", "value"), "phases": ABSORB}, "null selected"),
    *[({"null": (name, "value"), "phases": SELECT | ABSORB}, "null path_len, paths or considered with SELECT") for name in ("path_len", "paths", "considered")],  # 16
    *[({"null": (name, "move_slot"), "phases": ABSORB | CHOOSE}, "null value, leaf_terminal, cand_count, cand_actions or cand_prior with ABSORB")
      for name in INPUTS],                                                                  # 17
    *[({"null": (name,), "phases": CHOOSE, "odd": ("prior",)}, "null move_slot, move_action, child_weights, child_policy, child_actions or root_value with CHOOSE")
      for name in OUTPUTS],                                                                 # 18
    *[({"odd": (name, "cand_prior/2"), "phases": BEGIN | ABSORB}, "8-byte aligned") for name in ("prior", "value_sum", "value_max", "reward_lo", "reward_hi", "value")],  # 19
    ({"odd": ("root_value", "child_policy/2"), "phases": CHOOSE}, "8-byte aligned"),
    ({"odd": ("cand_prior/2", "child_policy/2"), "phases": ABSORB | CHOOSE}, "cand_prior must be 4-byte aligned"),  # 20
    ({"odd": ("child_policy/2",), "phases": CHOOSE | ABSORB}, "child_policy must be 4-byte aligned"),
    ({}, "null handle"),                                                                    # 21
    ({"c_puct": NAN}, "null handle"),                                                       # c_puct is never read, not even to be checked
    ({"c_puct": -INF, "phases": CHOOSE}, "null handle"),
    ({"c_visit": 0.0, "c_scale": 0.0, "Mc": 64, "Cc": 64, "n": 1}, "null handle"),          # the ends of the ranges are in
    ({"phases": BEGIN, "null": EXCHANGE + INPUTS + OUTPUTS + ("considered",), "K": 0}, "null handle"),  # what a phase does not use may be null
    ({"phases": ABSORB, "null": ("path_len", "paths") + BUDGET + OUTPUTS}, "null handle"),
    ({"phases": SELECT, "null": INPUTS + OUTPUTS, "K": 0}, "null handle"),
    ({"phases": CHOOSE, "null": EXCHANGE + INPUTS + ("considered",), "K": 0}, "null handle"),
    ({"odd": ("value",), "phases": SELECT}, "null handle"),                                 # value is not read without ABSORB
    ({"P": 0}, "null handle"),                                                              # the null handle is refused before the no-op
])
def test_argument_checks_need_no_device(kw, msg):
    rc, err = _call(**kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
