"""pcbenv_gumbel_tree_advance_leaves on the CPU side: include/pcbenv_gumbel_tree_leaves.h declares it and its contract and
adds no struct -- the request is pcbenv_gumbel_leaves_request as it is -- libpcbenv.so exports it, pcbenv/_gumbel_tree_leaves_lib.py
binds it with pcbenv/_gumbel_leaves_lib.py's structure, the earlier headers and bindings stay as they are, and every argument check
of pcbenv_gumbel_advance_leaves refuses here what it refuses there, in the same order, with the same message, before anything
touches a device.  No compute call is made."""
import ctypes as C
import os
import re
import shutil

import pytest

from abi_header import REPO
import model_harness
import test_gumbel_leaves_abi as tla
from pcbenv import _gumbel_leaves_lib, _gumbel_lib, _gumbel_tree_leaves_lib, _gumbel_tree_lib, _leaves_lib, _lib, _move_lib, _noise_lib, _search_lib

PATH = os.path.join(REPO, "include", "pcbenv_gumbel_tree_leaves.h")
NAME = "pcbenv_gumbel_tree_advance_leaves"
# the checks of pcbenv_gumbel_advance_leaves, every one, in the order its header gives: the very table of its test
CHECKS = tla.test_argument_checks_need_no_device.pytestmark[0].args[1]


def test_header_declares_the_function_and_the_contract_and_no_struct():
    with open(PATH) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r'#include\s+"pcbenv_gumbel_leaves.h"', text) and re.search(r'#include\s+"pcbenv_gumbel_tree.h"', text) and "PCBENV_ABI_VERSION" not in text
    assert "#define" not in text.replace("#define PCBENV_GUMBEL_TREE_LEAVES_H", "") and "struct" not in text and "typedef" not in text
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*const\s+pcbenv\s*\*\s*env\s*,\s*const\s+pcbenv_gumbel_leaves_request\s*\*\s*req\s*\)\s*;", text)
    assert len(re.findall(r"\b\w+\s*\([^()]*\)\s*;", text)) == 1  # one prototype
    block = re.sub(r" +", " ", re.sub(r"\s*\n \*\s*", " ", raw[:raw.index("int " + NAME)].rsplit("/*", 1)[1]))  # the formulas are aligned with blanks
    for phrase in ("one kernel launch on req->stream", "pcbenv_gumbel_leaves_request, the struct of pcbenv_gumbel_advance_leaves, as it is",
                   "Enqueue only, no allocation, no synchronisation", "hipGraph", "c_puct is never read", "never pending",
                   "max_b n_b inside sigma is the absorbed count too", "pi' of a node is the same for every leaf of a launch", "m_c = (int64) n_c + pn_c",
                   "Msum = sum_c m_c", "t_c = pi_c - (double) m_c / (1.0 + (double) Msum)", "ties to the lowest c", "no virtual loss enters q or vmix",
                   "|m_c - M pi_c| keeps the bound of the one-leaf rule", "With pending == 0, t_c has the bits of pcbenv_gumbel_tree.h's t_c",
                   "pending is data: it addresses nothing", "Msum == -1", "a NaN t_c counts as -inf, so the order is total",
                   "PCBENV_GUMBEL_BEGIN. pcbenv_gumbel_advance's, bit for bit", "pcbenv_puct_advance_leaves' PCBENV_TREE_ABSORB",
                   "PCBENV_GUMBEL_CHOOSE. pcbenv_gumbel_tree_advance's, bit for bit; it does not read pending", "with three replacements",
                   "They are computed once per launch and read no pending visit", "pending += 1 on every node left and on the node reached",
                   "at most T levels in all", "Out of budget, t >= n: leaf 0 is one descent from the root by the rule above", "leaves l >= 1 get selected = path_len = -1",
                   "takes its pending visits back, the root's included, consumes no simulation", "The repeat's own path rows hold what it passed",
                   "leaf 0 gets selected = 0, path_len = 0 and pending(0) += 1", "I1", "I2", "I3",
                   "With num_leaves == 1 and pending all zero every tensor pcbenv_gumbel_tree_advance writes gets the same bits", "On trees with non-negative visits",
                   "After the ABSORB of every SELECT, pending is zero", "PCBENV_EINVAL: pcbenv_gumbel_advance_leaves' checks, in its order, with its messages",
                   "num_roots == 0 is a no-op success"):
        assert phrase in block, phrase
    assert "only enqueues" in raw.split("#ifndef PCBENV_GUMBEL_TREE_LEAVES_H")[0] and "ABI version is pcbenv.h's and is unchanged" in re.sub(r"\s*\n \*\s*", " ", raw)


def test_exported_and_bound():
    L = _gumbel_tree_leaves_lib.bind(_lib.load())
    assert _gumbel_tree_leaves_lib.EXPORTS == (NAME,) and hasattr(L, NAME)
    assert len(getattr(L, NAME).argtypes) == 2 and getattr(L, NAME).restype is C.c_int
    assert getattr(L, NAME).argtypes[1]._type_ is _gumbel_leaves_lib.PcbenvGumbelLeavesRequest  # the request is the earlier entry point's, as it is
    assert all(NAME not in m.EXPORTS for m in (_lib, _search_lib, _move_lib, _noise_lib, _leaves_lib, _gumbel_lib, _gumbel_leaves_lib, _gumbel_tree_lib))
    assert C.sizeof(_gumbel_leaves_lib.PcbenvGumbelLeavesRequest) == 360  # csrc/pcb_gumbel_tree_leaves.hip static_asserts the same
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3  # the ABI version is unchanged


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_header_compiles_as_c_and_brings_the_struct():
    """A compiled probe: include/pcbenv_gumbel_tree_leaves.h alone gives a C compiler the request struct, laid out as the binding has it."""
    offsets, size = model_harness.layout("pcbenv_gumbel_tree_leaves.h", "pcbenv_gumbel_leaves_request", tla.MEMBERS)
    R = _gumbel_leaves_lib.PcbenvGumbelLeavesRequest
    assert size == C.sizeof(R) == 360 and offsets == {n: getattr(R, n).offset for n in tla.MEMBERS}


def _call(entry, request=True, size=None, phases=tla.ALL, P=8, N=5, Cc=3, T=4, K=2, n=8, Mc=4, Lv=3, reserved=0, reserved2=0, c_visit=50.0, c_scale=1.0, null=(), odd=()):
    L = _gumbel_tree_leaves_lib.bind(_lib.load())
    R = _gumbel_leaves_lib.PcbenvGumbelLeavesRequest
    req = R(struct_size=C.sizeof(R) if size is None else size, phases=phases, num_roots=P, capacity=N, max_children=Cc, max_steps=T, num_candidates=K,
            num_simulations=n, max_considered=Mc, reserved=reserved, c_puct=1.0, c_visit=c_visit, c_scale=c_scale, num_leaves=Lv, reserved2=reserved2)
    for name in tla.TREE + tla.EXCHANGE + tla.INPUTS + tla.BUDGET + tla.OUTPUTS:  # errors_dev and stream stay null: both are optional
        if name not in null:
            setattr(req, name, C.addressof(tla._HOST) + (4 if name in odd else 2 if name + "/2" in odd else 0))
    rc = getattr(L, entry)(None, C.byref(req) if request else None)
    return rc, L.pcbenv_last_error(None).decode()


def test_the_table_is_the_whole_of_it():
    messages = {msg for _, msg in CHECKS}
    assert len(CHECKS) >= 100 and {"null request", "struct_size", "null tree tensor", "null handle", "num_leaves must be in [1, 64]"} <= messages


@pytest.mark.parametrize("kw, msg", CHECKS)
def test_argument_checks_need_no_device(kw, msg):
    rc, err = _call(NAME, **kw)
    assert rc == _lib.PCBENV_EINVAL
    assert msg in err
    assert (rc, err) == _call("pcbenv_gumbel_advance_leaves", **kw)  # the earlier entry point's check, its message word for word
