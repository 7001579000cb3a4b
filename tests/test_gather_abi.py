"""pcbenv_gather on the CPU side: the header declares it, libpcbenv.so exports it, pcbenv/_lib.py binds it, and the
argument checks that need no device refuse what they must.  Also the index arithmetic of search.best_of_k on CPU
tensors.  No compute call is made."""
import ctypes as C
import re

import torch

import abi_header
from pcbenv import _lib
from pcbenv.search import child_index, pick_best


def test_gather_is_declared_exported_and_bound():
    text = abi_header.text()
    assert re.search(r"\bint\s+pcbenv_gather\s*\(\s*pcbenv\s*\*\s*dst\s*,\s*const\s+pcbenv\s*\*\s*src\s*,\s*const\s+int32_t\s*\*"
                     r"\s*src_index_dev\s*,\s*uint32_t\s*\*\s*errors_dev\s*,\s*void\s*\*\s*stream\s*\)", text)
    assert "pcbenv_gather" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(L, "pcbenv_gather")
    assert L.pcbenv_abi_version() == _lib.ABI_VERSION == 3  # an addition: the ABI version stays


def test_gather_null_arguments_are_errors_not_crashes():
    L = _lib.load()
    idx = (C.c_int32 * 4)()
    assert L.pcbenv_gather(None, None, C.cast(idx, C.c_void_p), None, None) == _lib.PCBENV_EINVAL


def test_best_of_k_child_index():
    idx = child_index(3, 4)
    assert idx.dtype == torch.int32 and idx.device.type == "cpu"
    assert idx.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]
    assert child_index(1, 1).tolist() == [0]
    # planner environment i plays root i // k
    P, k = 5, 7
    assert torch.equal(child_index(P, k).long(), torch.arange(P * k) // k)


def test_best_of_k_pick_best():
    r = torch.tensor([-3.0, -1.0, -2.0,  -5.0, -5.0, -4.0,  -0.5, -0.25, -0.25], dtype=torch.float64)
    reward, child = pick_best(r, 3)
    assert reward.tolist() == [-1.0, -4.0, -0.25]
    assert child.tolist() == [1, 5, 7]  # ties: the first such child
    assert torch.equal(reward, r[child])
