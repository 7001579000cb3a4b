"""ctypes binding of include/pcbenv_leaves.h: pcbenv_puct_advance_leaves, which libpcbenv.so exports beyond
include/pcbenv.h, include/pcbenv_search.h, include/pcbenv_priors.h and include/pcbenv_move.h.  `bind(L)` sets the
prototype on the library `_lib.load()` returns; nothing is added to `_lib`'s namespace."""
from __future__ import annotations

import ctypes as C

from ._lib import bind_exports
from ._search_lib import PUCT_EXCHANGE, PUCT_INPUTS, PUCT_TREE_TENSORS

EXPORTS = ("pcbenv_puct_advance_leaves",)
MAX_PUCT_LEAVES = 64

LEAVES_TREE_TENSORS = PUCT_TREE_TENSORS + ("pending",)


class PcbenvPuctLeavesRequest(C.Structure):
    """pcbenv_puct_leaves_request (include/pcbenv_leaves.h), the arguments of pcbenv_puct_advance_leaves."""
    _fields_ = ([("struct_size", C.c_uint32), ("phases", C.c_int32), ("num_roots", C.c_int32), ("capacity", C.c_int32),
                 ("max_children", C.c_int32), ("max_steps", C.c_int32), ("num_candidates", C.c_int32), ("reserved", C.c_int32),
                 ("c_puct", C.c_double), ("num_leaves", C.c_int32), ("reserved2", C.c_int32)]
                + [(n, C.c_void_p) for n in LEAVES_TREE_TENSORS + PUCT_EXCHANGE + PUCT_INPUTS + ("errors_dev", "stream")])


def bind(L):
    """Prototypes of EXPORTS on the loaded library; ImportError if it lacks one (there is no fallback).  Returns L."""
    return bind_exports(L, {name: PcbenvPuctLeavesRequest for name in EXPORTS})
