"""ctypes binding of include/pcbenv_search.h: what libpcbenv.so exports beyond include/pcbenv.h.  `bind(L)` sets the
prototypes on the library `_lib.load()` returns; nothing is added to `_lib`'s namespace."""
from __future__ import annotations

import ctypes as C

from ._lib import bind_exports

EXPORTS = ("pcbenv_puct_advance",)

PUCT_TREE_TENSORS = ("num_nodes", "parent", "depth", "visits", "num_children", "first_child", "node_action", "prior", "value_sum", "value_max",
                     "terminal", "reward_lo", "reward_hi")
PUCT_EXCHANGE = ("selected", "path_len", "paths")
PUCT_INPUTS = ("value", "leaf_terminal", "cand_count", "cand_actions", "cand_prior")


class PcbenvPuctRequest(C.Structure):
    """pcbenv_puct_request (include/pcbenv_search.h), the arguments of pcbenv_puct_advance."""
    _fields_ = ([("struct_size", C.c_uint32), ("phases", C.c_int32), ("num_roots", C.c_int32), ("capacity", C.c_int32),
                 ("max_children", C.c_int32), ("max_steps", C.c_int32), ("num_candidates", C.c_int32), ("reserved", C.c_int32),
                 ("c_puct", C.c_double)]
                + [(n, C.c_void_p) for n in PUCT_TREE_TENSORS + PUCT_EXCHANGE + PUCT_INPUTS + ("errors_dev", "stream")])


def bind(L):
    """Prototypes of EXPORTS on the loaded library; ImportError if it lacks one (there is no fallback).  Returns L."""
    return bind_exports(L, {name: PcbenvPuctRequest for name in EXPORTS})
