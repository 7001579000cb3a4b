"""ctypes binding of include/pcbenv_move.h: pcbenv_puct_move, which libpcbenv.so exports beyond include/pcbenv.h,
include/pcbenv_search.h and include/pcbenv_priors.h.  `bind(L)` sets the prototype on the library `_lib.load()` returns;
nothing is added to `_lib`'s namespace."""
from __future__ import annotations

import ctypes as C

from ._lib import bind_exports

EXPORTS = ("pcbenv_puct_move",)

MOVE_CHOOSE, MOVE_REROOT = 1, 2          # phases
MOVE_GREEDY, MOVE_PROPORTIONAL = 0, 1    # mode

MOVE_TREE_TENSORS = ("num_nodes", "parent", "depth", "visits", "num_children", "first_child", "node_action", "prior", "value_sum", "value_max",
                     "terminal", "reward_lo", "reward_hi")
MOVE_OUTPUTS = ("move_slot", "move_action", "child_visits", "child_actions", "root_value", "remap")


class PcbenvPuctMoveRequest(C.Structure):
    """pcbenv_puct_move_request (include/pcbenv_move.h), the arguments of pcbenv_puct_move."""
    _fields_ = ([("struct_size", C.c_uint32), ("phases", C.c_int32), ("num_roots", C.c_int32), ("capacity", C.c_int32),
                 ("max_children", C.c_int32), ("mode", C.c_int32), ("first_root", C.c_int32), ("reserved", C.c_int32),
                 ("seed", C.c_uint64), ("step_index", C.c_uint64)]
                + [(n, C.c_void_p) for n in MOVE_TREE_TENSORS + MOVE_OUTPUTS + ("reset", "errors_dev", "stream")])


def bind(L):
    """Prototypes of EXPORTS on the loaded library; ImportError if it lacks one (there is no fallback).  Returns L."""
    return bind_exports(L, {name: PcbenvPuctMoveRequest for name in EXPORTS})
