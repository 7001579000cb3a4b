"""ctypes binding of include/pcbenv_gumbel_leaves.h: pcbenv_gumbel_advance_leaves, which libpcbenv.so exports beyond
include/pcbenv.h, include/pcbenv_search.h, include/pcbenv_priors.h, include/pcbenv_move.h, include/pcbenv_leaves.h,
include/pcbenv_noise.h and include/pcbenv_gumbel.h.  `bind(L)` sets the prototype on the library `_lib.load()` returns;
nothing is added to `_lib`'s namespace.  The phases are `_gumbel_lib`'s, the bound on the leaves `_leaves_lib`'s."""
from __future__ import annotations

import ctypes as C

from ._gumbel_lib import GUMBEL_BUDGET, GUMBEL_OUTPUTS
from ._leaves_lib import LEAVES_TREE_TENSORS
from ._lib import bind_exports
from ._search_lib import PUCT_EXCHANGE, PUCT_INPUTS

EXPORTS = ("pcbenv_gumbel_advance_leaves",)


class PcbenvGumbelLeavesRequest(C.Structure):
    """pcbenv_gumbel_leaves_request (include/pcbenv_gumbel_leaves.h), the arguments of pcbenv_gumbel_advance_leaves."""
    _fields_ = ([("struct_size", C.c_uint32), ("phases", C.c_int32), ("num_roots", C.c_int32), ("capacity", C.c_int32),
                 ("max_children", C.c_int32), ("max_steps", C.c_int32), ("num_candidates", C.c_int32), ("num_simulations", C.c_int32),
                 ("max_considered", C.c_int32), ("first_root", C.c_int32), ("reserved", C.c_int32),
                 ("c_puct", C.c_double), ("c_visit", C.c_double), ("c_scale", C.c_double), ("seed", C.c_uint64), ("step_index", C.c_uint64),
                 ("num_leaves", C.c_int32), ("reserved2", C.c_int32)]
                + [(n, C.c_void_p) for n in LEAVES_TREE_TENSORS + PUCT_EXCHANGE + PUCT_INPUTS + GUMBEL_BUDGET + GUMBEL_OUTPUTS + ("errors_dev", "stream")])


assert C.sizeof(PcbenvGumbelLeavesRequest) == 360 and PcbenvGumbelLeavesRequest.stream.offset == 352 and PcbenvGumbelLeavesRequest.c_puct.offset == 48 and \
    PcbenvGumbelLeavesRequest.seed.offset == 72 and PcbenvGumbelLeavesRequest.num_leaves.offset == 88 and PcbenvGumbelLeavesRequest.num_nodes.offset == 96 and \
    PcbenvGumbelLeavesRequest.pending.offset == 200 and PcbenvGumbelLeavesRequest.sim_index.offset == 272 and \
    PcbenvGumbelLeavesRequest.move_slot.offset == 296  # csrc/pcb_gumbel_leaves.hip's static_assert


def bind(L):
    """Prototypes of EXPORTS on the loaded library; ImportError if it lacks one (there is no fallback).  Returns L."""
    return bind_exports(L, {name: PcbenvGumbelLeavesRequest for name in EXPORTS})
