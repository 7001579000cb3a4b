"""ctypes binding of include/pcbenv_gumbel.h: pcbenv_gumbel_advance, which libpcbenv.so exports beyond include/pcbenv.h,
include/pcbenv_search.h, include/pcbenv_priors.h, include/pcbenv_move.h and include/pcbenv_noise.h.  `bind(L)` sets the
prototype on the library `_lib.load()` returns; nothing is added to `_lib`'s namespace."""
from __future__ import annotations

import ctypes as C

from ._lib import bind_exports
from ._search_lib import PUCT_EXCHANGE, PUCT_INPUTS, PUCT_TREE_TENSORS

EXPORTS = ("pcbenv_gumbel_advance",)

GUMBEL_BEGIN, GUMBEL_ABSORB, GUMBEL_SELECT, GUMBEL_CHOOSE = 1, 2, 4, 8  # phases
MAX_CONSIDERED = 64

GUMBEL_BUDGET = ("sim_index", "sim_visits", "considered")
GUMBEL_OUTPUTS = ("move_slot", "move_action", "child_weights", "child_policy", "child_actions", "root_value")


class PcbenvGumbelRequest(C.Structure):
    """pcbenv_gumbel_request (include/pcbenv_gumbel.h), the arguments of pcbenv_gumbel_advance."""
    _fields_ = ([("struct_size", C.c_uint32), ("phases", C.c_int32), ("num_roots", C.c_int32), ("capacity", C.c_int32),
                 ("max_children", C.c_int32), ("max_steps", C.c_int32), ("num_candidates", C.c_int32), ("num_simulations", C.c_int32),
                 ("max_considered", C.c_int32), ("first_root", C.c_int32), ("reserved", C.c_int32),
                 ("c_puct", C.c_double), ("c_visit", C.c_double), ("c_scale", C.c_double), ("seed", C.c_uint64), ("step_index", C.c_uint64)]
                + [(n, C.c_void_p) for n in PUCT_TREE_TENSORS + PUCT_EXCHANGE + PUCT_INPUTS + GUMBEL_BUDGET + GUMBEL_OUTPUTS + ("errors_dev", "stream")])


assert C.sizeof(PcbenvGumbelRequest) == 344 and PcbenvGumbelRequest.stream.offset == 336 and PcbenvGumbelRequest.c_puct.offset == 48 and \
    PcbenvGumbelRequest.seed.offset == 72 and PcbenvGumbelRequest.num_nodes.offset == 88 and PcbenvGumbelRequest.sim_index.offset == 256 and \
    PcbenvGumbelRequest.move_slot.offset == 280  # csrc/pcb_gumbel.hip's static_assert


def bind(L):
    """Prototypes of EXPORTS on the loaded library; ImportError if it lacks one (there is no fallback).  Returns L."""
    return bind_exports(L, {name: PcbenvGumbelRequest for name in EXPORTS})
