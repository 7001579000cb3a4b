"""ctypes binding of include/pcbenv_frontier.h: pcbenv_frontier_advance, the frontier step of a beam search over
placements, which libpcbenv.so exports beyond include/pcbenv.h and the other search headers.  `bind(L)` sets the prototype
on the library `_lib.load()` returns; nothing is added to `_lib`'s namespace."""
from __future__ import annotations

import ctypes as C

from ._lib import bind_exports
from ._search_lib import PUCT_INPUTS

EXPORTS = ("pcbenv_frontier_advance",)
FRONTIER_INIT, FRONTIER_ADVANCE = 1, 2
MAX_FRONTIER_WIDTH, MAX_FRONTIER_CANDIDATES, MAX_FRONTIER_ROWS = 64, 64, 1024
ERR_ROW = 2  # bit 1 of the error word: a path_len_in outside [-1, T]

FRONTIER_SET = ("paths", "path_len", "cum_logp")  # the tensors of a set of rows: <name>_in and <name>_out in the request
FRONTIER_OWN = ("parent_row", "live", "best_value", "best_len", "best_path")


class PcbenvFrontierRequest(C.Structure):
    """pcbenv_frontier_request (include/pcbenv_frontier.h), the arguments of pcbenv_frontier_advance."""
    _fields_ = ([("struct_size", C.c_uint32), ("phases", C.c_int32), ("num_roots", C.c_int32), ("width", C.c_int32),
                 ("num_candidates", C.c_int32), ("max_steps", C.c_int32), ("prior_weight", C.c_double), ("reserved", C.c_int32),
                 ("reserved2", C.c_int32)]
                + [(n, C.c_void_p) for n in tuple(n + "_in" for n in FRONTIER_SET) + tuple(n + "_out" for n in FRONTIER_SET) + FRONTIER_OWN
                   + PUCT_INPUTS + ("errors_dev", "stream")])


def bind(L):
    """Prototypes of EXPORTS on the loaded library; ImportError if it lacks one (there is no fallback).  Returns L."""
    return bind_exports(L, {name: PcbenvFrontierRequest for name in EXPORTS})
