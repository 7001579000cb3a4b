"""ctypes binding of include/pcbenv_frontier_sample.h: pcbenv_frontier_sample, the frontier step of a stochastic beam
search over placements, which libpcbenv.so exports beyond include/pcbenv.h and the other search headers.  `bind(L)` sets
the prototype on the library `_lib.load()` returns; nothing is added to `_lib`'s namespace."""
from __future__ import annotations

import ctypes as C

from ._frontier_lib import FRONTIER_ADVANCE, FRONTIER_INIT, FRONTIER_OWN, MAX_FRONTIER_CANDIDATES, MAX_FRONTIER_ROWS, MAX_FRONTIER_WIDTH, ERR_ROW  # noqa: F401
from ._lib import bind_exports
from ._search_lib import PUCT_INPUTS

EXPORTS = ("pcbenv_frontier_sample",)
ERR_SET = 4  # bit 2 of the error word: a set_len outside [-1, T]

SAMPLE_SET = ("paths", "path_len", "cum_logp", "gumbel")  # the tensors of a set of rows: <name>_in and <name>_out in the request
SAMPLE_OWN = ("set_len", "set_gumbel", "set_logp", "set_value", "set_path")  # the sample set, beside FRONTIER_OWN


class PcbenvFrontierSampleRequest(C.Structure):
    """pcbenv_frontier_sample_request (include/pcbenv_frontier_sample.h), the arguments of pcbenv_frontier_sample."""
    _fields_ = ([("struct_size", C.c_uint32), ("phases", C.c_int32), ("num_roots", C.c_int32), ("width", C.c_int32),
                 ("num_candidates", C.c_int32), ("max_steps", C.c_int32), ("seed", C.c_uint64), ("step_index", C.c_uint64),
                 ("first_root", C.c_int32), ("reserved", C.c_int32)]
                + [(n, C.c_void_p) for n in tuple(n + "_in" for n in SAMPLE_SET) + tuple(n + "_out" for n in SAMPLE_SET) + FRONTIER_OWN + SAMPLE_OWN
                   + PUCT_INPUTS + ("errors_dev", "stream")])


def bind(L):
    """Prototypes of EXPORTS on the loaded library; ImportError if it lacks one (there is no fallback).  Returns L."""
    return bind_exports(L, {name: PcbenvFrontierSampleRequest for name in EXPORTS})
