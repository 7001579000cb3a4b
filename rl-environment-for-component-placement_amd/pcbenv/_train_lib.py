"""ctypes binding of include/pcbenv_train.h: pcbenv_evaluate_visits and pcbenv_evaluate_visits_backward, which
libpcbenv.so exports beyond include/pcbenv.h, include/pcbenv_search.h, include/pcbenv_priors.h and include/pcbenv_move.h.
`bind(L)` sets the prototypes on the library `_lib.load()` returns; nothing is added to `_lib`'s namespace."""
from __future__ import annotations

import ctypes as C

from ._lib import bind_exports

EXPORTS = ("pcbenv_evaluate_visits", "pcbenv_evaluate_visits_backward")

ROW_OK, ROW_ZERO, ROW_NO_TARGET = 0, 1, 2                 # stats[:, 3]
ERR_NONFINITE, ERR_ALL_NEG_INF, ERR_TARGET = 1, 2, 4      # the error bits

VISITS_INPUTS = ("logits", "mask_bits", "visits", "target_actions")
VISITS_FORWARD = ("cross_entropy", "entropy", "stats", "errors_dev")
VISITS_BACKWARD = ("grad_cross_entropy", "grad_entropy", "grad_logits")


class PcbenvVisitsRequest(C.Structure):
    """pcbenv_visits_request (include/pcbenv_train.h), the arguments of both calls."""
    _fields_ = ([("struct_size", C.c_uint32), ("logits_dtype", C.c_int32), ("action_format", C.c_int32), ("num_targets", C.c_int32),
                 ("num_rows", C.c_int64), ("reserved", C.c_int64)]
                + [(n, C.c_void_p) for n in VISITS_INPUTS + VISITS_FORWARD + VISITS_BACKWARD + ("stream",)])


def bind(L):
    """Prototypes of EXPORTS on the loaded library; ImportError if it lacks one (there is no fallback).  Returns L."""
    return bind_exports(L, {name: PcbenvVisitsRequest for name in EXPORTS})
