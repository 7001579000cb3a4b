"""ctypes binding of include/pcbenv_priors.h: pcbenv_top_priors, which libpcbenv.so exports beyond include/pcbenv.h and
include/pcbenv_search.h.  `bind(L)` sets the prototype on the library `_lib.load()` returns; nothing is added to `_lib`'s
namespace."""
from __future__ import annotations

import ctypes as C

from ._lib import bind_exports

EXPORTS = ("pcbenv_top_priors",)

TOP_PRIORS_INPUTS = ("logits", "mask_bits")
TOP_PRIORS_OUTPUTS = ("cand_count", "cand_actions", "cand_prior")


class PcbenvTopPriorsRequest(C.Structure):
    """pcbenv_top_priors_request (include/pcbenv_priors.h), the arguments of pcbenv_top_priors."""
    _fields_ = ([("struct_size", C.c_uint32), ("logits_dtype", C.c_int32), ("num_candidates", C.c_int32), ("reserved", C.c_int32),
                 ("num_rows", C.c_int64)]
                + [(n, C.c_void_p) for n in TOP_PRIORS_INPUTS + TOP_PRIORS_OUTPUTS + ("errors_dev", "stream")])


def bind(L):
    """Prototypes of EXPORTS on the loaded library; ImportError if it lacks one (there is no fallback).  Returns L."""
    return bind_exports(L, {name: PcbenvTopPriorsRequest for name in EXPORTS})
