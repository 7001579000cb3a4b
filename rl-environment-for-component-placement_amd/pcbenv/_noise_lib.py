"""ctypes binding of include/pcbenv_noise.h: pcbenv_puct_root_noise, which libpcbenv.so exports beyond include/pcbenv.h,
include/pcbenv_search.h, include/pcbenv_priors.h and include/pcbenv_move.h.  `bind(L)` sets the prototype on the library
`_lib.load()` returns; nothing is added to `_lib`'s namespace."""
from __future__ import annotations

import ctypes as C

from ._lib import bind_exports

EXPORTS = ("pcbenv_puct_root_noise",)

NOISE_TENSORS = ("num_children", "first_child", "prior", "noised")


class PcbenvPuctNoiseRequest(C.Structure):
    """pcbenv_puct_noise_request (include/pcbenv_noise.h), the arguments of pcbenv_puct_root_noise."""
    _fields_ = ([("struct_size", C.c_uint32), ("num_roots", C.c_int32), ("capacity", C.c_int32), ("max_children", C.c_int32),
                 ("first_root", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("step_index", C.c_uint64),
                 ("alpha", C.c_double), ("eps", C.c_double)]
                + [(n, C.c_void_p) for n in NOISE_TENSORS + ("errors_dev", "stream")])


def bind(L):
    """Prototypes of EXPORTS on the loaded library; ImportError if it lacks one (there is no fallback).  Returns L."""
    return bind_exports(L, {name: PcbenvPuctNoiseRequest for name in EXPORTS})
