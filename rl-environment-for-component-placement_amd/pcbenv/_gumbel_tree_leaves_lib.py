"""ctypes binding of include/pcbenv_gumbel_tree_leaves.h: pcbenv_gumbel_tree_advance_leaves, which libpcbenv.so exports beyond
include/pcbenv.h, include/pcbenv_search.h, include/pcbenv_priors.h, include/pcbenv_move.h, include/pcbenv_leaves.h,
include/pcbenv_noise.h, include/pcbenv_gumbel.h, include/pcbenv_gumbel_leaves.h and include/pcbenv_gumbel_tree.h.  `bind(L)` sets
the prototype on the library `_lib.load()` returns; nothing is added to `_lib`'s namespace.  The request and the phases are
`_gumbel_leaves_lib`'s: the entry point takes pcbenv_gumbel_leaves_request as it is."""
from __future__ import annotations

from ._gumbel_leaves_lib import PcbenvGumbelLeavesRequest
from ._lib import bind_exports

EXPORTS = ("pcbenv_gumbel_tree_advance_leaves",)


def bind(L):
    """Prototypes of EXPORTS on the loaded library; ImportError if it lacks one (there is no fallback).  Returns L."""
    return bind_exports(L, {name: PcbenvGumbelLeavesRequest for name in EXPORTS})
