"""ctypes binding of libegs_kmeans.so (the C ABI declared in include/egs_kmeans.h): Lloyd's k-means on the device -- the
nearest-centroid assignment on the f32 matrix cores and the weighted centroid update in fixed-size chunks -- for the SH
codebook of a compressed scene file (``compress``).

A library of its own beside libegs_hip.so (``_lib``) and the other side libraries, built by the same ``make``
(``_lib.build()``), with its own ABI number and its own last-error string.  As there, there is NO fallback: a missing or stale
library raises.  It is loaded by the first call into ``compress`` that needs a kernel, never by training.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libegs_kmeans.so")
ABI_VERSION = 1
ERR_BAD_ARG = 10001                    # include/egs_kmeans.h EGS_KMEANS_ERR_BAD_ARG
MAX_BLOCKS = 8192                      # EGS_KMEANS_MAX_BLOCKS
MAX_D = 64                             # EGS_KMEANS_MAX_D
MAX_K = 65536                          # EGS_KMEANS_MAX_K
ROWS = 256                             # EGS_KMEANS_ROWS: rows per workgroup of the assign kernel
TILE = 64                              # EGS_KMEANS_TILE: centroids per LDS tile of the assign kernel
CHUNK = 256                            # EGS_KMEANS_CHUNK: members per chunk of the update

_P = C.c_void_p
_i = C.c_int
_sz = C.c_size_t

# name -> (restype, argtypes); must list every symbol include/egs_kmeans.h declares
SIGNATURES = {
    "egs_kmeans_abi_version": (_i, []),
    "egs_kmeans_last_error_string": (C.c_char_p, []),
    "egs_kmeans_assign": (_i, [_i, _i, _i, _P, _P, _P, _P, _P, _i, _P]),
    "egs_kmeans_update_ws_bytes": (_sz, [_i, _i, _i]),
    "egs_kmeans_update": (_i, [_i, _i, _i, _P, _P, _P, _P, _P, _P, _P, _P, _sz, _i, _P]),
}

_lib = None


def load():
    """Load the library once; raise EgsLibraryError if it is absent or stale."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "egs_kmeans_abi_version", ABI_VERSION)
    return _lib


def check(rc: int):
    if rc != 0:
        msg = load().egs_kmeans_last_error_string().decode("utf-8", "replace")
        raise RuntimeError(msg)
