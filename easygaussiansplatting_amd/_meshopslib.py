"""ctypes binding of libegs_meshops.so (the C ABI declared in include/egs_meshops.h): connected components, removal of
small components with compaction, vertex normals and Taubin smoothing of an indexed triangle mesh on the device.

A library of its own beside libegs_hip.so (``_lib``) and the other side libraries (``_tsdflib`` among them), built by the
same ``make`` (``_lib.build()``), with its own ABI number and its own last-error string.  As there, there is NO fallback: a
missing or stale library raises.  It is loaded by the first call of one of ``mesh``'s cleaning functions, never by
training.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libegs_meshops.so")
ABI_VERSION = 1
ERR_BAD_ARG = 10001                    # include/egs_meshops.h EGS_MESHOPS_ERR_BAD_ARG
MAX_BLOCKS = 8192                      # EGS_MESHOPS_MAX_BLOCKS
MAX_COUNT = (1 << 31) - 1              # V, F < 2^31

_P = C.c_void_p
_i = C.c_int
_d = C.c_double

# name -> (restype, argtypes); must list every symbol include/egs_meshops.h declares
SIGNATURES = {
    "egs_meshops_abi_version": (_i, []),
    "egs_meshops_last_error_string": (C.c_char_p, []),
    "egs_meshops_components": (_i, [_i, _i, _P, _P, _P, _P, _i, _P]),
    "egs_meshops_keep_flags": (_i, [_i, _i, _P, _P, _P, _P, _i, _i, _P, _P, _i, _P]),
    "egs_meshops_compact": (_i, [_i, _i, _P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _P, _P, _P, _P, _i, _P]),
    "egs_meshops_vertex_normals": (_i, [_i, _i, _P, _P, _P, _P, _P, _i, _P]),
    "egs_meshops_taubin": (_i, [_i, _i, _P, _P, _P, _P, _i, _d, _d, _P, _P, _i, _P]),
}

_lib = None


def load():
    """Load the library once; raise EgsLibraryError if it is absent or stale."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "egs_meshops_abi_version", ABI_VERSION)
    return _lib


def check(rc: int):
    if rc != 0:
        msg = load().egs_meshops_last_error_string().decode("utf-8", "replace")
        raise RuntimeError(msg)
