"""ctypes binding of libegs_simplify.so (the C ABI declared in include/egs_simplify.h): vertex-clustering simplification of
an indexed triangle mesh on the device with quadric-optimal cluster representatives -- cell keys, per-vertex quadrics, the
per-cluster solve, the face remap and the first-of-run flags.

A library of its own beside libegs_hip.so (``_lib``) and the other side libraries (``_meshopslib`` among them, whose
compaction it is used with), built by the same ``make`` (``_lib.build()``), with its own ABI number and its own last-error
string.  As there, there is NO fallback: a missing or stale library raises.  It is loaded by the first call of
``mesh.simplify_vertex_clustering``, never by training.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libegs_simplify.so")
ABI_VERSION = 1
ERR_BAD_ARG = 10001                    # include/egs_simplify.h EGS_SIMPLIFY_ERR_BAD_ARG
MAX_BLOCKS = 8192                      # EGS_SIMPLIFY_MAX_BLOCKS
KEY_BITS = 21                          # EGS_SIMPLIFY_KEY_BITS: a cell index per axis lies in [0, 2^21)
PLACE_QUADRIC = 0                      # EGS_SIMPLIFY_PLACE_QUADRIC
PLACE_MEAN = 1                         # EGS_SIMPLIFY_PLACE_MEAN

_P = C.c_void_p
_i = C.c_int
_d = C.c_double

# name -> (restype, argtypes); must list every symbol include/egs_simplify.h declares
SIGNATURES = {
    "egs_simplify_abi_version": (_i, []),
    "egs_simplify_last_error_string": (C.c_char_p, []),
    "egs_simplify_keys": (_i, [_i, _P, _d, _d, _d, _d, _P, _i, _P]),
    "egs_simplify_vertex_quadrics": (_i, [_i, _i, _P, _P, _P, _P, _P, _d, _d, _d, _d, _P, _i, _P]),
    "egs_simplify_clusters": (_i, [_i, _i, _i, _P, _P, _P, _P, _P, _P, _P, _P, _P, _d, _d, _d, _d, _i, _P, _P, _P, _i, _P]),
    "egs_simplify_remap_faces": (_i, [_i, _i, _i, _P, _P, _P, _P, _P, _P, _i, _P]),
    "egs_simplify_keep_flags": (_i, [_i, _i, _P, _P, _P, _P, _P, _P, _P, _i, _P]),
}

_lib = None


def load():
    """Load the library once; raise EgsLibraryError if it is absent or stale."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "egs_simplify_abi_version", ABI_VERSION)
    return _lib


def check(rc: int):
    if rc != 0:
        msg = load().egs_simplify_last_error_string().decode("utf-8", "replace")
        raise RuntimeError(msg)
