"""ctypes binding of libegs_tsdf.so (the C ABI declared in include/egs_tsdf.h): fusion of depth maps into a truncated
signed distance volume and extraction of its zero level set as a triangle mesh.

A library of its own beside libegs_hip.so (``_lib``) and the other side libraries (``_mcmclib``, ``_prunelib``,
``_featlib``, ``_adamlib``, ``_bilagridlib``, ``_wlosslib``, ``_depthlosslib``, ``_normallosslib``), built by the same
``make`` (``_lib.build()``), with its own ABI number and its own last-error string.  As there, there is NO fallback: a
missing or stale library raises.  It is loaded by the first ``mesh.TSDFVolume`` call, never by training.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libegs_tsdf.so")
ABI_VERSION = 1
ERR_BAD_ARG = 10001
ERR_CAPACITY = 10003                   # include/egs_tsdf.h EGS_TSDF_ERR_CAPACITY
MAX_BLOCKS = 8192                      # EGS_TSDF_MAX_BLOCKS
CELL_TRIANGLES = 12                    # EGS_TSDF_CELL_TRIANGLES
MAX_SAMPLES = (1 << 31) - 1            # nx ny nz < 2^31, and so is the number of triangles

_P = C.c_void_p
_i = C.c_int
_f = C.c_float
_i64 = C.c_int64

# name -> (restype, argtypes); must list every symbol include/egs_tsdf.h declares
SIGNATURES = {
    "egs_tsdf_abi_version": (_i, []),
    "egs_tsdf_last_error_string": (C.c_char_p, []),
    "egs_tsdf_integrate": (_i, [_i, _i, _i, _f, _f, _f, _f, _i, _i, _i, _i, _i, _i, _P, _P, _P, _i, _i, _P, _P, _P, _P,
                                _f, _f, _f, _f, _P, _P, _f, _f, _f, _f, _i, _P]),
    "egs_tsdf_mesh_count": (_i, [_i, _i, _i, _P, _P, _f, _P, _P]),
    "egs_tsdf_mesh_emit": (_i, [_i, _i, _i, _f, _f, _f, _f, _P, _P, _P, _f, _P, _i64, _i64, _P, _P, _P, _P]),
}

_lib = None


def load():
    """Load the library once; raise EgsLibraryError if it is absent or stale."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "egs_tsdf_abi_version", ABI_VERSION)
    return _lib


def check(rc: int):
    if rc != 0:
        msg = load().egs_tsdf_last_error_string().decode("utf-8", "replace")
        raise RuntimeError(msg)
