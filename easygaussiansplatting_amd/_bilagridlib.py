"""ctypes binding of libegs_bilagrid.so (the C ABI declared in include/egs_bilagrid.h): slicing an image through a
bilateral grid of affine colour transforms, the adjoint of that, and the grid's total variation.

A library of its own beside libegs_hip.so (``_lib``) and the other side libraries (``_mcmclib``, ``_prunelib``,
``_featlib``, ``_adamlib``), built by the same ``make`` (``_lib.build()``), with its own ABI number and its own last-error
string.  As there, there is NO fallback: a missing or stale library raises.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libegs_bilagrid.so")
ABI_VERSION = 1
ERR_BAD_ARG = 10001
# include/egs_bilagrid.h
BLOCK_W, BLOCK_H = 64, 32              # EGS_BILAGRID_BLOCK_W / _H: the pixel block of one workgroup
LDS_FLOATS = 8192                      # EGS_BILAGRID_LDS_FLOATS: the LDS budget of one box of lattice nodes
MAX_GRID_FLOATS = 1 << 24              # EGS_BILAGRID_MAX_GRID_FLOATS
MAX_COORD_PRODUCT = 1 << 22            # EGS_BILAGRID_MAX_COORD_PRODUCT

_P = C.c_void_p
_i = C.c_int

# name -> (restype, argtypes); must list every symbol include/egs_bilagrid.h declares
SIGNATURES = {
    "egs_bilagrid_abi_version": (_i, []),
    "egs_bilagrid_last_error_string": (C.c_char_p, []),
    "egs_bilagrid_slice": (_i, [_i, _P, _i, _i, _i, _i, _i, _P, _P, _P]),
    "egs_bilagrid_slice_bwd": (_i, [_i, _P, _i, _i, _i, _i, _i, _P, _P, _P, _P, _P]),
    "egs_bilagrid_tv": (_i, [_i, _P, _i, _i, _i, _P, C.c_float, _P, _P]),
}

_lib = None


def load():
    """Load the library once; raise EgsLibraryError if it is absent or stale."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "egs_bilagrid_abi_version", ABI_VERSION)
    return _lib


def check(rc: int):
    if rc != 0:
        msg = load().egs_bilagrid_last_error_string().decode("utf-8", "replace")
        raise RuntimeError(msg)
