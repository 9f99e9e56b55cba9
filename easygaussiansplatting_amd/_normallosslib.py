"""ctypes binding of libegs_normalloss.so (the C ABI declared in include/egs_normalloss.h): surface-normal supervision and
edge-aware normal smoothness on the render's depth and opacity maps.

A library of its own beside libegs_hip.so (``_lib``) and the other side libraries (``_mcmclib``, ``_prunelib``,
``_featlib``, ``_adamlib``, ``_bilagridlib``, ``_wlosslib``, ``_depthlosslib``), built by the same ``make``
(``_lib.build()``), with its own ABI number and its own last-error string.  As there, there is NO fallback: a missing or
stale library raises.  It is loaded by the first normal-loss call, never by a training step without normal terms.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libegs_normalloss.so")
ABI_VERSION = 1
ERR_BAD_ARG = 10001
ERR_WORKSPACE = 10002
MAX_PIXELS = 1 << 26                   # include/egs_normalloss.h EGS_NORMALLOSS_MAX_PIXELS
TILE_W, TILE_H = 32, 8                 # EGS_NORMALLOSS_TILE_W / _TILE_H

_P = C.c_void_p
_i = C.c_int
_f = C.c_float
_sz = C.c_size_t

# name -> (restype, argtypes); must list every symbol include/egs_normalloss.h declares
SIGNATURES = {
    "egs_normalloss_abi_version": (_i, []),
    "egs_normalloss_last_error_string": (C.c_char_p, []),
    "egs_normalloss_ws_bytes": (_sz, [_i, _i]),
    "egs_normalloss": (_i, [_i, _i, _P, _P, _f, _f, _f, _f, _P, _P, _P, _i, _f, _f, _f, _f, _P, _sz, _P, _P, _P, _P,
                            _P]),
}

_lib = None


def load():
    """Load the library once; raise EgsLibraryError if it is absent or stale."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "egs_normalloss_abi_version", ABI_VERSION)
    return _lib


def check(rc: int):
    if rc != 0:
        msg = load().egs_normalloss_last_error_string().decode("utf-8", "replace")
        raise RuntimeError(msg)
