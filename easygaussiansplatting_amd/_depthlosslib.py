"""ctypes binding of libegs_depthloss.so (the C ABI declared in include/egs_depthloss.h): the depth-prior loss on the
render's depth and opacity maps.

A library of its own beside libegs_hip.so (``_lib``) and the other side libraries (``_mcmclib``, ``_prunelib``,
``_featlib``, ``_adamlib``, ``_bilagridlib``, ``_wlosslib``), built by the same ``make`` (``_lib.build()``), with its own
ABI number and its own last-error string.  As there, there is NO fallback: a missing or stale library raises.  It is
loaded by the first depth-loss call, never by a training step without depth priors.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libegs_depthloss.so")
ABI_VERSION = 1
ERR_BAD_ARG = 10001
ERR_WORKSPACE = 10002
MAX_PIXELS = 1 << 28                   # include/egs_depthloss.h EGS_DEPTHLOSS_MAX_PIXELS
KINDS = {"metric": 0, "affine": 1, "pearson": 2}      # EGS_DEPTHLOSS_METRIC / _AFFINE / _PEARSON

_P = C.c_void_p
_i = C.c_int
_f = C.c_float
_sz = C.c_size_t

# name -> (restype, argtypes); must list every symbol include/egs_depthloss.h declares
SIGNATURES = {
    "egs_depthloss_abi_version": (_i, []),
    "egs_depthloss_last_error_string": (C.c_char_p, []),
    "egs_depthloss_ws_bytes": (_sz, [_i, _i]),
    "egs_depthloss": (_i, [_i, _i, _P, _P, _P, _P, _i, _f, _f, _P, _sz, _P, _P, _P, _P]),
}

_lib = None


def load():
    """Load the library once; raise EgsLibraryError if it is absent or stale."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "egs_depthloss_abi_version", ABI_VERSION)
    return _lib


def check(rc: int):
    if rc != 0:
        msg = load().egs_depthloss_last_error_string().decode("utf-8", "replace")
        raise RuntimeError(msg)
