"""ctypes binding of libegs_prune.so (the C ABI declared in include/egs_prune.h): per-Gaussian blend-weight statistics.

A third library beside libegs_hip.so (``_lib``) and libegs_mcmc.so (``_mcmclib``), built by the same ``make``
(``_lib.build()``), with its own ABI number and its own last-error string.  As there, there is NO fallback: a missing or
stale library raises.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import DRAW_MASKED_LISTS, EgsPolicy, load_library  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libegs_prune.so")
ABI_VERSION = 1
ERR_BAD_ARG = 10001

_P = C.c_void_p
_i = C.c_int

# name -> (restype, argtypes); must list every symbol include/egs_prune.h declares
SIGNATURES = {
    "egs_prune_abi_version": (_i, []),
    "egs_prune_last_error_string": (C.c_char_p, []),
    "egs_blend_weights": (_i, [_i, _i, _i, _P, C.POINTER(EgsPolicy), _P, _P, _P, _i, _P, _P]),
}

_lib = None


def load():
    """Load the library once; raise EgsLibraryError if it is absent or stale."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "egs_prune_abi_version", ABI_VERSION)
    return _lib


def check(rc: int):
    if rc != 0:
        msg = load().egs_prune_last_error_string().decode("utf-8", "replace")
        raise RuntimeError(msg)
