"""ctypes binding of libegs_feat.so (the C ABI declared in include/egs_feat.h): per-Gaussian feature vectors rendered
through the tile lists of a finished forward pass, and the adjoint of that render.

A fourth library beside libegs_hip.so (``_lib``), libegs_mcmc.so (``_mcmclib``) and libegs_prune.so (``_prunelib``), built by the same ``make``
(``_lib.build()``), with its own ABI number and its own last-error string.  As there, there is NO fallback: a missing or
stale library raises.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import DRAW_MASKED_LISTS, EgsPolicy, load_library  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libegs_feat.so")
ABI_VERSION = 1
ERR_BAD_ARG = 10001
MAX_CHANNELS = 4096        # include/egs_feat.h EGS_FEAT_MAX_CHANNELS

_P = C.c_void_p
_i = C.c_int

# name -> (restype, argtypes); must list every symbol include/egs_feat.h declares
SIGNATURES = {
    "egs_feat_abi_version": (_i, []),
    "egs_feat_last_error_string": (C.c_char_p, []),
    "egs_feature_render": (_i, [_i, _i, _i, _P, C.POINTER(EgsPolicy), _P, _P, _P, _i, _i, _P, _P, _P]),
    "egs_feature_gather": (_i, [_i, _i, _i, _P, C.POINTER(EgsPolicy), _P, _P, _P, _i, _i, _P, _P, _P]),
}

_lib = None


def load():
    """Load the library once; raise EgsLibraryError if it is absent or stale."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "egs_feat_abi_version", ABI_VERSION)
    return _lib


def check(rc: int):
    if rc != 0:
        msg = load().egs_feat_last_error_string().decode("utf-8", "replace")
        raise RuntimeError(msg)
