"""ctypes binding of libegs_adam.so (the C ABI declared in include/egs_adam.h): visibility-masked ("sparse") Adam.

A library of its own beside libegs_hip.so (``_lib``), libegs_mcmc.so, libegs_prune.so and libegs_feat.so, built by the
same ``make`` (``_lib.build()``), with its own ABI number and its own last-error string.  As there, there is NO fallback:
a missing or stale library raises.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import EgsAdamGroup, load_library  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libegs_adam.so")
ABI_VERSION = 1
ERR_BAD_ARG = 10001
MAX_GROUPS = 8             # include/egs_adam.h EGS_SPARSE_ADAM_MAX_GROUPS


class EgsSparseAdamGroup(C.Structure):
    """Mirror of `struct EgsSparseAdamGroup`: one [n][width] tensor with its gradient and moments."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("width", C.c_int32), ("lr", C.c_float), ("step", C.c_int32)]


_P = C.c_void_p
_i = C.c_int
_d = C.c_double

# name -> (restype, argtypes); must list every symbol include/egs_adam.h declares
SIGNATURES = {
    "egs_adam_abi_version": (_i, []),
    "egs_adam_last_error_string": (C.c_char_p, []),
    "egs_sparse_adam_step": (_i, [_i, C.POINTER(EgsSparseAdamGroup), _i, _P, _d, _d, _d, _P]),
    "egs_sparse_adam_sh_factored": (_i, [_i, _i, _i, _P, _P, C.c_int64, C.c_float, C.POINTER(EgsAdamGroup),
                                         C.POINTER(EgsAdamGroup), _P, _d, _d, _d, _P]),
}

_lib = None


def load():
    """Load the library once; raise EgsLibraryError if it is absent or stale."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "egs_adam_abi_version", ABI_VERSION)
    return _lib


def check(rc: int):
    if rc != 0:
        msg = load().egs_adam_last_error_string().decode("utf-8", "replace")
        raise RuntimeError(msg)
