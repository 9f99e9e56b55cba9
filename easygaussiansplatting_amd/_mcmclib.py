"""ctypes binding of libegs_mcmc.so (the C ABI declared in include/egs_mcmc.h): MCMC densification.

A second library beside libegs_hip.so (``_lib``), built by the same ``make`` (``_lib.build()``), with its own ABI
number and its own last-error string.  As there, there is NO fallback: a missing or stale library raises.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import EgsGaussianParams, load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libegs_mcmc.so")
ABI_VERSION = 1
ERR_BAD_ARG = 10001
# random streams (include/egs_mcmc.h): sampling round r draws uniform01(seed, STREAM_SAMPLE + r, j), the noise of step t
# is unit_normal(seed, STREAM_NOISE + t, 3 i + c) == scene.normal(seed, STREAM_NOISE + t, (n, 3))
STREAM_SAMPLE = 1 << 62
STREAM_NOISE = 1 << 40
N_MAX = 51

_P = C.c_void_p
_PG = C.POINTER(EgsGaussianParams)
_f = C.c_float
_i = C.c_int
_u64 = C.c_uint64
_sz = C.c_size_t

# name -> (restype, argtypes); must list every symbol include/egs_mcmc.h declares
SIGNATURES = {
    "egs_mcmc_abi_version": (_i, []),
    "egs_mcmc_last_error_string": (C.c_char_p, []),
    "egs_mcmc_weights": (_i, [_i, _P, _f, _i, _P, _P, _P, _P]),
    "egs_mcmc_sample_ws_bytes": (_sz, [_i]),
    "egs_mcmc_sample": (_i, [_i, _P, _i, _i, _u64, _u64, _P, _P, _sz, _P]),
    "egs_mcmc_relocate_ws_bytes": (_sz, [_i]),
    "egs_mcmc_relocate": (_i, [_i, _i, _i, _P, _P, _PG, _PG, _PG, _f, _P, _sz, _P]),
    "egs_mcmc_add_reg_grad": (_i, [_i, _P, _P, _f, _f, _P, _P, _P]),
    "egs_mcmc_add_noise": (_i, [_i, _P, _P, _P, _P, _P, _f, _f, _u64, _u64, _P]),
}

_lib = None


def load():
    """Load the library once; raise EgsLibraryError if it is absent or stale."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "egs_mcmc_abi_version", ABI_VERSION)
    return _lib


def check(rc: int):
    if rc != 0:
        msg = load().egs_mcmc_last_error_string().decode("utf-8", "replace")
        raise RuntimeError(msg)
