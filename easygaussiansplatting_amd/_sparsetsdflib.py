"""ctypes binding of libegs_sparsetsdf.so (the C ABI declared in include/egs_sparse_tsdf.h): the block-allocated TSDF
volume -- allocation of the 8^3 blocks a view's truncation band meets, fusion into the allocated blocks, extraction of the
zero level set per block.

A library of its own beside libegs_hip.so (``_lib``), libegs_tsdf.so (``_tsdflib``) and the other side libraries, built by
the same ``make`` (``_lib.build()``), with its own ABI number and its own last-error string.  As there, there is NO
fallback: a missing or stale library raises.  It is loaded by the first ``mesh.SparseTSDFVolume`` call, never by training.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libegs_sparsetsdf.so")
ABI_VERSION = 1
ERR_BAD_ARG = 10001
ERR_CAPACITY = 10003                   # include/egs_sparse_tsdf.h EGS_SPARSETSDF_ERR_CAPACITY
BLOCK = 8                              # EGS_SPARSETSDF_BLOCK
BLOCK_SAMPLES = 512                    # EGS_SPARSETSDF_BLOCK_SAMPLES
MAX_DIRECTORY = 1 << 27                # EGS_SPARSETSDF_MAX_DIRECTORY
MAX_SLOTS = 1 << 22                    # EGS_SPARSETSDF_MAX_SLOTS
MAX_BLOCKS = 8192                      # EGS_SPARSETSDF_MAX_BLOCKS
MAX_MARCH = 4096                       # EGS_SPARSETSDF_MAX_MARCH

_P = C.c_void_p
_i = C.c_int
_f = C.c_float
_i64 = C.c_int64

# name -> (restype, argtypes); must list every symbol include/egs_sparse_tsdf.h declares
SIGNATURES = {
    "egs_sparsetsdf_abi_version": (_i, []),
    "egs_sparsetsdf_last_error_string": (C.c_char_p, []),
    "egs_sparsetsdf_touch": (_i, [_i, _i, _i, _f, _f, _f, _f, _i, _i, _P, _P, _P, _f, _f, _f, _f, _P, _P, _f, _f, _f, _f,
                                  _P, _P]),
    "egs_sparsetsdf_mark": (_i, [_i, _i, _i, _P, _P, _P, _P]),
    "egs_sparsetsdf_assign": (_i, [_i, _i, _i, _P, _P, _i, _i, _P, _P, _P]),
    "egs_sparsetsdf_integrate": (_i, [_i, _i, _i, _f, _f, _f, _f, _i, _i, _P, _P, _P, _P, _i, _i, _P, _P, _P, _P,
                                      _f, _f, _f, _f, _P, _P, _f, _f, _f, _f, _i, _P]),
    "egs_sparsetsdf_mesh_count": (_i, [_i, _i, _i, _i, _i, _P, _P, _P, _P, _f, _P, _P]),
    "egs_sparsetsdf_mesh_emit": (_i, [_i, _i, _i, _f, _f, _f, _f, _i, _i, _P, _P, _P, _P, _P, _f, _P, _i64, _i64, _P, _P,
                                      _P, _P]),
}

_lib = None


def load():
    """Load the library once; raise EgsLibraryError if it is absent or stale."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SIGNATURES, "egs_sparsetsdf_abi_version", ABI_VERSION)
    return _lib


def check(rc: int):
    if rc != 0:
        msg = load().egs_sparsetsdf_last_error_string().decode("utf-8", "replace")
        raise RuntimeError(msg)
