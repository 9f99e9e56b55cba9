"""Helpers of the GPU tests that call the C ABI directly: the policy / stream / pointer arguments and device output
buffers with sentinel bands in front of and behind them."""
import ctypes as C

import numpy as np
import torch

BAND = 2048                                         # sentinel words in front of and behind every output
DEV = "cuda"


def _pol():
    from easygaussiansplatting_amd import _host
    return _host._pol()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(lib, rc):
    assert rc == 0, (rc, lib.egs_last_error_string())


def _ptr(t):
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


# ----------------------------------------------------------------------------------------------------- sentinel bands
def _sentinel(words):
    """quiet-NaN words with a running payload: an untouched word is recognisable, a shifted one too"""
    return (np.int32(0x7FC00000) + (np.arange(words, dtype=np.int32) & 0xFFFF)).astype(np.int32)


class Out:
    """a device buffer [BAND | words | BAND] of 32-bit words, sentinel-filled unless ``content`` is given"""

    def __init__(self, words, content=None):
        self.words = words
        self.before = _sentinel(words + 2 * BAND)
        if content is not None:
            self.before[BAND:BAND + words] = np.ascontiguousarray(content).reshape(-1).view(np.int32)
        self.t = torch.from_numpy(self.before.copy()).to(DEV)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + 4 * BAND)          # 8 KiB in: 16-B aligned like the allocation

    def read(self, what):
        """-> the words as int32 after checking both bands"""
        got = self.t.cpu().numpy()
        assert np.array_equal(got[:BAND], self.before[:BAND]), (what, "written in front of the output")
        assert np.array_equal(got[BAND + self.words:], self.before[BAND + self.words:]), (what, "written behind it")
        return got[BAND:BAND + self.words]

    def old(self):
        return self.before[BAND:BAND + self.words]
