"""ctypes binding of the MI355X BGZF block compressor (bmz_* in libbmf.so, C ABI in include/bmz.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _bmf_lib

BMZ_OK, BMZ_ERR_ARG, BMZ_ERR_HIP = 0, 1, 2
BLOCK_MAX = 65280         # BMZ_BLOCK_MAX
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")   # the BGZF end-of-file block


class BmzError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bmz error {code}: {msg}")
        self.code = code


_u8p, _u32p, _u64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64))

SYMBOLS = {
    "bmz_last_error": (C.c_char_p, []),
    "bmz_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "bmz_destroy": (None, [C.c_void_p]),
    "bmz_bound": (C.c_uint64, [C.c_uint64, C.c_uint32]),
    "bmz_deflate": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, C.c_uint32, _u8p, C.c_uint64, _u64p]),
    "bmz_blocks": (C.c_int, [C.c_void_p, _u64p]),
    "bmz_last_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), _u32p, _u32p, _u32p]),
}
_ready = False


def lib() -> C.CDLL:
    global _ready
    L = _bmf_lib()
    if not _ready:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _ready = True
    return L


def _check(rc: int) -> None:
    if rc != BMZ_OK:
        raise BmzError(rc, lib().bmz_last_error().decode(errors="replace"))


def bound(n_bytes: int, block_bytes: int = BLOCK_MAX) -> int:
    return int(lib().bmz_bound(n_bytes, block_bytes))


class Compressor:
    """One bmz_ctx.  deflate() returns (the blocks as bytes, the n_blocks + 1 offsets, [n_stored, n_fixed, n_dynamic])."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().bmz_create(device, C.byref(self._h)))
        self.ms_kernels = 0.0

    def deflate(self, data, block_bytes: int = BLOCK_MAX, out_cap: int | None = None):
        a = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
        n_blocks = (a.size + block_bytes - 1) // block_bytes if block_bytes > 0 else 0
        cap = bound(a.size, block_bytes) if out_cap is None else out_cap
        out = np.empty(max(cap, 1), np.uint8)
        got = C.c_uint64(0)
        _check(lib().bmz_deflate(self._h, a.ctypes.data_as(_u8p), a.size, block_bytes, out.ctypes.data_as(_u8p), cap, C.byref(got)))
        offsets = np.zeros(n_blocks + 1, np.uint64)
        _check(lib().bmz_blocks(self._h, offsets.ctypes.data_as(_u64p)))
        ms, f = C.c_float(0), [C.c_uint32(0) for _ in range(3)]
        _check(lib().bmz_last_stats(self._h, C.byref(ms), *[C.byref(x) for x in f]))
        self.ms_kernels = float(ms.value)
        return out[: got.value].tobytes(), [int(x) for x in offsets], [int(x.value) for x in f]

    def close(self) -> None:
        if self._h:
            lib().bmz_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
