"""ctypes binding of the MI355X reference-block pass (bmr_* in libbmf.so, C ABI and the rule in include/bmr.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _bmf_lib

BMR_OK, BMR_ERR_ARG, BMR_ERR_HIP = 0, 1, 2
MAX_BANDS, BLOCK_WORDS, CONF_WORDS, EXCLUDE_WORDS = 16, 8, 2, 3
IN, EXCLUDED, NO_ALLELE = 1 << 16, 1 << 17, 1 << 18
DEFAULT_BANDS = (1, 10, 20, 30, 40, 50, 60, 70, 80, 90, 99)   # the command line's
# the words of a block
W_REF, W_START, W_END, W_BAND, W_MIN_GQ, W_MIN_DP, W_SUM_DP = 0, 1, 2, 3, 4, 5, 6


class BmrError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bmr error {code}: {msg}")
        self.code = code


_u8p, _u32p, _u64p, _f32p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64, C.c_float))

SYMBOLS = {
    "bmr_last_error": (C.c_char_p, []),
    "bmr_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "bmr_destroy": (None, [C.c_void_p]),
    "bmr_run": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), _u32p, C.c_uint32, _u32p, C.c_uint64, _u64p]),
    "bmr_blocks": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, _u32p]),
    "bmr_conf_at": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _u32p]),
    "bmr_last_stats": (C.c_int, [C.c_void_p, _f32p, _u64p]),
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
    if rc != BMR_OK:
        raise BmrError(rc, lib().bmr_last_error().decode(errors="replace"))


class RefBlocks:
    """One bmr_ctx.  run(cells, ref_bases, bands, exclude) -> the number of blocks, for a genotype.Genotype after begin() and
    any number of add(), one bytes object per reference, the band bounds and (reference, start, end) intervals; then
    blocks(first, count) -> a (count, 8) uint32 array and conf_at(ref, start, count) -> a (count, 2) uint32 array.  After a
    run ms_kernels / bytes_state hold bmr_last_stats."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().bmr_create(device, C.byref(self._h)))
        self.ms_kernels, self.bytes_state, self.n_blocks = 0.0, 0, 0

    def run(self, cells, ref_bases, bands=DEFAULT_BANDS, exclude=()) -> int:
        keep = [np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else np.ascontiguousarray(b, np.uint8) for b in ref_bases]
        ptrs = (C.c_void_p * max(len(keep), 1))(*[a.ctypes.data if a.size else None for a in keep])
        bd = np.ascontiguousarray(bands, np.uint32).reshape(-1)
        ex = np.ascontiguousarray(exclude, np.uint32).reshape(-1, EXCLUDE_WORDS)
        n = C.c_uint64(0)
        _check(lib().bmr_run(self._h, cells._h, ptrs, bd.ctypes.data_as(_u32p) if bd.size else None, bd.size,
                             ex.ctypes.data_as(_u32p) if ex.size else None, ex.shape[0], C.byref(n)))
        ms, held = C.c_float(0), C.c_uint64(0)
        _check(lib().bmr_last_stats(self._h, C.byref(ms), C.byref(held)))
        self.ms_kernels, self.bytes_state, self.n_blocks = float(ms.value), int(held.value), int(n.value)
        return self.n_blocks

    def blocks(self, first: int = 0, count: int | None = None):
        count = self.n_blocks - first if count is None else count
        out = np.zeros((max(count, 1), BLOCK_WORDS), np.uint32)
        _check(lib().bmr_blocks(self._h, first, count, out.ctypes.data_as(_u32p)))
        return out[:count]

    def conf_at(self, ref: int, start: int, count: int):
        out = np.zeros((max(count, 1), CONF_WORDS), np.uint32)
        _check(lib().bmr_conf_at(self._h, ref, start, count, out.ctypes.data_as(_u32p)))
        return out[:count]

    def close(self) -> None:
        if self._h:
            lib().bmr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
