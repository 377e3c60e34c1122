"""ctypes binding of the MI355X BAM record sorter (bms_* in libbmf.so, C ABI and the order in include/bms.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _bmf_lib
from .bgzf import BLOCK_MAX, bound

BMS_OK, BMS_ERR_ARG, BMS_ERR_HIP = 0, 1, 2
MIN_RECORD = 36           # BMS_MIN_RECORD


class BmsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bms error {code}: {msg}")
        self.code = code


_u8p, _u32p, _u64p, _f32p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64, C.c_float))

SYMBOLS = {
    "bms_last_error": (C.c_char_p, []),
    "bms_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "bms_destroy": (None, [C.c_void_p]),
    "bms_sort": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, C.c_uint64, _u8p, _u32p, _u64p]),
    "bms_sort_deflate": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, C.c_uint64, C.c_uint32, _u8p, C.c_uint64, _u64p, _u32p, _u64p]),
    "bms_last_stats": (C.c_int, [C.c_void_p, _f32p, _f32p, _f32p, _u32p]),
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
    if rc != BMS_OK:
        raise BmsError(rc, lib().bms_last_error().decode(errors="replace"))


def record_offsets(stream) -> np.ndarray:
    """The n + 1 offsets of the records of a BAM stream, read from their block_size fields."""
    b = bytes(stream)
    out, at = [0], 0
    while at < len(b):
        at += 4 + int.from_bytes(b[at: at + 4], "little")
        out.append(at)
    return np.asarray(out, np.uint64)


class Sorter:
    """One bms_ctx.  sort() returns (the sorted stream as bytes, perm, sorted_offset); sort_deflate() returns (the BGZF blocks
    of the sorted stream, perm, sorted_offset).  After either, ms_sort / ms_gather / ms_deflate / n_passes hold bms_last_stats."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().bms_create(device, C.byref(self._h)))
        self.ms_sort = self.ms_gather = self.ms_deflate = 0.0
        self.n_passes = 0

    @staticmethod
    def _inputs(stream, rec_offset):
        a = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else np.ascontiguousarray(stream, np.uint8)
        off = record_offsets(a.tobytes()) if rec_offset is None else np.ascontiguousarray(rec_offset, np.uint64)
        n = max(off.size - 1, 0)
        return a, off, n, np.zeros(max(n, 1), np.uint32), np.zeros(n + 1, np.uint64)

    def _stats(self) -> None:
        ms, p = [C.c_float(0) for _ in range(3)], C.c_uint32(0)
        _check(lib().bms_last_stats(self._h, *[C.byref(x) for x in ms], C.byref(p)))
        self.ms_sort, self.ms_gather, self.ms_deflate = (float(x.value) for x in ms)
        self.n_passes = int(p.value)

    def sort(self, stream, rec_offset=None):
        a, off, n, perm, so = self._inputs(stream, rec_offset)
        out = np.empty(max(a.size, 1), np.uint8)
        _check(lib().bms_sort(self._h, a.ctypes.data_as(_u8p), a.size, off.ctypes.data_as(_u64p), n, out.ctypes.data_as(_u8p),
                              perm.ctypes.data_as(_u32p), so.ctypes.data_as(_u64p)))
        self._stats()
        return out[: a.size].tobytes(), perm[:n], so

    def sort_deflate(self, stream, rec_offset=None, block_bytes: int = BLOCK_MAX, out_cap: int | None = None):
        a, off, n, perm, so = self._inputs(stream, rec_offset)
        cap = bound(a.size, block_bytes) if out_cap is None else out_cap
        out = np.empty(max(cap, 1), np.uint8)
        got = C.c_uint64(0)
        _check(lib().bms_sort_deflate(self._h, a.ctypes.data_as(_u8p), a.size, off.ctypes.data_as(_u64p), n, block_bytes,
                                      out.ctypes.data_as(_u8p), cap, C.byref(got), perm.ctypes.data_as(_u32p), so.ctypes.data_as(_u64p)))
        self._stats()
        return out[: got.value].tobytes(), perm[:n], so

    def close(self) -> None:
        if self._h:
            lib().bms_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
