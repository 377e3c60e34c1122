"""ctypes binding of the MI355X duplicate marker (bmd_* in libbmf.so, C ABI and the rule in include/bmd.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _bmf_lib
from .bamsort import record_offsets
from .bgzf import BLOCK_MAX, bound

BMD_OK, BMD_ERR_ARG, BMD_ERR_HIP = 0, 1, 2


class BmdError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bmd error {code}: {msg}")
        self.code = code


_u8p, _u32p, _u64p, _f32p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64, C.c_float))

SYMBOLS = {
    "bmd_last_error": (C.c_char_p, []),
    "bmd_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "bmd_destroy": (None, [C.c_void_p]),
    "bmd_ends": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, C.c_uint64, _u64p, _u64p, _u8p]),
    "bmd_mark": (C.c_int, [C.c_void_p, _u64p, _u64p, _u8p, C.c_uint64, _u8p, _u64p]),
    "bmd_mark_sort_deflate": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, C.c_uint64, C.c_uint32, _u8p, C.c_uint64, _u64p, _u32p, _u64p,
                                        _u8p, _u64p]),
    "bmd_last_stats": (C.c_int, [C.c_void_p, _f32p, _f32p, _u32p]),
    "bmd_last_sort_stats": (C.c_int, [C.c_void_p, _f32p, _f32p, _f32p, _u32p]),
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
    if rc != BMD_OK:
        raise BmdError(rc, lib().bmd_last_error().decode(errors="replace"))


class Marker:
    """One bmd_ctx.  ends() returns (end, score, kind); mark() returns (dup, counts); mark_sort_deflate() returns (the BGZF
    blocks of the marked, sorted stream, perm, sorted_offset, dup, counts).  counts = [pair units, fragment units, duplicate
    records from pair units, duplicate fragment records].  After a call ms_ends / ms_mark / n_passes hold bmd_last_stats and
    ms_sort / ms_gather / ms_deflate / n_sort_passes the sorter's share of a fused call."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().bmd_create(device, C.byref(self._h)))
        self.ms_ends = self.ms_mark = self.ms_sort = self.ms_gather = self.ms_deflate = 0.0
        self.n_passes = self.n_sort_passes = 0

    @staticmethod
    def _inputs(stream, rec_offset):
        a = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else np.ascontiguousarray(stream, np.uint8)
        off = record_offsets(a.tobytes()) if rec_offset is None else np.ascontiguousarray(rec_offset, np.uint64)
        return a, off, max(off.size - 1, 0)

    def _stats(self) -> None:
        ms, p = [C.c_float(0) for _ in range(2)], C.c_uint32(0)
        _check(lib().bmd_last_stats(self._h, *[C.byref(x) for x in ms], C.byref(p)))
        self.ms_ends, self.ms_mark = (float(x.value) for x in ms)
        self.n_passes = int(p.value)
        ms = [C.c_float(0) for _ in range(3)]
        _check(lib().bmd_last_sort_stats(self._h, *[C.byref(x) for x in ms], C.byref(p)))
        self.ms_sort, self.ms_gather, self.ms_deflate = (float(x.value) for x in ms)
        self.n_sort_passes = int(p.value)

    def ends(self, stream, rec_offset=None):
        a, off, n = self._inputs(stream, rec_offset)
        end, score, kind = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint8)
        _check(lib().bmd_ends(self._h, a.ctypes.data_as(_u8p), a.size, off.ctypes.data_as(_u64p), n, end.ctypes.data_as(_u64p),
                              score.ctypes.data_as(_u64p), kind.ctypes.data_as(_u8p)))
        self._stats()
        return end[:n], score[:n], kind[:n]

    def mark(self, end, score, kind):
        end, score = np.ascontiguousarray(end, np.uint64), np.ascontiguousarray(score, np.uint64)
        kind = np.ascontiguousarray(kind, np.uint8)
        n = end.size
        assert score.size == n and kind.size == n
        dup, counts = np.zeros(max(n, 1), np.uint8), np.zeros(4, np.uint64)
        _check(lib().bmd_mark(self._h, end.ctypes.data_as(_u64p), score.ctypes.data_as(_u64p), kind.ctypes.data_as(_u8p), n,
                              dup.ctypes.data_as(_u8p), counts.ctypes.data_as(_u64p)))
        self._stats()
        return dup[:n], [int(x) for x in counts]

    def mark_sort_deflate(self, stream, rec_offset=None, block_bytes: int = BLOCK_MAX, out_cap: int | None = None):
        a, off, n = self._inputs(stream, rec_offset)
        cap = bound(a.size, block_bytes) if out_cap is None else out_cap
        out, perm, so = np.empty(max(cap, 1), np.uint8), np.zeros(max(n, 1), np.uint32), np.zeros(n + 1, np.uint64)
        dup, counts, got = np.zeros(max(n, 1), np.uint8), np.zeros(4, np.uint64), C.c_uint64(0)
        _check(lib().bmd_mark_sort_deflate(self._h, a.ctypes.data_as(_u8p), a.size, off.ctypes.data_as(_u64p), n, block_bytes,
                                           out.ctypes.data_as(_u8p), cap, C.byref(got), perm.ctypes.data_as(_u32p), so.ctypes.data_as(_u64p),
                                           dup.ctypes.data_as(_u8p), counts.ctypes.data_as(_u64p)))
        self._stats()
        return out[: got.value].tobytes(), perm[:n], so, dup[:n], [int(x) for x in counts]

    def close(self) -> None:
        if self._h:
            lib().bmd_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
