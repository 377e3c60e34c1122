"""ctypes binding of the MI355X coverage counter (bmc_* in libbmf.so, C ABI and the rule in include/bmc.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _bmf_lib
from .bamsort import record_offsets

BMC_OK, BMC_ERR_ARG, BMC_ERR_HIP = 0, 1, 2
N_STATS = 7
STATS = ("n_reads", "cov_bases", "sum_depth", "sum_mapq", "sum_qual", "n_qual", "n_long")


class BmcError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bmc error {code}: {msg}")
        self.code = code


_u8p, _u32p, _u64p, _f32p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64, C.c_float))

SYMBOLS = {
    "bmc_last_error": (C.c_char_p, []),
    "bmc_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "bmc_destroy": (None, [C.c_void_p]),
    "bmc_begin": (C.c_int, [C.c_void_p, _u32p, C.c_uint32]),
    "bmc_add": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, C.c_uint64, _u8p]),
    "bmc_finish": (C.c_int, [C.c_void_p, _u64p, _u64p]),
    "bmc_runs": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, _u32p]),
    "bmc_depth_at": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _u32p]),
    "bmc_last_stats": (C.c_int, [C.c_void_p, _f32p, _f32p]),
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
    if rc != BMC_OK:
        raise BmcError(rc, lib().bmc_last_error().decode(errors="replace"))


class Depth:
    """One bmc_ctx.  begin(ref_len), add(stream, rec_offset, skip) any number of times, finish() -> (n_runs, stats: an
    (n_ref, 7) uint64 array in the order of STATS); then runs(first, count) -> an (count, 4) uint32 array of (reference, start,
    end, depth) and depth_at(ref, start, count) -> uint32 depths.  count(...) is all of that in one call.  After a call
    ms_add / ms_finish hold bmc_last_stats."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().bmc_create(device, C.byref(self._h)))
        self.ms_add = self.ms_finish = 0.0
        self.n_ref = 0
        self.n_runs = 0

    def _stats(self) -> None:
        ms = [C.c_float(0) for _ in range(2)]
        _check(lib().bmc_last_stats(self._h, *[C.byref(x) for x in ms]))
        self.ms_add, self.ms_finish = (float(x.value) for x in ms)

    def begin(self, ref_len) -> None:
        lens = np.ascontiguousarray(ref_len, np.uint32)
        _check(lib().bmc_begin(self._h, lens.ctypes.data_as(_u32p), lens.size))
        self.n_ref, self.n_runs = int(lens.size), 0

    def add(self, stream, rec_offset=None, skip=None) -> None:
        a = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else np.ascontiguousarray(stream, np.uint8)
        off = record_offsets(a.tobytes()) if rec_offset is None else np.ascontiguousarray(rec_offset, np.uint64)
        n = max(off.size - 1, 0)
        mask = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        assert mask is None or mask.size == n
        _check(lib().bmc_add(self._h, a.ctypes.data_as(_u8p), a.size, off.ctypes.data_as(_u64p), n,
                             None if mask is None or n == 0 else mask.ctypes.data_as(_u8p)))
        self._stats()

    def finish(self):
        n_runs, stats = C.c_uint64(0), np.zeros((max(self.n_ref, 1), N_STATS), np.uint64)
        _check(lib().bmc_finish(self._h, C.byref(n_runs), stats.ctypes.data_as(_u64p)))
        self.n_runs = int(n_runs.value)
        self._stats()
        return self.n_runs, stats[: self.n_ref]

    def runs(self, first: int = 0, count: int | None = None):
        count = self.n_runs - first if count is None else count
        out = np.zeros((max(count, 1), 4), np.uint32)
        _check(lib().bmc_runs(self._h, first, count, out.ctypes.data_as(_u32p)))
        return out[:count]

    def depth_at(self, ref: int, start: int, count: int):
        out = np.zeros(max(count, 1), np.uint32)
        _check(lib().bmc_depth_at(self._h, ref, start, count, out.ctypes.data_as(_u32p)))
        return out[:count]

    def count(self, ref_len, stream, rec_offset=None, skip=None):
        """(runs, stats) of one stream on the references."""
        self.begin(ref_len)
        self.add(stream, rec_offset, skip)
        _, stats = self.finish()
        return self.runs(), stats

    def close(self) -> None:
        if self._h:
            lib().bmc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
