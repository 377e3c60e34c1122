"""ctypes binding of the MI355X mapping statistics of a BAM record stream (bmq_* in libbmf.so, C ABI and the rule in
include/bmq.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _bmf_lib
from .bamsort import record_offsets

BMQ_OK, BMQ_ERR_ARG, BMQ_ERR_HIP = 0, 1, 2
N_TALLIES, N_TABLES, MAX_LDS_CYCLES = 35, 8, 512
PARAMS = ("max_cycle", "max_insert")
DEFAULTS = dict(max_cycle=1024, max_insert=8000)   # the command line's
TABLES = ("MAPQ", "RL", "IS", "GC", "ID", "BC", "QC", "MC")   # BMQ_T_* in order
WIDTH = (1, 1, 3, 1, 2, 5, 64, 6)


class BmqError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bmq error {code}: {msg}")
        self.code = code


_u8p, _u32p, _u64p, _f32p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64, C.c_float))

SYMBOLS = {
    "bmq_last_error": (C.c_char_p, []),
    "bmq_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "bmq_destroy": (None, [C.c_void_p]),
    "bmq_begin": (C.c_int, [C.c_void_p, _u32p]),
    "bmq_add": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, C.c_uint64, _u8p]),
    "bmq_finish": (C.c_int, [C.c_void_p, _u64p]),
    "bmq_table": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, _u64p]),
    "bmq_last_stats": (C.c_int, [C.c_void_p, _f32p, _f32p]),
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
    if rc != BMQ_OK:
        raise BmqError(rc, lib().bmq_last_error().decode(errors="replace"))


def table_rows(which: int, max_cycle: int, max_insert: int) -> int:
    return (256, max_cycle + 1, max_insert + 1, 101, 256, max_cycle, max_cycle, max_cycle)[which]


class Stats:
    """One bmq_ctx.  begin(**params); then add(stream, rec_offset, skip) any number of times; finish() -> the 35 tallies; then
    table(which, first, count) -> a (count, width) uint64 array of rows of table `which` (an index or a name of TABLES).  After
    a call ms_add / ms_finish hold bmq_last_stats.  BMQ_LDS_CYCLES in the environment is read when the context is made."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().bmq_create(device, C.byref(self._h)))
        self.ms_add = self.ms_finish = 0.0
        self.max_cycle, self.max_insert = DEFAULTS["max_cycle"], DEFAULTS["max_insert"]

    def _stats(self) -> None:
        ms = [C.c_float(0) for _ in range(2)]
        _check(lib().bmq_last_stats(self._h, *[C.byref(x) for x in ms]))
        self.ms_add, self.ms_finish = (float(x.value) for x in ms)

    def begin(self, **params) -> None:
        pr = np.array([{**DEFAULTS, **params}[k] for k in PARAMS], np.uint32)
        _check(lib().bmq_begin(self._h, pr.ctypes.data_as(_u32p)))
        self.max_cycle, self.max_insert = int(pr[0]), int(pr[1])
        self._stats()

    def add(self, stream, rec_offset=None, skip=None) -> None:
        a = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else np.ascontiguousarray(stream, np.uint8)
        off = record_offsets(a.tobytes()) if rec_offset is None else np.ascontiguousarray(rec_offset, np.uint64)
        n = max(off.size - 1, 0)
        mask = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        assert mask is None or mask.size == n
        _check(lib().bmq_add(self._h, a.ctypes.data_as(_u8p), a.size, off.ctypes.data_as(_u64p), n,
                             None if mask is None or n == 0 else mask.ctypes.data_as(_u8p)))
        self._stats()

    def finish(self):
        tallies = np.zeros(N_TALLIES, np.uint64)
        _check(lib().bmq_finish(self._h, tallies.ctypes.data_as(_u64p)))
        self._stats()
        return tallies

    def table(self, which, first: int = 0, count=None):
        which = TABLES.index(which) if isinstance(which, str) else int(which)
        width = WIDTH[which] if 0 <= which < N_TABLES else 1
        if count is None:
            count = table_rows(which, self.max_cycle, self.max_insert) - first
        out = np.zeros((max(count, 1), width), np.uint64)
        _check(lib().bmq_table(self._h, which, first, count, out.ctypes.data_as(_u64p)))
        return out[:count]

    def close(self) -> None:
        if self._h:
            lib().bmq_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
