"""ctypes binding of the MI355X indel caller (bmn_* in libbmf.so, C ABI and the rule in include/bmn.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _bmf_lib
from .bamsort import record_offsets

BMN_OK, BMN_ERR_ARG, BMN_ERR_HIP = 0, 1, 2
EVENT_WORDS, ALLELE_WORDS, CALL_WORDS, N_STATS, MAX_INS = 4, 8, 16, 3, 32
GENOTYPED, VARIANT = 1, 2
INS, OTHER, LEN_MASK = 1 << 31, 1 << 30, (1 << 28) - 1
PARAMS = ("min_mapq", "min_alt", "min_frac_ppm", "q_indel", "prior")
DEFAULTS = dict(min_mapq=0, min_alt=2, min_frac_ppm=200000, q_indel=30, prior=4000)   # the command line's
STATS = ("n_reads", "n_low_mapq", "n_left_out")
# the words of a call
W_REF, W_ANCHOR, W_W1, W_SEQ, W_FLAGS, W_COPIES, W_GQ, W_QUAL, W_NREF, W_NALT, W_NOTH, W_DP, W_PL = 0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13


class BmnError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bmn error {code}: {msg}")
        self.code = code


_u8p, _u32p, _u64p, _f32p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64, C.c_float))

SYMBOLS = {
    "bmn_last_error": (C.c_char_p, []),
    "bmn_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "bmn_destroy": (None, [C.c_void_p]),
    "bmn_begin": (C.c_int, [C.c_void_p, _u32p, C.c_uint32, _u32p]),
    "bmn_add": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, C.c_uint64, _u8p]),
    "bmn_finish": (C.c_int, [C.c_void_p, _u64p, _u64p, _u64p, _u64p]),
    "bmn_alleles": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, _u32p]),
    "bmn_calls": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, _u32p]),
    "bmn_events_of": (C.c_int, [C.c_void_p, C.c_uint64, _u64p, _u64p, _u32p]),
    "bmn_cover_at": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _u32p]),
    "bmn_last_stats": (C.c_int, [C.c_void_p, _f32p, _f32p]),
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
    if rc != BMN_OK:
        raise BmnError(rc, lib().bmn_last_error().decode(errors="replace"))


class Indel:
    """One bmn_ctx.  begin(ref_len, **params), any number of add(stream, rec_offset, skip), finish() -> the per-reference sums
    as an (n_ref, 3) uint64 array, then alleles() -> (n_alleles, 8), calls() -> (n_calls, 16) and cover_at(ref, start, count)
    -> uint32 arrays.  events_of(add) -> the (n, 4) unsorted events of one add; n_adds() counts the adds.  After a call
    ms_add / ms_finish hold bmn_last_stats."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().bmn_create(device, C.byref(self._h)))
        self.ms_add = self.ms_finish = 0.0
        self.n_ref = self.n_events = self.n_alleles = self.n_calls = 0

    def _stats(self) -> None:
        ms = [C.c_float(0) for _ in range(2)]
        _check(lib().bmn_last_stats(self._h, *[C.byref(x) for x in ms]))
        self.ms_add, self.ms_finish = (float(x.value) for x in ms)

    def begin(self, ref_len, **params) -> None:
        lens = np.ascontiguousarray(ref_len, np.uint32)
        pr = np.array([{**DEFAULTS, **params}[k] for k in PARAMS], np.uint32)
        _check(lib().bmn_begin(self._h, lens.ctypes.data_as(_u32p), lens.size, pr.ctypes.data_as(_u32p)))
        self.n_ref = int(lens.size)
        self.n_events = self.n_alleles = self.n_calls = 0
        self._stats()

    def add(self, stream, rec_offset=None, skip=None) -> None:
        a = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else np.ascontiguousarray(stream, np.uint8)
        off = record_offsets(a.tobytes()) if rec_offset is None else np.ascontiguousarray(rec_offset, np.uint64)
        n = max(off.size - 1, 0)
        mask = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        assert mask is None or mask.size == n
        _check(lib().bmn_add(self._h, a.ctypes.data_as(_u8p), a.size, off.ctypes.data_as(_u64p), n,
                             None if mask is None or n == 0 else mask.ctypes.data_as(_u8p)))
        self._stats()

    def finish(self):
        counts = [C.c_uint64(0) for _ in range(3)]
        stats = np.zeros((max(self.n_ref, 1), N_STATS), np.uint64)
        _check(lib().bmn_finish(self._h, *[C.byref(x) for x in counts], stats.ctypes.data_as(_u64p)))
        self.n_events, self.n_alleles, self.n_calls = (int(x.value) for x in counts)
        self._stats()
        return stats[: self.n_ref]

    def _list(self, fn, total, words, first, count):
        count = total - first if count is None else count
        out = np.zeros((max(count, 1), words), np.uint32)
        _check(fn(self._h, first, count, out.ctypes.data_as(_u32p)))
        return out[:count]

    def alleles(self, first: int = 0, count=None):
        return self._list(lib().bmn_alleles, self.n_alleles, ALLELE_WORDS, first, count)

    def calls(self, first: int = 0, count=None):
        return self._list(lib().bmn_calls, self.n_calls, CALL_WORDS, first, count)

    def n_adds(self) -> int:
        n = C.c_uint64(0)
        _check(lib().bmn_events_of(self._h, 0, C.byref(n), None, None))
        return int(n.value)

    def events_of(self, add: int):
        n_adds, n = C.c_uint64(0), C.c_uint64(0)
        _check(lib().bmn_events_of(self._h, add, C.byref(n_adds), C.byref(n), None))
        out = np.zeros((max(int(n.value), 1), EVENT_WORDS), np.uint32)
        _check(lib().bmn_events_of(self._h, add, C.byref(n_adds), C.byref(n), out.ctypes.data_as(_u32p)))
        return out[: int(n.value)]

    def cover_at(self, ref: int, start: int, count: int):
        out = np.zeros(max(count, 1), np.uint32)
        _check(lib().bmn_cover_at(self._h, ref, start, count, out.ctypes.data_as(_u32p)))
        return out[:count]

    def close(self) -> None:
        if self._h:
            lib().bmn_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
