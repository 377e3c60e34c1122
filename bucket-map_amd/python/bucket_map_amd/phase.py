"""ctypes binding of the MI355X read-backed phaser of het SNV calls (bmk_* in libbmf.so, C ABI and the rule in
include/bmk.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _bmf_lib
from .bamsort import record_offsets

BMK_OK, BMK_ERR_ARG, BMK_ERR_HIP = 0, 1, 2
CALL_WORDS, OUT_WORDS, N_STATS, MAX_REACH = 24, 8, 4, 8
PHASED, ROOT = 1, 2
PARAMS = ("min_mapq", "min_bq", "min_links", "min_frac_ppm", "reach")
DEFAULTS = dict(min_mapq=0, min_bq=13, min_links=2, min_frac_ppm=800000, reach=4)   # the command line's
# the words of a site
W_CALL, W_ROOT, W_ROOT_POS, W_HAP, W_FLAGS, W_D, W_CIS, W_TRANS = range(8)


class BmkError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bmk error {code}: {msg}")
        self.code = code


_u8p, _u32p, _u64p, _f32p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64, C.c_float))

SYMBOLS = {
    "bmk_last_error": (C.c_char_p, []),
    "bmk_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "bmk_destroy": (None, [C.c_void_p]),
    "bmk_begin": (C.c_int, [C.c_void_p, _u32p, C.c_uint32, _u32p, _u32p, C.c_uint64, _u64p]),
    "bmk_add": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, C.c_uint64, _u8p]),
    "bmk_finish": (C.c_int, [C.c_void_p, _u64p]),
    "bmk_phase": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, _u32p]),
    "bmk_links": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, _u32p]),
    "bmk_last_stats": (C.c_int, [C.c_void_p, _f32p, _f32p]),
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
    if rc != BMK_OK:
        raise BmkError(rc, lib().bmk_last_error().decode(errors="replace"))


class Phase:
    """One bmk_ctx.  begin(ref_len, calls, **params) -> H for an (n_calls, 24) array of calls as Genotype.call returns them;
    then add(stream, rec_offset, skip) any number of times; finish() -> the four sums; then phase(first, count) -> a (count, 8)
    uint32 array and links(first, count) -> a (count, reach, 4) uint32 array (links works before finish too).  After a call
    ms_add / ms_finish hold bmk_last_stats."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().bmk_create(device, C.byref(self._h)))
        self.ms_add = self.ms_finish = 0.0
        self.n_sites = 0
        self.reach = DEFAULTS["reach"]

    def _stats(self) -> None:
        ms = [C.c_float(0) for _ in range(2)]
        _check(lib().bmk_last_stats(self._h, *[C.byref(x) for x in ms]))
        self.ms_add, self.ms_finish = (float(x.value) for x in ms)

    def begin(self, ref_len, calls, **params) -> int:
        lens = np.ascontiguousarray(ref_len, np.uint32)
        pr = np.array([{**DEFAULTS, **params}[k] for k in PARAMS], np.uint32)
        s = np.ascontiguousarray(calls, np.uint32).reshape(-1, CALL_WORDS)
        n = C.c_uint64(0)
        _check(lib().bmk_begin(self._h, lens.ctypes.data_as(_u32p), lens.size, pr.ctypes.data_as(_u32p), s.ctypes.data_as(_u32p) if s.shape[0] else None,
                               s.shape[0], C.byref(n)))
        self.n_sites, self.reach = int(n.value), int(pr[4])
        self._stats()
        return self.n_sites

    def add(self, stream, rec_offset=None, skip=None) -> None:
        a = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else np.ascontiguousarray(stream, np.uint8)
        off = record_offsets(a.tobytes()) if rec_offset is None else np.ascontiguousarray(rec_offset, np.uint64)
        n = max(off.size - 1, 0)
        mask = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        assert mask is None or mask.size == n
        _check(lib().bmk_add(self._h, a.ctypes.data_as(_u8p), a.size, off.ctypes.data_as(_u64p), n,
                             None if mask is None or n == 0 else mask.ctypes.data_as(_u8p)))
        self._stats()

    def finish(self):
        stats = np.zeros(N_STATS, np.uint64)
        _check(lib().bmk_finish(self._h, stats.ctypes.data_as(_u64p)))
        self._stats()
        return stats

    def phase(self, first: int = 0, count=None):
        count = self.n_sites - first if count is None else count
        out = np.zeros((max(count, 1), OUT_WORDS), np.uint32)
        _check(lib().bmk_phase(self._h, first, count, out.ctypes.data_as(_u32p)))
        return out[:count]

    def links(self, first: int = 0, count=None):
        count = self.n_sites - first if count is None else count
        out = np.zeros((max(count, 1), self.reach, 4), np.uint32)
        _check(lib().bmk_links(self._h, first, count, out.ctypes.data_as(_u32p)))
        return out[:count]

    def close(self) -> None:
        if self._h:
            lib().bmk_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
