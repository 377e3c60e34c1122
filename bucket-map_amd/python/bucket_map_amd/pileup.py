"""ctypes binding of the MI355X pileup counter (bmp_* in libbmf.so, C ABI and the rule in include/bmp.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _bmf_lib
from .bamsort import record_offsets

BMP_OK, BMP_ERR_ARG, BMP_ERR_HIP = 0, 1, 2
N_COUNTERS, N_STATS, SITE_WORDS = 8, 6, 12
COUNTERS = ("A", "C", "G", "T", "N", "del", "ins", "lowq")
STATS = ("n_reads", "n_low_mapq", "n_left_out", "n_bases", "n_lowq", "n_sites")
THRESHOLDS = ("min_mapq", "min_bq", "min_alt", "min_frac_ppm")
DEFAULTS = dict(min_mapq=0, min_bq=13, min_alt=2, min_frac_ppm=200000)   # the command line's
KIND_SNV, KIND_DEL, KIND_INS = 1, 2, 4


class BmpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bmp error {code}: {msg}")
        self.code = code


_u8p, _u32p, _u64p, _f32p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64, C.c_float))

SYMBOLS = {
    "bmp_last_error": (C.c_char_p, []),
    "bmp_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "bmp_destroy": (None, [C.c_void_p]),
    "bmp_begin": (C.c_int, [C.c_void_p, _u32p, C.c_uint32, C.POINTER(C.c_void_p), _u32p]),
    "bmp_add": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, C.c_uint64, _u8p]),
    "bmp_finish": (C.c_int, [C.c_void_p, _u64p, _u64p]),
    "bmp_sites": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, _u32p]),
    "bmp_counts_at": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _u32p]),
    "bmp_last_stats": (C.c_int, [C.c_void_p, _f32p, _f32p]),
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
    if rc != BMP_OK:
        raise BmpError(rc, lib().bmp_last_error().decode(errors="replace"))


def base_pointers(ref_bases):
    """(the arrays kept alive, a C array of one pointer per reference) for bmp_begin."""
    keep = [np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else np.ascontiguousarray(b, np.uint8) for b in ref_bases]
    ptrs = (C.c_void_p * max(len(keep), 1))(*[a.ctypes.data if a.size else None for a in keep])
    return keep, ptrs


class Pileup:
    """One bmp_ctx.  begin(ref_len, ref_bases, **thresholds), add(stream, rec_offset, skip) any number of times, finish() ->
    (n_sites, stats: an (n_ref, 6) uint64 array in the order of STATS); then sites(first, count) -> a (count, 12) uint32 array of
    (reference, position, allele, the eight counters, kind) and counts_at(ref, start, count) -> a (count, 8) uint32 array in
    the order of COUNTERS.  pile(...) is all of that in one call.  After a call ms_add / ms_finish hold bmp_last_stats."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().bmp_create(device, C.byref(self._h)))
        self.ms_add = self.ms_finish = 0.0
        self.n_ref = 0
        self.n_sites = 0

    def _stats(self) -> None:
        ms = [C.c_float(0) for _ in range(2)]
        _check(lib().bmp_last_stats(self._h, *[C.byref(x) for x in ms]))
        self.ms_add, self.ms_finish = (float(x.value) for x in ms)

    def begin(self, ref_len, ref_bases, **thresholds) -> None:
        lens = np.ascontiguousarray(ref_len, np.uint32)
        assert len(ref_bases) == lens.size and all(len(b) == n for b, n in zip(ref_bases, lens.tolist()))
        th = np.array([{**DEFAULTS, **thresholds}[k] for k in THRESHOLDS], np.uint32)
        keep, ptrs = base_pointers(ref_bases)
        _check(lib().bmp_begin(self._h, lens.ctypes.data_as(_u32p), lens.size, ptrs, th.ctypes.data_as(_u32p)))
        del keep                                         # bmp_begin has uploaded the bases
        self.n_ref, self.n_sites = int(lens.size), 0

    def add(self, stream, rec_offset=None, skip=None) -> None:
        a = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else np.ascontiguousarray(stream, np.uint8)
        off = record_offsets(a.tobytes()) if rec_offset is None else np.ascontiguousarray(rec_offset, np.uint64)
        n = max(off.size - 1, 0)
        mask = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        assert mask is None or mask.size == n
        _check(lib().bmp_add(self._h, a.ctypes.data_as(_u8p), a.size, off.ctypes.data_as(_u64p), n,
                             None if mask is None or n == 0 else mask.ctypes.data_as(_u8p)))
        self._stats()

    def finish(self):
        n_sites, stats = C.c_uint64(0), np.zeros((max(self.n_ref, 1), N_STATS), np.uint64)
        _check(lib().bmp_finish(self._h, C.byref(n_sites), stats.ctypes.data_as(_u64p)))
        self.n_sites = int(n_sites.value)
        self._stats()
        return self.n_sites, stats[: self.n_ref]

    def sites(self, first: int = 0, count: int | None = None):
        count = self.n_sites - first if count is None else count
        out = np.zeros((max(count, 1), SITE_WORDS), np.uint32)
        _check(lib().bmp_sites(self._h, first, count, out.ctypes.data_as(_u32p)))
        return out[:count]

    def counts_at(self, ref: int, start: int, count: int):
        out = np.zeros((max(count, 1), N_COUNTERS), np.uint32)
        _check(lib().bmp_counts_at(self._h, ref, start, count, out.ctypes.data_as(_u32p)))
        return out[:count]

    def pile(self, ref_len, ref_bases, stream, rec_offset=None, skip=None, **thresholds):
        """(sites, stats) of one stream on the references."""
        self.begin(ref_len, ref_bases, **thresholds)
        self.add(stream, rec_offset, skip)
        _, stats = self.finish()
        return self.sites(), stats

    def close(self) -> None:
        if self._h:
            lib().bmp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
