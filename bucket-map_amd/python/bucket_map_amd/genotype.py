"""ctypes binding of the MI355X genotype caller (bmg_* in libbmf.so, C ABI and the rule in include/bmg.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _bmf_lib
from .bamsort import record_offsets

BMG_OK, BMG_ERR_ARG, BMG_ERR_HIP = 0, 1, 2
N_CELLS, N_GENOTYPES, SITE_WORDS, CALL_WORDS = 4, 10, 12, 24
GENOTYPED, VARIANT = 1, 2
GENOTYPES = ("AA", "AC", "CC", "AG", "CG", "GG", "AT", "CT", "GT", "TT")   # index b (b + 1) / 2 + a for the letters a <= b
PARAMS = ("min_mapq", "min_bq", "q_absent", "q_cap", "prior")
DEFAULTS = dict(min_mapq=0, min_bq=13, q_absent=30, q_cap=60, prior=3000)   # the command line's
# the words of a call
W_REF, W_POS, W_R, W_FLAGS, W_GT, W_GQ, W_QUAL, W_N, W_PL, W_DP = 0, 1, 2, 3, 4, 6, 7, 8, 12, 22


class BmgError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bmg error {code}: {msg}")
        self.code = code


_u8p, _u32p, _u64p, _f32p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64, C.c_float))

SYMBOLS = {
    "bmg_last_error": (C.c_char_p, []),
    "bmg_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "bmg_destroy": (None, [C.c_void_p]),
    "bmg_begin": (C.c_int, [C.c_void_p, _u32p, C.c_uint32, _u32p]),
    "bmg_add": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, C.c_uint64, _u8p]),
    "bmg_call": (C.c_int, [C.c_void_p, _u32p, C.c_uint64, _u32p]),
    "bmg_cells_at": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _u64p]),
    "bmg_last_stats": (C.c_int, [C.c_void_p, _f32p, _f32p]),
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
    if rc != BMG_OK:
        raise BmgError(rc, lib().bmg_last_error().decode(errors="replace"))


class Genotype:
    """One bmg_ctx.  begin(ref_len, **params), then in any order and any number of times add(stream, rec_offset, skip),
    call(sites) -> a (n_sites, 24) uint32 array for an (n_sites, 12) array of sites as Pileup.sites() returns them, and
    cells_at(ref, start, count) -> a (count, 4) uint64 array of n << 32 | Q for A C G T.  After a call ms_add / ms_call hold
    bmg_last_stats."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().bmg_create(device, C.byref(self._h)))
        self.ms_add = self.ms_call = 0.0
        self.n_ref = 0

    def _stats(self) -> None:
        ms = [C.c_float(0) for _ in range(2)]
        _check(lib().bmg_last_stats(self._h, *[C.byref(x) for x in ms]))
        self.ms_add, self.ms_call = (float(x.value) for x in ms)

    def begin(self, ref_len, **params) -> None:
        lens = np.ascontiguousarray(ref_len, np.uint32)
        pr = np.array([{**DEFAULTS, **params}[k] for k in PARAMS], np.uint32)
        _check(lib().bmg_begin(self._h, lens.ctypes.data_as(_u32p), lens.size, pr.ctypes.data_as(_u32p)))
        self.n_ref = int(lens.size)
        self._stats()

    def add(self, stream, rec_offset=None, skip=None) -> None:
        a = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else np.ascontiguousarray(stream, np.uint8)
        off = record_offsets(a.tobytes()) if rec_offset is None else np.ascontiguousarray(rec_offset, np.uint64)
        n = max(off.size - 1, 0)
        mask = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        assert mask is None or mask.size == n
        _check(lib().bmg_add(self._h, a.ctypes.data_as(_u8p), a.size, off.ctypes.data_as(_u64p), n,
                             None if mask is None or n == 0 else mask.ctypes.data_as(_u8p)))
        self._stats()

    def call(self, sites):
        s = np.ascontiguousarray(sites, np.uint32).reshape(-1, SITE_WORDS)
        n = s.shape[0]
        out = np.zeros((max(n, 1), CALL_WORDS), np.uint32)
        _check(lib().bmg_call(self._h, s.ctypes.data_as(_u32p) if n else None, n, out.ctypes.data_as(_u32p)))
        self._stats()
        return out[:n]

    def cells_at(self, ref: int, start: int, count: int):
        out = np.zeros((max(count, 1), N_CELLS), np.uint64)
        _check(lib().bmg_cells_at(self._h, ref, start, count, out.ctypes.data_as(_u64p)))
        return out[:count]

    def close(self) -> None:
        if self._h:
            lib().bmg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
