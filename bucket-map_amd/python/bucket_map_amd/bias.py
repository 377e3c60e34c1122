"""ctypes binding of the MI355X strand-bias and mapping-quality annotator (bmb_* in libbmf.so, C ABI and the rule in
include/bmb.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _bmf_lib
from .bamsort import record_offsets

BMB_OK, BMB_ERR_ARG, BMB_ERR_HIP = 0, 1, 2
N_STRAND_CELLS, CALL_WORDS, OUT_WORDS = 4, 24, 16
N_LF, N_E, FS_CAP, FS_MAX_N = 65536, 12001, 6000, 65535
ANNOTATED, NO_FS = 1, 2
PARAMS = ("min_mapq", "min_bq")
DEFAULTS = dict(min_mapq=0, min_bq=13)   # the command line's
# the words of an annotation
W_FWD, W_REV, W_MQ, W_FS, W_FLAGS, W_N, W_TABLE = 0, 4, 8, 9, 10, 11, 12


class BmbError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bmb error {code}: {msg}")
        self.code = code


_u8p, _u32p, _u64p, _f32p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64, C.c_float))

SYMBOLS = {
    "bmb_last_error": (C.c_char_p, []),
    "bmb_tables": (C.c_int, [_u32p, _u64p]),
    "bmb_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "bmb_destroy": (None, [C.c_void_p]),
    "bmb_begin": (C.c_int, [C.c_void_p, _u32p, C.c_uint32, _u32p]),
    "bmb_add": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, C.c_uint64, _u8p]),
    "bmb_annotate": (C.c_int, [C.c_void_p, _u32p, C.c_uint64, _u32p]),
    "bmb_cells_at": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _u64p, _u64p]),
    "bmb_last_stats": (C.c_int, [C.c_void_p, _f32p, _f32p]),
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
    if rc != BMB_OK:
        raise BmbError(rc, lib().bmb_last_error().decode(errors="replace"))


def tables():
    """(LF, E) as bmb_tables makes them on the host: a (65536,) uint32 and a (12001,) uint64 array.  Needs no device."""
    lf, e = np.zeros(N_LF, np.uint32), np.zeros(N_E, np.uint64)
    _check(lib().bmb_tables(lf.ctypes.data_as(_u32p), e.ctypes.data_as(_u64p)))
    return lf, e


class Bias:
    """One bmb_ctx.  begin(ref_len, **params), then in any order and any number of times add(stream, rec_offset, skip),
    annotate(calls) -> an (n_calls, 16) uint32 array for an (n_calls, 24) array of calls as Genotype.call returns them, and
    cells_at(ref, start, count) -> a (count, 4) uint64 array of fwd << 32 | rev for A C G T and a (count,) uint64 array of
    n << 40 | S.  After a call ms_add / ms_annotate hold bmb_last_stats."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().bmb_create(device, C.byref(self._h)))
        self.ms_add = self.ms_annotate = 0.0
        self.n_ref = 0

    def _stats(self) -> None:
        ms = [C.c_float(0) for _ in range(2)]
        _check(lib().bmb_last_stats(self._h, *[C.byref(x) for x in ms]))
        self.ms_add, self.ms_annotate = (float(x.value) for x in ms)

    def begin(self, ref_len, **params) -> None:
        lens = np.ascontiguousarray(ref_len, np.uint32)
        pr = np.array([{**DEFAULTS, **params}[k] for k in PARAMS], np.uint32)
        _check(lib().bmb_begin(self._h, lens.ctypes.data_as(_u32p), lens.size, pr.ctypes.data_as(_u32p)))
        self.n_ref = int(lens.size)
        self._stats()

    def add(self, stream, rec_offset=None, skip=None) -> None:
        a = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else np.ascontiguousarray(stream, np.uint8)
        off = record_offsets(a.tobytes()) if rec_offset is None else np.ascontiguousarray(rec_offset, np.uint64)
        n = max(off.size - 1, 0)
        mask = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        assert mask is None or mask.size == n
        _check(lib().bmb_add(self._h, a.ctypes.data_as(_u8p), a.size, off.ctypes.data_as(_u64p), n,
                             None if mask is None or n == 0 else mask.ctypes.data_as(_u8p)))
        self._stats()

    def annotate(self, calls):
        s = np.ascontiguousarray(calls, np.uint32).reshape(-1, CALL_WORDS)
        n = s.shape[0]
        out = np.zeros((max(n, 1), OUT_WORDS), np.uint32)
        _check(lib().bmb_annotate(self._h, s.ctypes.data_as(_u32p) if n else None, n, out.ctypes.data_as(_u32p)))
        self._stats()
        return out[:n]

    def cells_at(self, ref: int, start: int, count: int):
        strand, mapq = np.zeros((max(count, 1), N_STRAND_CELLS), np.uint64), np.zeros(max(count, 1), np.uint64)
        _check(lib().bmb_cells_at(self._h, ref, start, count, strand.ctypes.data_as(_u64p), mapq.ctypes.data_as(_u64p)))
        return strand[:count], mapq[:count]

    def close(self) -> None:
        if self._h:
            lib().bmb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
