"""ctypes binding of the MI355X BGZF block inflater (bmu_* in libbmf.so, C ABI in include/bmu.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _bmf_lib

BMU_OK, BMU_ERR_ARG, BMU_ERR_HIP, BMU_ERR_FORMAT, BMU_ERR_DATA = 0, 1, 2, 3, 4
(REASON_NONE, REASON_TRUNCATED, REASON_BLOCK_TYPE, REASON_STORED_LEN, REASON_CODE, REASON_DISTANCE, REASON_TOO_LONG,
 REASON_TOO_SHORT, REASON_CRC) = range(9)


class BmuError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bmu error {code}: {msg}")
        self.code = code


_u8p, _u32p, _u64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64))

SYMBOLS = {
    "bmu_last_error": (C.c_char_p, []),
    "bmu_layout": (C.c_int, [_u8p, C.c_uint64, _u64p, _u64p, _u64p, _u64p]),
    "bmu_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "bmu_destroy": (None, [C.c_void_p]),
    "bmu_inflate": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u8p, C.c_uint64, _u64p]),
    "bmu_bad_block": (C.c_int, [C.c_void_p, _u64p, _u32p]),
    "bmu_last_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), _u64p, _u64p, _u64p]),
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
    if rc != BMU_OK:
        raise BmuError(rc, lib().bmu_last_error().decode(errors="replace"))


def _array(data) -> np.ndarray:
    return np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)


def layout(data):
    """(in_offset, out_offset): the n_blocks + 1 starts of the BGZF blocks of `data` in the file and in the text.  Host
    only; BmuError(BMU_ERR_FORMAT) for anything that is not BGZF."""
    a = _array(data)
    n, total = C.c_uint64(0), C.c_uint64(0)
    _check(lib().bmu_layout(a.ctypes.data_as(_u8p), a.size, None, None, C.byref(n), C.byref(total)))
    in_off, out_off = np.zeros(n.value + 1, np.uint64), np.zeros(n.value + 1, np.uint64)
    _check(lib().bmu_layout(a.ctypes.data_as(_u8p), a.size, in_off.ctypes.data_as(_u64p), out_off.ctypes.data_as(_u64p), C.byref(n),
                            C.byref(total)))
    return [int(x) for x in in_off], [int(x) for x in out_off]


class Inflater:
    """One bmu_ctx.  inflate() returns the text; ms_kernels and n_stored / n_fixed / n_dynamic (DEFLATE blocks by type) are
    those of the last call."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().bmu_create(device, C.byref(self._h)))
        self.ms_kernels = 0.0
        self.n_stored = self.n_fixed = self.n_dynamic = 0

    def _stats(self) -> None:
        ms, f = C.c_float(0), [C.c_uint64(0) for _ in range(3)]
        _check(lib().bmu_last_stats(self._h, C.byref(ms), *[C.byref(x) for x in f]))
        self.ms_kernels = float(ms.value)
        self.n_stored, self.n_fixed, self.n_dynamic = (int(x.value) for x in f)

    def inflate(self, data, out_cap: int | None = None) -> bytes:
        a = _array(data)
        if out_cap is None:
            n, total = C.c_uint64(0), C.c_uint64(0)
            _check(lib().bmu_layout(a.ctypes.data_as(_u8p), a.size, None, None, C.byref(n), C.byref(total)))
            out_cap = int(total.value)
        out = np.empty(max(out_cap, 1), np.uint8)
        got = C.c_uint64(0)
        rc = lib().bmu_inflate(self._h, a.ctypes.data_as(_u8p), a.size, out.ctypes.data_as(_u8p), out_cap, C.byref(got))
        self._stats()
        _check(rc)
        return out[: got.value].tobytes()

    def bad_block(self):
        """(block, reason) of the first bad block of the last inflate(), or None."""
        b, r = C.c_uint64(0), C.c_uint32(0)
        _check(lib().bmu_bad_block(self._h, C.byref(b), C.byref(r)))
        return None if r.value == 0 else (int(b.value), int(r.value))

    def close(self) -> None:
        if self._h:
            lib().bmu_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
