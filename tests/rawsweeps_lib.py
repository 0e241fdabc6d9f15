"""ctypes loader for tests/rawsweeps/librawsweeps.so — C entry points over host/RawSweeps.cpp, the raw-sweep readers of
batch_multi_bev_gen.  Tests only."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

DIR = Path(__file__).resolve().parent / "rawsweeps"
SO = DIR / "librawsweeps.so"
MULRAN, OXFORD, KITTI = 0, 1, 2
CAP = {MULRAN: 64 * 1024, KITTI: 64 * 2083}   # MulranPointCloudSelect.cpp:113, KittiPointCloudSelect.cpp:174
_lib = None


def build() -> None:
    r = subprocess.run(["make", "-C", str(DIR)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"make -C {DIR} failed:\n{r.stdout}")


def lib():
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(str(SO))
        l.rs_parse_format.argtypes = [C.c_char_p]
        l.rs_fits_sensor.argtypes = [C.c_int, C.c_int]
        l.rs_returns.argtypes = [C.c_int, C.c_ulonglong]
        l.rs_returns.restype = C.c_ulonglong
        l.rs_read.argtypes = [C.c_int, C.c_char_p, C.c_void_p, C.c_ulonglong]
        l.rs_read.restype = C.c_longlong
        l.rs_list.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_ulonglong]
        _lib = l
    return _lib


def read(fmt: int, path) -> np.ndarray | None:
    """the floats readRawSweep gives for the file; None: unreadable"""
    cap = 4 * 200000
    out = np.full(cap, np.float32(-777.0), dtype=np.float32)
    n = lib().rs_read(fmt, str(path).encode(), out.ctypes.data, cap)
    if n == -1:
        return None
    assert n >= 0
    return out[:n].copy()


def expected(fmt: int, data: bytes) -> np.ndarray:
    """what the reader is defined to give (RawSweeps.h), in numpy: whole 16-byte records, the first cap of them"""
    n = len(data) // 16
    n = min(n, CAP[fmt]) if fmt in CAP else n
    return np.frombuffer(data[:16 * n], dtype="<f4").copy()


def listing(directory, ext: str) -> list[str]:
    buf = C.create_string_buffer(1 << 16)
    n = lib().rs_list(str(directory).encode(), ext.encode(), buf, len(buf))
    assert n >= 0
    names = buf.value.decode().splitlines()
    assert len(names) == n
    return names
