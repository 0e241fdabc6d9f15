"""ctypes loader for tests/verify/libverify_oracle.so — the sequential checker of the verification calls: the
moved query, a brute-force nearest neighbour in both directions, the counts.  Built on demand.  Tests only."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from bev_amd import POINT_DTYPE, VERIFY_RESULT_DTYPE, VerifyParams, verify_params

DIR = Path(__file__).resolve().parent / "verify"
SO = DIR / "libverify_oracle.so"
F32 = np.float32
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
        vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
        l.verify_oracle.argtypes = [vp, u32, sz, vp, u32, sz, vp, C.POINTER(VerifyParams), vp]
        l.verify_oracle.restype = None
        _lib = l
    return _lib


def _floats(cloud):
    """(contiguous float32 view, points, stride in floats) of POINT_DTYPE records or (n, 3) / (n, 4) rows"""
    a = np.asarray(cloud)
    if a.dtype == POINT_DTYPE:
        a = np.ascontiguousarray(a)
        return a.view(F32).reshape(-1), len(a), POINT_DTYPE.itemsize // 4
    a = np.ascontiguousarray(a, dtype=F32)
    a = a.reshape(-1, a.shape[-1] if a.ndim == 2 else 3)
    return a.reshape(-1), len(a), a.shape[1]


def oracle(src, tgt, T, params: VerifyParams | None = None) -> np.ndarray:
    """One VERIFY_RESULT_DTYPE record: src moved by rows 0 ... 2 of the 4 x 4 T against tgt, as the contract counts"""
    prm = params if params is not None else verify_params()
    s, ns, ss = _floats(src)
    t, nt, ts = _floats(tgt)
    t16 = np.ascontiguousarray(np.asarray(T, dtype=F32).reshape(16))
    out = np.zeros(1, VERIFY_RESULT_DTYPE)
    lib().verify_oracle(C.c_void_p(s.ctypes.data) if ns else None, ns, ss, C.c_void_p(t.ctypes.data) if nt else None, nt, ts,
                        C.c_void_p(t16.ctypes.data), C.byref(prm), C.c_void_p(out.ctypes.data))
    return out[0]


def points(xyz) -> np.ndarray:
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    out = np.zeros(len(xyz), POINT_DTYPE)
    out["x"], out["y"], out["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return out


def shift4(dx=0.0, dy=0.0, dz=0.0) -> np.ndarray:
    T = np.eye(4, dtype=F32)
    T[:3, 3] = [dx, dy, dz]
    return T


def lattice(n: int, seed: int, extent: int = 40 * 32) -> np.ndarray:
    """(n, 3) float32: distinct seeded points whose coordinates are multiples of 1 / 32 inside +-extent / 64 (z a tenth of it);
    every distance between them, and to copies moved by multiples of 1 / 32, is exact in float32"""
    rng = np.random.default_rng([int(seed), 0x7E1F])
    k = np.unique(np.c_[rng.integers(-extent // 2, extent // 2, (2 * n + 8, 2)), rng.integers(0, extent // 10, 2 * n + 8)], axis=0)
    k = k[rng.permutation(len(k))][:n]
    assert len(k) == n
    return (k / 32.0).astype(F32)
