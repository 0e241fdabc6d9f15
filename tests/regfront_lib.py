"""ctypes loader for tests/regfront/libregfront_oracle.so — the sequential C checker of the registration front end
(top-part flatten, voxel grid, 2-D normals; DESIGN.md "Registration front end").  Tests only."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from bev_amd import POINT_DTYPE

DIR = Path(__file__).resolve().parent / "regfront"
SO = DIR / "libregfront_oracle.so"
_lib = None


def build() -> None:
    r = subprocess.run(["make", "-C", str(DIR)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"make -C {DIR} failed:\n{r.stdout}")


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(str(SO))
        vp, u32, f = C.c_void_p, C.c_uint32, C.c_float
        l.rf_top_part.argtypes = [vp, u32, vp]
        l.rf_top_part.restype = u32
        l.rf_max_out.argtypes = [C.c_uint64]
        l.rf_max_out.restype = u32
        l.rf_voxel.argtypes = [vp, u32, f, vp, vp]
        l.rf_voxel.restype = u32
        l.rf_normals.argtypes = [vp, u32, f, f, f, vp, vp]
        l.rf_normals.restype = None
        l.rf_chain.argtypes = [vp, u32, f, f, f, f, vp]
        l.rf_chain.restype = u32
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _xyz4(xyz):
    a = np.asarray(xyz, dtype=np.float32)
    if a.ndim == 2 and a.shape[1] == 3:
        a = np.concatenate([a, np.zeros((len(a), 1), np.float32)], axis=1)
    return np.ascontiguousarray(a.reshape(-1, 4))


def top_part(cloud):
    cloud = np.ascontiguousarray(cloud, dtype=POINT_DTYPE)
    out = np.zeros((lib().rf_max_out(len(cloud)), 4), np.float32)
    m = lib().rf_top_part(_p(cloud), len(cloud), _p(out))
    return out[:m].copy()


def voxel(xyz, leaf=0.2, want_info=False):
    xyz = _xyz4(xyz)
    out = np.zeros((max(len(xyz), 1), 4), np.float32)
    info = np.zeros(4, np.int64)
    m = lib().rf_voxel(_p(xyz), len(xyz), leaf, _p(out), _p(info))
    return (out[:m].copy(), info) if want_info else out[:m].copy()


def normals(xyz, radius=2.0, viewpoint=(0.0, 0.0, 0.0), want_nn=False):
    xyz = _xyz4(xyz)
    out = np.zeros((len(xyz), 8), np.float32)
    nn = np.zeros(max(len(xyz), 1), np.uint32)
    lib().rf_normals(_p(xyz), len(xyz), radius, viewpoint[0], viewpoint[1], _p(out), _p(nn))
    return (out, nn[: len(xyz)]) if want_nn else out


def chain(cloud, leaf=0.2, radius=2.0, viewpoint=(0.0, 0.0, 0.0)):
    cloud = np.ascontiguousarray(cloud, dtype=POINT_DTYPE)
    out = np.zeros((lib().rf_max_out(len(cloud)), 12), np.float32)
    m = lib().rf_chain(_p(cloud), len(cloud), leaf, radius, viewpoint[0], viewpoint[1], _p(out))
    return out[:m].copy()
