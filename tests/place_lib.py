"""ctypes loader for tests/place/libplace_oracle.so — the sequential checker of place retrieval.  Tests only."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from bev_amd import PLACE_HIT_DTYPE, POINT_DTYPE, PlaceParams, place_params

DIR = Path(__file__).resolve().parent / "place"
SO = DIR / "libplace_oracle.so"
HANDLE_BYTES = 2112
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
        vp, i32 = C.c_void_p, C.c_int
        l.place_accumulate.argtypes = [vp, C.c_uint32, vp, C.POINTER(PlaceParams), C.c_float, vp]
        l.place_accumulate.restype = None
        l.place_handle.argtypes = [vp, i32, i32, vp]
        l.place_handle.restype = None
        l.place_pair_shifts.argtypes = [vp, vp, i32, i32, vp, vp]
        l.place_pair_shifts.restype = None
        l.place_match.argtypes = [vp, i32, vp, i32, vp, i32, i32, i32, vp]
        l.place_match.restype = None
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def descriptor(entries, params: PlaceParams | None = None, lidar_to_ground: float = 2.0) -> np.ndarray:
    """The (n_rings, n_sectors) uint8 descriptor of a list of (cloud, pose) entries: POINT_DTYPE clouds, each under its
    row-major 3 x 4 matrix (None: the raw coordinates).  An empty list gives the all-zero descriptor."""
    prm = params if params is not None else place_params()
    desc = np.zeros((prm.n_rings, prm.n_sectors), np.uint8)
    for cloud, pose in entries:
        cloud = np.ascontiguousarray(cloud, dtype=POINT_DTYPE)
        m = None if pose is None else np.ascontiguousarray(pose, dtype=np.float32).reshape(12)
        lib().place_accumulate(_p(cloud), len(cloud), _p(m), C.byref(prm), lidar_to_ground, _p(desc))
    return desc


def handle(desc) -> np.ndarray:
    """The product's per-descriptor record (HANDLE_BYTES uint8) of a descriptor."""
    desc = np.ascontiguousarray(desc, np.uint8)
    out = np.zeros(HANDLE_BYTES, np.uint8)
    lib().place_handle(_p(desc), desc.shape[0], desc.shape[1], _p(out))
    return out


def pair_shifts(dq, dc):
    """(S, cnt) of every shift of a pair: two int32 arrays of n_sectors values."""
    dq, dc = np.ascontiguousarray(dq, np.uint8), np.ascontiguousarray(dc, np.uint8)
    assert dq.shape == dc.shape
    S, cnt = np.zeros(dq.shape[1], np.int32), np.zeros(dq.shape[1], np.int32)
    lib().place_pair_shifts(_p(dq), _p(dc), dq.shape[0], dq.shape[1], _p(S), _p(cnt))
    return S, cnt


def match(dq, ddb, top_k=1, limit=None) -> np.ndarray:
    """(n_queries, top_k) PLACE_HIT_DTYPE records of (n, n_rings, n_sectors) descriptors."""
    dq, ddb = np.ascontiguousarray(dq, np.uint8), np.ascontiguousarray(ddb, np.uint8)
    R, Cn = dq.shape[1:]
    assert ddb.shape[1:] == (R, Cn) or len(ddb) == 0
    lim = None if limit is None else np.ascontiguousarray(limit, np.int32)
    hits = np.zeros((len(dq), top_k), PLACE_HIT_DTYPE)
    lib().place_match(_p(dq), len(dq), _p(ddb), len(ddb), _p(lim), top_k, R, Cn, _p(hits))
    return hits
