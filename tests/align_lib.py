"""ctypes loader for tests/align/libalign_oracle.so — the sequential checker of the translation guess of retrieved pairs
(DESIGN.md §6ab).  Tests only."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from bev_amd import ALIGN_DETAIL_DTYPE, ICP_RESULT_DTYPE, POINT_DTYPE, AlignParams, align_params

DIR = Path(__file__).resolve().parent / "align"
SO = DIR / "libalign_oracle.so"
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
        vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
        l.align_params_admitted.argtypes = [C.POINTER(AlignParams)]
        l.align_params_admitted.restype = i32
        l.align_accumulate.argtypes = [vp, C.c_uint32, vp, C.POINTER(AlignParams), f32, vp]
        l.align_accumulate.restype = None
        l.align_energy.argtypes = [vp, i32]
        l.align_energy.restype = C.c_uint32
        l.align_scores.argtypes = [vp, vp, i32, i32, vp]
        l.align_scores.restype = None
        l.align_guess.argtypes = [f32, i32, f32, i32, vp]
        l.align_guess.restype = None
        l.align_hit.argtypes = [vp, C.c_uint32, vp, C.POINTER(AlignParams), f32, f32, vp, vp, vp, vp, vp]
        l.align_hit.restype = None
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def admitted(prm: AlignParams) -> bool:
    return bool(lib().align_params_admitted(C.byref(prm)))


def grid(entries, params: AlignParams | None = None, lidar_to_ground: float = 2.0) -> np.ndarray:
    """The (G, G) uint8 height grid of a list of (cloud, pose) entries: POINT_DTYPE clouds, each under its row-major 3 x 4
    matrix (None: the raw coordinates).  An empty list gives the all-zero grid."""
    prm = params if params is not None else align_params()
    out = np.zeros((prm.grid, prm.grid), np.uint8)
    for cloud, pose in entries:
        cloud = np.ascontiguousarray(cloud, dtype=POINT_DTYPE)
        m = None if pose is None else np.ascontiguousarray(np.asarray(pose, np.float32).reshape(-1)[:12])
        lib().align_accumulate(_p(cloud), len(cloud), _p(m), C.byref(prm), lidar_to_ground, _p(out))
    return out


def energy(g) -> int:
    g = np.ascontiguousarray(g, np.uint8)
    return int(lib().align_energy(_p(g), g.shape[0]))


def scores(q, c, S) -> np.ndarray:
    """(2S + 1, 2S + 1) uint32: [dy + S, dx + S]"""
    q, c = np.ascontiguousarray(q, np.uint8), np.ascontiguousarray(c, np.uint8)
    assert q.shape == c.shape and q.shape[0] == q.shape[1]
    out = np.zeros((2 * S + 1, 2 * S + 1), np.uint32)
    lib().align_scores(_p(q), _p(c), q.shape[0], S, _p(out))
    return out


def guess(angle_guess, k, yaw_step, flip) -> np.ndarray:
    T = np.zeros(16, np.float32)
    lib().align_guess(angle_guess, k, yaw_step, flip, _p(T))
    return T


def hit(query, cand_grid, angle_guess, params: AlignParams | None = None, lidar_to_ground: float = 2.0, want_tables=False):
    """One hit: (results (2,) ICP_RESULT_DTYPE, best int, detail (2,) ALIGN_DETAIL_DTYPE[, scores (2, 2K + 1, 2S + 1, 2S + 1),
    query grids (2, 2K + 1, G, G)]); cand_grid None: no candidate."""
    prm = params if params is not None else align_params()
    query = np.ascontiguousarray(query, dtype=POINT_DTYPE)
    cg = None if cand_grid is None else np.ascontiguousarray(cand_grid, np.uint8)
    res, det, best = np.zeros(2, ICP_RESULT_DTYPE), np.zeros(2, ALIGN_DETAIL_DTYPE), np.zeros(1, np.int32)
    side, nk = 2 * prm.max_shift + 1, 2 * prm.yaw_steps + 1
    sc = np.zeros((2, nk, side, side), np.uint32) if want_tables else None
    qg = np.zeros((2, nk, prm.grid, prm.grid), np.uint8) if want_tables else None
    lib().align_hit(_p(query), len(query), C.c_void_p(cg.ctypes.data) if cg is not None else None, C.byref(prm),
                    lidar_to_ground, angle_guess, _p(res), _p(best), _p(det), _p(sc), _p(qg))
    return (res, int(best[0]), det, sc, qg) if want_tables else (res, int(best[0]), det)


def hits(queries, cand_grids, hit_list, params: AlignParams | None = None, lidar_to_ground: float = 2.0):
    """A hit list of (query_idx, match_idx, angle_guess) records: (results (n, 2), best (n,), detail (n, 2)); equal hits are
    computed once."""
    n = len(hit_list)
    res, det, best = np.zeros((n, 2), ICP_RESULT_DTYPE), np.zeros((n, 2), ALIGN_DETAIL_DTYPE), np.zeros(n, np.int32)
    seen = {}
    for m, h in enumerate(hit_list):
        q, c, a = int(h["query_idx"]), int(h["match_idx"]), np.float32(h["angle_guess"])
        key = (q, max(c, -1), a.tobytes())
        if key not in seen:
            seen[key] = hit(queries[q], cand_grids[c] if c >= 0 else None, a, params, lidar_to_ground)
        res[m], best[m], det[m] = seen[key]
    return res, best, det
