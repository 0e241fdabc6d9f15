"""The inputs of the tests of the translation guess of retrieved pairs: seeded and hand-made clouds for the
checker and kernel tests (test_align_cpu.py, test_align_grid_gpu.py, test_align_hits_gpu.py), and the ground-truth case
(test_align_ground_truth_cpu.py, test_align_ground_truth_gpu.py) on the world of ground_truth_cases.py, which is imported and
not edited, built as place_cases.py builds its own.

Ground truth.  Database: the seven frames of ground_truth_cases.setup().  Queries: for every database pose P_f and every turn of
place_cases.TURNS, the world within RANGE of P_q = P_f * [Rz(turn) | d], d a seeded displacement of MIN_SHIFT ... MAX_SHIFT
metres in the frame's x-y plane: 49 frames.  T_true = P_f^-1 P_q = [Rz(turn) | d].  A hit is made from the truth: the frame, and
place_angle of the sector nearest to the turn; every other query's angle is turned by half a circle, so that its true flip is 1.
Tests only."""
from __future__ import annotations

import functools

import numpy as np

import ground_truth_cases as gt
import place_cases
from bev_amd import MATCH_DTYPE, POINT_DTYPE, align_params

F32 = np.float32
L2G = 2.0  # bev_params_for_sensor's lidar_to_ground


# ---- seeded and hand-made clouds -------------------------------------------------------------------------------------------------
def seeded(rng, n, G, cell):
    """points over 1.2 x the grid, heights from below 0 to above the 127 clamp, a fifth of the labels 0"""
    half = 0.5 * G * cell
    c = np.zeros(n, POINT_DTYPE)
    c["x"], c["y"] = rng.uniform(-1.2 * half, 1.2 * half, (2, n)).astype(F32)
    c["z"] = rng.uniform(-6.0, 40.0, n).astype(F32)
    c["label"] = rng.uniform(size=n) >= 0.2
    return c


def cloud_of(xy, z=1.0, label=1):
    xy = np.asarray(xy, F32).reshape(-1, 2)
    c = np.zeros(len(xy), POINT_DTYPE)
    c["x"], c["y"], c["z"], c["label"] = xy[:, 0], xy[:, 1], z, label
    return c


def edge_frame(G, cell):
    """points exactly on cell edges and one ulp to either side, at +-G/2 * cell and an ulp to either side, the origin, NaN, inf
    and -0.0 coordinates: POINT_DTYPE records of label 1 (every third 0), heights that differ per point; then one cell with NaN,
    inf, negative and clamped heights"""
    cell, up, down = F32(cell), F32(np.inf), F32(-np.inf)
    vals = []
    for k in (-G // 2, -G // 2 + 1, -3, -1, 0, 1, 2, G // 2 - 1, G // 2):
        e = F32(k) * cell
        vals += [np.nextafter(e, down), e, np.nextafter(e, up)]
    nz, inf, nan = F32(-0.0), F32(np.inf), F32(np.nan)
    mid = F32(0.37) * cell
    xy = [(v, mid) for v in vals] + [(mid, v) for v in vals] + [(v, v) for v in vals] + [(v, -v) for v in vals]
    xy += [(0.0, 0.0), (nz, nz), (nz, 0.0), (0.0, mid), (nz, mid), (mid, nz), (nan, mid), (mid, nan), (inf, mid), (mid, -inf),
           (inf, inf), (nan, nan), (F32(1e-30), 0.0), (F32(1e-23), F32(1e-23)), (F32(3e38), 1.0), (F32(-3e38), F32(3e38)),
           (F32(4e9) * cell, mid), (F32(-4e9) * cell, mid)]
    c = np.zeros(len(xy) + 4, POINT_DTYPE)
    c["x"][: len(xy)], c["y"][: len(xy)] = np.array(xy, F32).T
    c["z"] = 1.0 + (np.arange(len(c)) % 9) * 0.25
    c["label"] = np.arange(len(c)) % 3 != 0
    c["x"][len(xy):], c["y"][len(xy):] = F32(2.5) * cell, F32(-1.5) * cell  # one cell: NaN, inf, negative and clamped heights
    c["z"][len(xy):] = [nan, inf, -5.0, 1000.0]
    c["label"][len(xy):] = 1
    return c


def rigid12(roll, pitch, yaw, t):
    return gt.pose(roll, pitch, yaw, t)[:3].astype(F32).reshape(12)


def moved(cloud, yaw_deg, tx, ty):
    """the cloud as a sensor displaced by [Rz(yaw) | (tx, ty)] sees it: p_query = T^-1 p, so that p = T p_query"""
    inv = gt.inverse(gt.pose(0.0, 0.0, yaw_deg, [tx, ty, 0.0]))
    xyz = np.c_[cloud["x"], cloud["y"], cloud["z"]].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]
    out = cloud.copy()
    out["x"], out["y"], out["z"] = xyz[:, 0].astype(F32), xyz[:, 1].astype(F32), xyz[:, 2].astype(F32)
    return out


# ---- ground truth ---------------------------------------------------------------------------------------------------------------
MIN_SHIFT, MAX_SHIFT = 1.5, 3.0
GRID, CELL, SHIFT, YAW_STEPS, YAW_STEP = 64, 0.6, 8, 1, 2.0
SEED = 20267


def params():
    return align_params(GRID, CELL, SHIFT, YAW_STEPS, YAW_STEP, True)


def place_angle(n, n_sectors=place_cases.N_SECTORS) -> np.float32:
    """bev_place_exact.h's place_angle, restated"""
    a = F32(n) * (F32(360.0) / F32(n_sectors))
    return F32(a - F32(360.0)) if a >= F32(180.0) else a


@functools.lru_cache(maxsize=None)
def case():
    """dict: db_poses, db_clouds (7); q_poses, q_clouds (49); truth (49,) the database frame of each query; turn (49,); shift
    (49, 2) the displacement d; flip (49,) the true flip of each hit; hits (49,) MATCH_DTYPE over the frame list db + queries;
    T_true (49, 4, 4)"""
    S = gt.setup()
    rng = np.random.default_rng(SEED)
    db_poses = S["poses"][: gt.N_POSES]
    q_poses, truth, turn, shift, flip, hits, T_true = [], [], [], [], [], [], []
    for f, P in enumerate(db_poses):
        for t in place_cases.TURNS:
            r, a = rng.uniform(MIN_SHIFT, MAX_SHIFT), rng.uniform(0, 2 * np.pi)
            T = gt.pose(0.0, 0.0, t, [r * np.cos(a), r * np.sin(a), 0.0])
            k = len(q_poses)
            sector = int(np.floor(t / place_cases.SECTOR_DEG + 0.5)) % place_cases.N_SECTORS
            fl = k % 2
            angle = place_angle((sector + (place_cases.N_SECTORS // 2 if fl else 0)) % place_cases.N_SECTORS)
            q_poses.append(P @ T)
            truth.append(f), turn.append(t), shift.append(T[:2, 3]), flip.append(fl), T_true.append(T)
            hits.append((gt.N_POSES + k, f, angle))
    return dict(db_poses=db_poses, db_clouds=[place_cases.frame_of(P) for P in db_poses], q_poses=q_poses,
                q_clouds=[place_cases.frame_of(P) for P in q_poses], truth=np.array(truth), turn=np.array(turn),
                shift=np.array(shift), flip=np.array(flip), hits=np.array(hits, MATCH_DTYPE), T_true=np.array(T_true))


HAND_OVER = tuple(range(0, 49, 8))  # the queries handed to the fine stage: every database frame once, every turn once
ITERATIONS = (1, 2, 3, 8)           # ground_truth_cases.K: the iteration counts the fine stage is compared at


def frames(S=None):
    """one list: a hit's indices are the registration call's frame indices"""
    S = S or case()
    return S["db_clouds"] + S["q_clouds"]


def xyz32(cloud):
    return np.c_[cloud["x"], cloud["y"], cloud["z"]].astype(F32)


@functools.lru_cache(maxsize=None)
def checker_table():
    """(candidate grids (7, G, G), results (49, 2), best (49,), detail (49, 2)) of the sequential checker"""
    import align_lib

    S, prm = case(), params()
    grids = np.stack([align_lib.grid([(c, None)], prm, L2G) for c in S["db_clouds"]])
    return (grids,) + align_lib.hits(frames(S), grids, S["hits"], prm, L2G)


@functools.lru_cache(maxsize=None)
def trajectory(k, dtype_name="float64", bare=False):
    """iterates 1 .. 8 of ref64_registration's point-to-point run of hit k under the top-part fine settings' distance (D = 1):
    from the chosen record of the checker's table, or (bare) from the yaw guess of the true flip alone"""
    import ref64_registration as ref

    S, fr = case(), frames()
    h = S["hits"][k]
    if bare:
        start = ref.yaw_guess(h["angle_guess"], int(S["flip"][k]))
    else:
        _, res, best, _ = checker_table()
        start = res[k, best[k]]["T"].astype(np.float64).reshape(4, 4)
    return ref.point_to_point(xyz32(fr[h["query_idx"]]), xyz32(fr[h["match_idx"]]), start, gt.FINE_D, max(ITERATIONS),
                              np.dtype(dtype_name).type)


def tol(k) -> float:
    """§6o's rule: FACTOR times the largest distance, over the compared iterations, between the plain code in float32 and in
    float64 from the same start"""
    a, b = trajectory(k, "float64"), trajectory(k, "float32")
    return gt.FACTOR * max(float(np.abs(a[i - 1] - b[i - 1].astype(np.float64)).max()) for i in ITERATIONS)


def precompute(jobs, threads=None):
    """trajectory(*job) of every job on a few threads (numpy releases the GIL); later calls find them cached"""
    import os
    from concurrent.futures import ThreadPoolExecutor

    checker_table()
    with ThreadPoolExecutor(threads or min(16, os.cpu_count() or 4)) as ex:
        list(ex.map(lambda j: trajectory(*j), jobs))
