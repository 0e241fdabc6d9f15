"""The inputs and the ground truth of the place-retrieval tests (test_place_cpu.py,
test_place_ground_truth_gpu.py), on the world of ground_truth_cases.py, which is imported and not edited.

Database: the seven frames of ground_truth_cases.setup() (the world within RANGE of the seven poses along the path).  Queries:
for every database pose P_f and every turn of TURNS, the world within RANGE of P_q = P_f * [Rz(turn) | d], d a seeded
displacement of at most 0.5 m in the frame's x-y plane: 49 frames.  The truth of query (f, turn) is frame f, and the yaw of
P_f^-1 P_q is the turn.  20 rings, 60 sectors, 18 m.  Tests only."""
from __future__ import annotations

import functools

import numpy as np

import ground_truth_cases as gt
from bev_amd import POINT_DTYPE, place_params

TURNS = (0.0, 47.0, 90.0, 133.0, 180.0, -95.0, -171.0)
MAX_SHIFT = 0.5
N_RINGS, N_SECTORS, MAX_RANGE = 20, 60, 18.0
SECTOR_DEG = 360.0 / N_SECTORS
LIDAR_TO_GROUND = 2.0  # every sensor's (bev_params_for_sensor)


def params():
    return place_params(N_RINGS, N_SECTORS, MAX_RANGE, True)


def frame_of(P) -> np.ndarray:
    """the world within RANGE of pose P, in P's coordinates, as POINT_DTYPE records (label 1), rounded to float32 last"""
    xyz, _ = gt.world()
    seen = np.flatnonzero(np.linalg.norm(xyz - P[:3, 3], axis=1) < gt.RANGE)
    inv = gt.inverse(P)
    local = (xyz[seen] @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    c = np.zeros(len(seen), POINT_DTYPE)
    c["x"], c["y"], c["z"] = local[:, 0], local[:, 1], local[:, 2]
    c["intensity"], c["label"] = 1.0, 1
    return c


@functools.lru_cache(maxsize=None)
def case():
    """dict: db_poses, db_clouds (7); q_poses, q_clouds (49); truth (49,) the database frame of each query; turn (49,) the yaw
    of P_db^-1 P_q in degrees"""
    S = gt.setup()
    rng = np.random.default_rng(20266)
    db_poses = S["poses"][: gt.N_POSES]
    q_poses, truth, turn = [], [], []
    for f, P in enumerate(db_poses):
        for t in TURNS:
            r, a = MAX_SHIFT * np.sqrt(rng.uniform()), rng.uniform(0, 2 * np.pi)
            q_poses.append(P @ gt.pose(0.0, 0.0, t, [r * np.cos(a), r * np.sin(a), 0.0]))
            truth.append(f)
            turn.append(t)
    return dict(db_poses=db_poses, db_clouds=[frame_of(P) for P in db_poses], q_poses=q_poses,
                q_clouds=[frame_of(P) for P in q_poses], truth=np.array(truth), turn=np.array(turn))


def yaw_of(T) -> float:
    return float(np.degrees(np.arctan2(T[1, 0], T[0, 0])))


def angle_error(a, b) -> float:
    """|a - b| in degrees on the circle"""
    return abs((float(a) - float(b) + 180.0) % 360.0 - 180.0)
