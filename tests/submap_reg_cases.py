"""The checker and the seeded cases of scan-to-map registration (test_submap_registration_cpu.py,
test_submap_registration_gpu.py, test_cli_submap_registration_gpu.py).  The checker is a composition of what exists: the
fine stage's sequential voxel grid per frame (fineicp_lib.voxel_irct), the oracle's transform per entry
(oracle_lib.transform_cloud), concatenation in the map's entry order, the fine stage's sequential ICP (fineicp_lib.run).
Tests only."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

import fineicp_lib as fl
import oracle_lib as orc
from bev_amd import ICP_RESULT_DTYPE, MATCH_DTYPE, POINT_DTYPE

F32 = np.float32
IDENTITY = np.eye(3, 4, dtype=F32).reshape(12)
REG_MAX_TARGET = 1 << 22        # BEV_SUBMAP_REG_MAX_TARGET, restated
GRID_CELLS = 128 * 128          # kFineCells


def shift(dx=0.0, dy=0.0, dz=0.0) -> np.ndarray:
    m = np.eye(3, 4, dtype=F32)
    m[:, 3] = [dx, dy, dz]
    return m.reshape(12)


def planar(yaw_deg: float, tx: float, ty: float) -> np.ndarray:
    """reg_cases.rigid as a row-major 3 x 4"""
    a = np.deg2rad(float(yaw_deg))
    m = np.eye(3, 4, dtype=F32)
    m[0, 0] = m[1, 1] = F32(np.cos(a))
    m[0, 1], m[1, 0] = F32(-np.sin(a)), F32(np.sin(a))
    m[0, 3], m[1, 3] = F32(tx), F32(ty)
    return m.reshape(12)


class Maps:
    """The three host arrays of a submap call, built map by map: add([(frame, matrix), ...]) returns the map's index."""

    def __init__(self):
        self.offsets, self.frame, self.pose = [0], [], []

    def add(self, entries) -> int:
        for f, m in entries:
            self.frame.append(int(f))
            self.pose.append(np.asarray(m, F32).reshape(12))
        self.offsets.append(len(self.frame))
        return len(self.offsets) - 2

    def __len__(self):
        return len(self.offsets) - 1

    def entries(self, g):
        return [(self.frame[e], self.pose[e]) for e in range(self.offsets[g], self.offsets[g + 1])]

    def arrays(self):
        return (np.array(self.offsets, np.uint64), np.array(self.frame, np.int32),
                np.array(self.pose, F32).reshape(-1, 12))


def matches(rows) -> np.ndarray:
    return np.array([(int(q), int(g), F32(a)) for q, g, a in rows], MATCH_DTYPE)


def target(vox, entries) -> np.ndarray:
    """the concatenation, in the order given, of every entry's voxel cloud under its matrix"""
    parts = [orc.transform_cloud(vox[f], m) for f, m in entries]
    return np.concatenate(parts) if parts else np.zeros(0, POINT_DTYPE)


def expected(clouds, maps: Maps, m, prm, guesses=None, leaf=0.2, threads=16) -> np.ndarray:
    """(n,) ICP_RESULT_DTYPE: the checker's result of every match; guesses[k]: a 4 x 4, or None: the yaw guess"""
    used_maps = sorted({int(g) for g in m["match_idx"]})
    named = sorted({int(q) for q in m["query_idx"]} | {f for g in used_maps for f, _ in maps.entries(g)})
    with ThreadPoolExecutor(max(1, threads)) as ex:
        vox = dict(zip(named, ex.map(lambda f: fl.voxel_irct(clouds[f], leaf), named)))
        tgt = dict(zip(used_maps, ex.map(lambda g: target(vox, maps.entries(g)), used_maps)))
    res = np.zeros(len(m), ICP_RESULT_DTYPE)

    def one(k):
        g = fl.tool_guess(float(m["angle_guess"][k])) if guesses is None else guesses[k]
        res[k] = fl.run(vox[int(m["query_idx"][k])], tgt[int(m["match_idx"][k])], g, prm)

    with ThreadPoolExecutor(max(1, threads)) as ex:
        list(ex.map(one, range(len(m))))
    return res


# ---- the mirror tie ---------------------------------------------------------------------------------------------------------
def mirror_tie():
    """(clouds, maps, matches): frame 0 is A, 400 points on a lattice of 4 m (one point per voxel at leaf 0.2, so A is its own
    voxel cloud up to the voxel order; coordinates are multiples of 1 / 32, so moves by +-0.5 are exact in float32), frame 1
    the source: A moved by 0.125 in y, which lies on the mirror plane of A under x + 0.5 and A under x - 0.5.  Map 0 holds
    (A, x + 0.5) then (A, x - 0.5), map 1 the same entries the other way round.  Every source point is exactly as far from
    its own point's image in one entry as from its image in the other (0.25 + 1 / 64 squared, within both tools' distances;
    every other point is metres away), so its correspondence is decided by the entry order alone."""
    rng = np.random.default_rng(4242)
    cells = rng.choice(10 * 10 * 6, 400, replace=False)
    ix, iy, iz = cells % 10, (cells // 10) % 10, cells // 100
    a = np.zeros(400, POINT_DTYPE)
    a["x"] = (ix * 4.0 - 20.0 + 0.0625 + rng.integers(0, 2, 400) * 0.03125).astype(F32)
    a["y"] = (iy * 4.0 - 20.0 + 0.0625 + rng.integers(0, 2, 400) * 0.03125).astype(F32)
    a["z"] = (iz * 4.0 + 0.0625).astype(F32)
    a["label"] = 1
    src = a.copy()
    src["y"] = (a["y"] + F32(0.125)).astype(F32)
    maps = Maps()
    maps.add([(0, shift(0.5)), (0, shift(-0.5))])
    maps.add([(0, shift(-0.5)), (0, shift(0.5))])
    return [a, src], maps, matches([(1, 0, 0.0), (1, 1, 0.0)])
