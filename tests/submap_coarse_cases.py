"""The checker and the seeded cases of scan-to-map coarse ICP (test_submap_coarse_registration_cpu.py,
test_submap_coarse_registration_gpu.py, test_cli_submap_top_part_registration_gpu.py).  The checker is a composition of what
exists: the move of a PointNormal record restated in numpy float32 (plain float32 products and sums in the pinned association
are exact restatements; NaNs canonicalised), concatenation in the map's entry order, the coarse stage's sequential ICP per guess
(icp_lib.run) and its choice (icp_lib.best).  Tests only."""
from __future__ import annotations

import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import icp_lib
import submap_reg_cases as sc
from bev_amd import ICP_NO_CORRESPONDENCES, ICP_RESULT_DTYPE

F32 = np.float32
COARSE_MAX_TARGET = 1 << 22     # BEV_SUBMAP_COARSE_MAX_TARGET, restated
GRID_CELLS = 64 * 64            # kIcpCells
QNAN = np.uint32(0x7FC00000)


def _canon(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, F32)
    a.view(np.uint32)[np.isnan(a)] = QNAN
    return a


def move(rows, m) -> np.ndarray:
    """(n, 12) PointNormal rows under the row-major 3 x 4 m, in float32 without FMA: position component i =
    m[i][0] x + (m[i][1] y + (m[i][2] z + m[i][3])), normal component i = m[i][0] nx + (m[i][1] ny + m[i][2] nz); the
    curvature copied, the pads 0, every NaN 0x7fc00000."""
    r = np.asarray(rows, F32).reshape(-1, 12)
    m = np.asarray(m, F32).reshape(3, 4)
    out = np.zeros_like(r)
    x, y, z, nx, ny, nz = r[:, 0], r[:, 1], r[:, 2], r[:, 4], r[:, 5], r[:, 6]
    with np.errstate(all="ignore"):
        for i in range(3):
            out[:, i] = m[i, 0] * x + (m[i, 1] * y + (m[i, 2] * z + m[i, 3]))
            out[:, 4 + i] = m[i, 0] * nx + (m[i, 1] * ny + m[i, 2] * nz)
    out[:, 8] = r[:, 8]
    return _canon(out)


def target(frames, entries, stride=None) -> np.ndarray:
    """the concatenation, in the order given, of every entry's rows (cut at stride) under its matrix"""
    parts = [move(frames[f][:stride], m) for f, m in entries]
    return np.concatenate(parts) if parts else np.zeros((0, 12), F32)


def expected(frames, maps: sc.Maps, m, prm=None, stride=None, threads=16):
    """(results (n, 2) ICP_RESULT_DTYPE, best (n,) int32): the checker's results of every match and guess"""
    used = sorted({int(g) for g in m["match_idx"]})
    tgt = {g: target(frames, maps.entries(g), stride) for g in used}
    res = np.zeros((len(m), 2), ICP_RESULT_DTYPE)

    def one(k):
        i, g = divmod(k, 2)
        res[i, g] = icp_lib.run(frames[int(m["query_idx"][i])][:stride], tgt[int(m["match_idx"][i])],
                                icp_lib.tool_guess(float(m["angle_guess"][i]), g), prm)

    with ThreadPoolExecutor(max(1, threads)) as ex:
        list(ex.map(one, range(2 * len(m))))
    best = np.array([icp_lib.best(float(r[0]["fitness"]), float(r[1]["fitness"])) for r in res], np.int32).reshape(-1)
    return res, best


def pose3d(roll_deg, pitch_deg, yaw_deg, tx, ty, tz) -> np.ndarray:
    """Rz(yaw) Ry(pitch) Rx(roll) and a translation as a row-major 3 x 4 float32"""
    r, p, y = np.deg2rad([float(roll_deg), float(pitch_deg), float(yaw_deg)])
    rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    m = np.zeros((3, 4), F32)
    m[:, :3] = (rz @ ry @ rx).astype(F32)
    m[:, 3] = [tx, ty, tz]
    return m.reshape(12)


def frame(n: int, seed: int) -> np.ndarray:
    """n PointNormal rows of a scene in three dimensions, in a seeded order: five vertical wall segments (60 % of the rows;
    the unit normal is the segment's, turned towards the origin as the front end turns its normals) and a ground patch (the
    normal is +z).  The front end's own clouds (regfront_lib.chain) are flat, z = 0 and nz = 0: against a map whose entries
    roll and pitch them, the step along z is v / M with both of the order nz^2, and the checker itself loses its
    correspondences (measured: a third of such matches keep them).  With walls AND ground all six unknowns are determined, so
    the seeded list can ask that the reference converges."""
    rng = np.random.default_rng([int(seed), 0x3D])
    ends = rng.uniform(-22, 22, (5, 2, 2))
    n_wall = int(round(0.6 * n))
    seg = rng.integers(0, 5, n_wall)
    t = rng.uniform(0, 1, n_wall)[:, None]
    wall_xy = ends[seg, 0] * (1 - t) + ends[seg, 1] * t + rng.normal(0, 0.02, (n_wall, 2))
    d = ends[:, 1] - ends[:, 0]
    nrm = np.c_[-d[:, 1], d[:, 0]] / np.linalg.norm(d, axis=1)[:, None]
    nrm = nrm[seg] * np.where((nrm[seg] * wall_xy).sum(axis=1) > 0, -1.0, 1.0)[:, None]
    out = np.zeros((n, 12), F32)
    out[:n_wall, :2], out[:n_wall, 2] = wall_xy, rng.uniform(0, 3, n_wall)
    out[:n_wall, 4:6] = nrm
    out[n_wall:, :2], out[n_wall:, 2] = rng.uniform(-22, 22, (n - n_wall, 2)), -1.7 + rng.normal(0, 0.03, n - n_wall)
    out[n_wall:, 6] = 1.0
    out[:, 8] = rng.uniform(0, 0.3, n)
    return np.ascontiguousarray(out[rng.permutation(n)])


def group_count(maps: sc.Maps, m, stride: int, cap: int):
    """the plan's greedy rule restated for PointNormal maps: (launch groups, maps alone above the cap)"""
    used = sorted({int(g) for g in m["match_idx"]})
    groups, cur, alone = 0, 0, 0
    for g in used:
        b = 64 * len(maps.entries(g)) * stride + 4 * (GRID_CELLS + 1) + 32
        if cur and cur + b > cap:
            groups, cur = groups + 1, 0
        alone += b > cap
        cur += b
    return groups + (1 if cur else 0), alone


# ---- the seeded list ----------------------------------------------------------------------------------------------------------
LIST_STRIDE = 400   # a part of the frames are longer: their counts stay above it


@functools.lru_cache(maxsize=None)
def seeded_list():
    """dict: frames (80: 40 ragged frames of 0 .. 512 rows and a moved copy of each), stride, maps (0 .. 79: frame f under the
    identity; 80 .. 119: one to six entries under planar and full 3-D poses, the first entry a frame whose moved copy or
    original is the map's own query; 120: no entries), m (about a thousand matches, the first n_id against identity maps)."""
    rng = np.random.default_rng(20262)
    sizes = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512] + rng.integers(100, 513, 28).tolist()
    H = len(sizes)
    base = [frame(n, 8000 + k) for k, n in enumerate(sizes)]
    near = [sc.planar(rng.uniform(-3, 3), *rng.uniform(-0.7, 0.7, 2)) for _ in range(H)]
    frames = base + [move(base[i], near[i]) for i in range(H)]
    good = [f for f in range(2 * H) if len(frames[f]) >= 63]
    maps = sc.Maps()
    for f in range(2 * H):
        maps.add([(f, sc.IDENTITY)])

    def any_pose(k):
        if k % 2:
            return sc.planar(rng.uniform(-4, 4), *rng.uniform(-1, 1, 2))
        return pose3d(rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-4, 4), *rng.uniform(-1, 1, 2), rng.uniform(-0.3, 0.3))

    for i in range(H):
        entries = [(H + i, pose3d(rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-2, 2), *rng.uniform(-0.3, 0.3, 3)))]
        for k in range(i % 6):
            entries.append((int(rng.choice(good)) if k % 3 else int(rng.integers(0, 2 * H)), any_pose(k)))
        maps.add(entries)
    empty = maps.add([])
    pick = lambda: int(rng.choice(good)) if rng.uniform() < 0.96 else int(rng.integers(0, 2 * H))
    rows = []
    for i in range(H):  # a frame against its moved copy under the identity, both ways
        rows.append((i, H + i, rng.uniform(-3, 3)))
        rows.append((H + i, i, rng.uniform(-3, 3)))
    n_id = 420
    while len(rows) < n_id:
        i = pick() % H
        rows.append((i, H + i, rng.uniform(-5, 5)) if rng.uniform() < 0.5 else (pick(), pick(), rng.uniform(-5, 5)))
    for i in range(H):  # every posed map by the original of its first entry
        rows.append((i, 2 * H + i, rng.uniform(-3, 3)))
    while len(rows) < 1000:
        i = pick() % H
        rows.append((i if rng.uniform() < 0.5 else H + i, 2 * H + i, rng.uniform(-4, 4)))
    rows += [(good[0], empty, 0.0), (0, empty, 2.0)]
    order = list(range(n_id)) + (n_id + rng.permutation(len(rows) - n_id)).tolist()
    m = sc.matches([rows[k] for k in order])
    return dict(frames=frames, stride=LIST_STRIDE, maps=maps, m=m, n_id=n_id, empty=empty, H=H)


@functools.lru_cache(maxsize=None)
def seeded_expected(threads=16):
    S = seeded_list()
    return expected(S["frames"], S["maps"], S["m"], None, S["stride"], threads)


def condition_share(res) -> float:
    """the share of matches whose two guesses both end with a state other than NO_CORRESPONDENCES after at least two iterations"""
    ok = (res["state"] != ICP_NO_CORRESPONDENCES) & (res["iterations"] >= 2)
    return float(ok.all(axis=1).mean())


# ---- the mirror tie -------------------------------------------------------------------------------------------------------------
def mirror_tie():
    """(frames, maps, matches): submap_reg_cases.mirror_tie's lattice made flat for the coarse stage.  Frame 0 is A, 400
    PointNormal rows on a flat lattice of 4 m (coordinates multiples of 1 / 32, so moves by +-0.5 are exact) with seeded unit
    normals in the plane whose nx is not 0; frame 1 the source: A's points moved by 0.125 in y, on the mirror plane of A under
    x + 0.5 and A under x - 0.5.  Map 0 holds (A, x + 0.5) then (A, x - 0.5), map 1 the other order.  Every source point is
    exactly as far from its own point's image in one entry as in the other (0.25 + 1 / 64 squared; every other point is metres
    away), so its first correspondence is decided by the entry order alone, and with it d = n . (t - s) = +-0.5 nx - 0.125 ny."""
    rng = np.random.default_rng(4243)
    cells = rng.choice(24 * 24, 400, replace=False)
    ix, iy = cells % 24, cells // 24
    xyz = np.zeros((400, 3), F32)
    xyz[:, 0] = (ix * 4.0 - 48.0 + 0.0625 + rng.integers(0, 2, 400) * 0.03125).astype(F32)
    xyz[:, 1] = (iy * 4.0 - 48.0 + 0.0625 + rng.integers(0, 2, 400) * 0.03125).astype(F32)
    xyz[:, 2] = F32(0.0625)
    ang = rng.uniform(-1.2, 1.2, 400) + np.pi * rng.integers(0, 2, 400)   # |cos| > 0.36
    a = np.zeros((400, 12), F32)
    a[:, :3] = xyz
    a[:, 4], a[:, 5] = np.cos(ang), np.sin(ang)
    src = a.copy()
    src[:, 1] = a[:, 1] + F32(0.125)
    maps = sc.Maps()
    maps.add([(0, sc.shift(0.5)), (0, sc.shift(-0.5))])
    maps.add([(0, sc.shift(-0.5)), (0, sc.shift(0.5))])
    return [a, src], maps, sc.matches([(1, 0, 0.0), (1, 1, 0.0)])
