"""The checker and the seeded cases of scan-to-map registration against maps thinned by a voxel grid over their union
(test_submap_voxel_registration_cpu.py, test_submap_voxel_registration_gpu.py,
test_cli_submap_voxel_registration_gpu.py).  The checker is a composition of what exists: §6k's target
(submap_reg_cases.target), the fine stage's sequential voxel grid over it (fineicp_lib.voxel_irct at map_leaf), the fine
stage's sequential ICP (fineicp_lib.run).  Tests only."""
from __future__ import annotations

import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import fineicp_lib as fl
import reg_cases as rc
import submap_reg_cases as sc
from bev_amd import ICP_RESULT_DTYPE, POINT_DTYPE

F32 = np.float32
TILE = 4096                     # bevsubvox::kTile, restated: keys a workgroup of the sort holds in LDS
MAP_LEAVES = (0.2, 0.5)


def thin(concat: np.ndarray, map_leaf: float) -> np.ndarray:
    """target(g) of a concatenation: the voxel grid over it, or (map_leaf 0) itself"""
    return fl.voxel_irct(concat, map_leaf) if map_leaf > 0 else concat


def voxel_clouds(clouds, frames, leaf=0.2, threads=16) -> dict:
    frames = sorted(set(int(f) for f in frames))
    with ThreadPoolExecutor(max(1, threads)) as ex:
        return dict(zip(frames, ex.map(lambda f: fl.voxel_irct(clouds[f], leaf), frames)))


def targets(clouds, maps: sc.Maps, map_ids, map_leaf, leaf=0.2, threads=16, vox=None) -> dict:
    """g -> (concat(g), target(g)) for the maps named"""
    map_ids = sorted(set(int(g) for g in map_ids))
    vox = vox if vox is not None else voxel_clouds(clouds, {f for g in map_ids for f, _ in maps.entries(g)}, leaf, threads)

    def one(g):
        c = sc.target(vox, maps.entries(g))
        return c, thin(c, map_leaf)

    with ThreadPoolExecutor(max(1, threads)) as ex:
        return dict(zip(map_ids, ex.map(one, map_ids)))


def expected(clouds, maps: sc.Maps, m, prm, map_leaf, guesses=None, leaf=0.2, threads=16) -> np.ndarray:
    """(n,) ICP_RESULT_DTYPE: the checker's result of every match against its map's thinned target"""
    vox = voxel_clouds(clouds, {int(q) for q in m["query_idx"]} |
                       {f for g in set(m["match_idx"].tolist()) for f, _ in maps.entries(int(g))}, leaf, threads)
    tgt = targets(clouds, maps, m["match_idx"], map_leaf, leaf, threads, vox)
    res = np.zeros(len(m), ICP_RESULT_DTYPE)

    def one(k):
        g = fl.tool_guess(float(m["angle_guess"][k])) if guesses is None else guesses[k]
        res[k] = fl.run(vox[int(m["query_idx"][k])], tgt[int(m["match_idx"][k])][1], g, prm)

    with ThreadPoolExecutor(max(1, threads)) as ex:
        list(ex.map(one, range(len(m))))
    return res


def rows(target: np.ndarray) -> np.ndarray:
    """(n, 4) float32: the cloud call's records of a target: x, y, z and a pad of 0"""
    out = np.zeros((len(target), 4), F32)
    out[:, 0], out[:, 1], out[:, 2] = target["x"], target["y"], target["z"]
    return out


def union_voxels(concat: np.ndarray, entry_of: np.ndarray, map_leaf: float):
    """the union grid restated in numpy for the conditions on the inputs only: (voxels, the largest number of points in a
    voxel that holds points of two or more entries).  Finite points, no overflow."""
    inv = F32(1.0) / F32(map_leaf)
    xyz = np.c_[concat["x"], concat["y"], concat["z"]].astype(F32)
    assert np.isfinite(xyz).all()
    ijk = np.floor(xyz * inv).astype(np.int64)
    ijk -= ijk.min(axis=0)
    div = ijk.max(axis=0) + 1
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    uniq, inverse, counts = np.unique(idx, return_inverse=True, return_counts=True)
    mixed = 0
    for v in np.nonzero(counts >= 3)[0]:
        if len(set(entry_of[inverse == v].tolist())) >= 2:
            mixed = max(mixed, int(counts[v]))
    return len(uniq), mixed


def entry_index(vox, entries) -> np.ndarray:
    """the entry of every point of submap_reg_cases.target(vox, entries)"""
    return np.concatenate([np.full(len(vox[f]), e, np.int32) for e, (f, _) in enumerate(entries)]) if entries else np.zeros(0, np.int32)


def coarse_table(m, seed: int = 23):
    """Made-up outputs of the coarse entry for some hundreds of matches (reg_cases.synthetic_coarse wants more than a
    launch of 1024): (coarse (n, 2) ICP_RESULT_DTYPE, best (n,) int32, guesses: the 4 x 4 the fine stage must start from,
    coarse[k, best[k]].T).  The chosen record is a rigid motion near the yaw guess, the other one far off; a few chosen
    records hold NaN or are not rigid."""
    rng = np.random.default_rng([int(seed), 0xC0A])
    n = len(m)
    coarse = np.zeros((n, 2), ICP_RESULT_DTYPE)
    best = rng.integers(0, 2, n).astype(np.int32)
    for k in range(n):
        a = float(m["angle_guess"][k])
        coarse[k, best[k]]["T"] = rc.rigid(a + rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)).reshape(16)
        coarse[k, 1 - best[k]]["T"] = rc.rigid(a + 90.0, 5.0, -5.0).reshape(16)
        coarse[k]["fitness"] = rng.uniform(0, 2, 2)
        coarse[k]["converged"], coarse[k]["iterations"], coarse[k]["state"] = 1, 10, 1
    for j, k in enumerate(rng.choice(n, min(n, 9), replace=False).tolist()):
        T = coarse[k, best[k]]["T"].reshape(4, 4).copy()
        if j % 3 == 0:
            T[0, (j // 3) % 4] = np.nan
        elif j % 3 == 1:
            T[:3, :3] *= F32(1.3)  # a scale
        else:
            T[0, 1] += F32(0.4)    # a shear
        coarse[k, best[k]]["T"] = T.reshape(16)
    guesses = [coarse[k, best[k]]["T"].reshape(4, 4).copy() for k in range(n)]
    return coarse, best, guesses


# ---- the main case ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def main_case():
    """24 scenes of at most 512 records, a moved copy of each as the query side, and 30 maps of 1 .. 8 entries: a scene and
    copies of it moved by a few centimetres and a fraction of a degree, so that neighbouring entries lie on top of each
    other as neighbouring sweeps do.  Map 30 has no entries.  400 matches: every map by the moved copy of its own scene
    first, then random pairs.  .clouds .maps .m .coarse .best .guesses .multi (the maps of two or more entries)"""
    rng = np.random.default_rng(20262)
    sizes = [0, 1, 2, 3, 64, 65, 255, 256, 257, 511, 512, 512] + rng.integers(150, 513, 12).tolist()
    H = len(sizes)
    base = [rc.scene(n, 8000 + k) for k, n in enumerate(sizes)]
    yaw = rng.uniform(-8, 8, H).astype(F32)
    tr = rng.uniform(-0.4, 0.4, (H, 2)).astype(F32)
    clouds = base + [rc.moved(base[i], yaw[i], tr[i, 0], tr[i, 1]) for i in range(H)]
    maps = sc.Maps()
    scene_of, multi = [], []
    for g in range(30):
        k = 1 + g % 8
        # the maps of one entry: the scenes of 0 .. 3 records; of two: scenes of 511 records or more (a voxel of three points
        # from two entries needs two of a scene's own centroids in one voxel of the union's grid, which small scenes lack)
        i = g // 8 if k == 1 else 9 + (g // 8) % 3 if k == 2 else 4 + g % (H - 4)
        entries = [(i, sc.IDENTITY)] + [(i, sc.planar(rng.uniform(-0.2, 0.2), *rng.uniform(-0.04, 0.04, 2))) for _ in range(k - 1)]
        maps.add(entries)
        scene_of.append(i)
        if k >= 2:
            multi.append(g)
    empty = maps.add([])
    pairs = [(H + scene_of[g], g, float(-yaw[scene_of[g]]) + rng.uniform(-2, 2)) for g in range(30)]
    pairs += [(int(rng.integers(0, 2 * H)), int(rng.integers(0, 30)), rng.uniform(-10, 10)) for _ in range(366)]
    pairs += [(7, empty, 0.0), (H + 9, empty, 2.0), (0, 9, 0.0), (1, 10, 0.0)]
    order = rng.permutation(len(pairs))
    m = sc.matches([pairs[k] for k in order])
    coarse, best, guesses = coarse_table(m)
    return dict(clouds=clouds, maps=maps, m=m, coarse=coarse, best=best, guesses=guesses, multi=multi, empty=empty)


@functools.lru_cache(maxsize=None)
def main_expected(settings: str, map_leaf: float, threads=16):
    S = main_case()
    if settings == "whole":
        return expected(S["clouds"], S["maps"], S["m"], fl.params(**fl.WHOLE), map_leaf, threads=threads)
    return expected(S["clouds"], S["maps"], S["m"], fl.params(**fl.FINE), map_leaf, S["guesses"], threads=threads)


# ---- the sort's boundaries ----------------------------------------------------------------------------------------------------
def lattice(n, seed, spacing=0.5):
    """n points with one point per voxel at leaf 0.2 (a lattice of `spacing` >= 0.25 m): the voxel cloud has n points"""
    rng = np.random.default_rng([int(seed), 0x1A7])
    side = int(np.ceil(n ** 0.5)) + 3
    cells = rng.choice(side * side, n, replace=False)
    c = np.zeros(n, POINT_DTYPE)
    c["x"] = ((cells % side) * spacing - side * spacing / 2 + 0.0625).astype(F32)
    c["y"] = ((cells // side) * spacing - side * spacing / 2 + 0.0625).astype(F32)
    c["z"] = (rng.integers(0, 4, n) * 0.5 + 0.0625).astype(F32)
    c["label"] = 1
    return c


SORT_COUNTS = (1, 255, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 8 * TILE + 1234)


@functools.lru_cache(maxsize=None)
def sort_case():
    """maps whose concatenations have exactly SORT_COUNTS points: two entries each (but for the one-point map), lattice
    frames whose voxel clouds are themselves, the second entry the first moved by 5 cm so that most union voxels hold two
    points.  One query, a lattice of 300 points, against every map.  (clouds, maps, matches, counts)"""
    clouds, maps, rows_ = [], sc.Maps(), []
    for k, n in enumerate(SORT_COUNTS):
        a = n // 2
        parts = [n] if n == 1 else [n - a, a]
        ent = []
        for e, cnt in enumerate(parts):
            clouds.append(lattice(cnt, 100 + 2 * k + e))
            ent.append((len(clouds) - 1, sc.shift(0.05 * e, 0.0, 0.0)))
        maps.add(ent)
    q = len(clouds)
    clouds.append(rc.moved(lattice(300, 100), 1.0, 0.05, 0.05))
    for g in range(len(maps)):
        rows_.append((q, g, 0.5))
    return clouds, maps, sc.matches(rows_), SORT_COUNTS
