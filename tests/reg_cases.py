"""Seeded inputs of the registration tests that go past one launch group (test_registration_cases_cpu.py anchors them to
plain references and proves on the host that they reach what they are for; test_registration_batch_gpu.py runs them on
the device).  Nothing here is read from disk: every cloud, match list and guess comes from a seed.  Tests only."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from bev_amd import ICP_RESULT_DTYPE, MATCH_DTYPE, POINT_DTYPE

F32 = np.float32

# the library's launch constants (bev_internal.h), restated: the cases exist to cross them
FINE_VOXEL_GROUP = 256       # kFineVoxelGroup: slots of one k_fine_voxel launch
PROBLEMS_PER_LAUNCH = 1024   # kFineProblemsPerLaunch, kIcpProblemsPerLaunch
CHUNK, CHUNK_SLOTS = 64, 32  # reg_pass: 32 chunk sums of 64 points in LDS at once
RF_LDS_KEYS = 8192           # kRfLdsKeys: more keys are sorted in global scratch
RF_MIN_CELL = 20             # kRfMinCellPoints

FIXED_LENGTHS = [0, 1, 2, 3, 19, 20, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049]
MAX_LENGTH = 4096
LEAF_RADIUS = [(0.2, 2.0), (0.35, 0.1), (0.35, 3.3), (1.0, 0.5), (5.0, 2.0), (0.05, 7.0), (500.0, 2.0), (1e-6, 2.0)]
CHUNK_SIZES = [63, 64, 65, 2047, 2048, 2049, 4097]


# ---- clouds with structure ----------------------------------------------------------------------------------------------
def scene(n: int, seed: int) -> np.ndarray:
    """n POINT_DTYPE records: five vertical wall segments (60 % of the points, labels -2, -1, 1, 2) and a noisy ground
    patch (mostly label 0), in a seeded random order."""
    rng = np.random.default_rng([int(seed), 0x5CE])
    ends = rng.uniform(-22, 22, (5, 2, 2))
    n_wall = int(round(0.6 * n))
    n_gnd = n - n_wall
    seg = rng.integers(0, 5, n_wall)
    t = rng.uniform(0, 1, n_wall)[:, None]
    wall_xy = ends[seg, 0] * (1 - t) + ends[seg, 1] * t + rng.normal(0, 0.02, (n_wall, 2))
    wall = np.c_[wall_xy, rng.uniform(0, 3, n_wall)]
    gnd = np.c_[rng.uniform(-22, 22, (n_gnd, 2)), -1.7 + rng.normal(0, 0.03, n_gnd)]
    lab_wall = rng.choice([-2, -1, 1, 2], n_wall)
    lab_gnd = np.where(rng.uniform(0, 1, n_gnd) < 0.85, 0, rng.choice([-2, -1, 1, 2], n_gnd))
    order = rng.permutation(n)
    xyz = np.concatenate([wall, gnd]).astype(F32)[order]
    out = np.zeros(n, POINT_DTYPE)
    out["x"], out["y"], out["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out["intensity"] = rng.uniform(0, 1, n).astype(F32)
    out["label"] = np.concatenate([lab_wall, lab_gnd])[order]
    out["row"], out["col"], out["t"] = 7, 9, 11  # no accumulator: the voxels carry 0, the overflow branch copies them
    return out


def rigid(yaw_deg: float, tx: float, ty: float) -> np.ndarray:
    """The 4 x 4 float32 transform of moved()."""
    a = np.deg2rad(float(yaw_deg))
    T = np.eye(4, dtype=F32)
    T[0, 0] = T[1, 1] = F32(np.cos(a))
    T[0, 1], T[1, 0] = F32(-np.sin(a)), F32(np.sin(a))
    T[0, 3], T[1, 3] = F32(tx), F32(ty)
    return T


def moved(cloud: np.ndarray, yaw_deg: float, tx: float, ty: float) -> np.ndarray:
    """The cloud turned by yaw_deg about z and shifted by (tx, ty), in float32; every other field as it was."""
    T = rigid(yaw_deg, tx, ty)
    out = cloud.copy()
    out["x"] = (T[0, 0] * cloud["x"] + T[0, 1] * cloud["y"]) + T[0, 3]
    out["y"] = (T[1, 0] * cloud["x"] + T[1, 1] * cloud["y"]) + T[1, 3]
    return out


def points(xyz) -> np.ndarray:
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    out = np.zeros(len(xyz), POINT_DTYPE)
    out["x"], out["y"], out["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return out


def finite_records(cloud) -> int:
    return int((np.isfinite(cloud["x"]) & np.isfinite(cloud["y"]) & np.isfinite(cloud["z"])).sum())


# ---- the ragged pack ------------------------------------------------------------------------------------------------------
SPECIAL_AT = {"all_nan": 7, "part_nan": 41, "identical": 130, "overflow": 201, "ground_only": 288}
HALF = 300


def _special(name: str, seed: int) -> np.ndarray:
    rng = np.random.default_rng([int(seed), 0x5BEC])
    if name == "all_nan":
        c = scene(40, seed + 1)
        c["x"] = c["y"] = c["z"] = np.nan
    elif name == "part_nan":  # NaN / inf in a tenth of the records
        c = scene(2000, seed + 2)
        bad = rng.permutation(2000)[:200]
        c["x"][bad[:70]] = np.nan
        c["y"][bad[70:130]] = np.inf
        c["z"][bad[130:]] = -np.inf
    elif name == "identical":
        c = scene(500, seed + 3)
        c["x"], c["y"], c["z"] = F32(3.25), F32(-8.5), F32(0.75)
    elif name == "overflow":  # the voxel grid's "leaf size is too small" branch at leaf 0.2: the output is the input
        c = scene(600, seed + 4)
        c["x"][333] = c["y"][333] = c["z"][333] = F32(1e6)
    else:  # ground_only: nothing for the top part
        c = scene(1500, seed + 5)
        c["label"] = 0
    return c


def ragged_pack(seed: int = 2026):
    """600 packed frames: HALF base frames and a moved copy of each (frame HALF + i is frame i moved by yaw[i], tr[i]).
    .clouds, .offsets (uint64, 601), .special (name -> base index), .degenerate (frames no ICP can use), .yaw, .tr."""
    rng = np.random.default_rng([int(seed), 1])
    n_plain = HALF - len(SPECIAL_AT)
    lens = FIXED_LENGTHS * 2 + [MAX_LENGTH, MAX_LENGTH]
    lens += rng.integers(300, 4001, n_plain - len(lens)).tolist()
    lens = [lens[k] for k in rng.permutation(len(lens))]
    base = [scene(n, 1000 * seed + k) for k, n in enumerate(lens)]
    for name, at in sorted(SPECIAL_AT.items(), key=lambda kv: kv[1]):
        base.insert(at, _special(name, seed))
    assert len(base) == HALF
    yaw = rng.uniform(-15, 15, HALF).astype(F32)
    tr = rng.uniform(-1, 1, (HALF, 2)).astype(F32)
    clouds = base + [moved(base[i], yaw[i], tr[i, 0], tr[i, 1]) for i in range(HALF)]
    offsets = np.zeros(len(clouds) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(c) for c in clouds])
    degenerate = {f for f, c in enumerate(clouds) if finite_records(c) < 3}
    degenerate |= {SPECIAL_AT["identical"], HALF + SPECIAL_AT["identical"]}  # one voxel: never three correspondences from it
    return SimpleNamespace(clouds=clouds, offsets=offsets, special=dict(SPECIAL_AT), degenerate=degenerate, yaw=yaw, tr=tr,
                           half=HALF, seed=seed)


def packed(clouds) -> np.ndarray:
    total = sum(len(c) for c in clouds)
    return np.concatenate(clouds) if total else np.zeros(1, POINT_DTYPE)


def ragged_matches(pack, seed: int = 7):
    """(matches MATCH_DTYPE, truth): truth[k] is the 4 x 4 motion that registers the source of match k on its target where
    the pack knows it (a frame against its moved copy, either way, and self matches), else None."""
    rng = np.random.default_rng([int(seed), 2])
    H = pack.half
    special = set(pack.special.values())
    plain = [i for i in range(H) if i not in special]
    unnamed = set(rng.choice(plain, 12, replace=False).tolist())  # neither they nor their copies are in any match
    named = [i for i in range(H) if i not in unnamed]
    out = []
    for i in named:
        T = rigid(pack.yaw[i], pack.tr[i, 0], pack.tr[i, 1])
        out.append((i, H + i, float(pack.yaw[i]) + rng.uniform(-2, 2), T))
        if i % 3 == 0 and i < 100:
            out.append((H + i, i, -float(pack.yaw[i]) + rng.uniform(-2, 2), np.linalg.inv(T.astype(np.float64)).astype(F32)))
    for i in range(100):  # consecutive pairs: frames 100 .. of the base half stay sources only, their copies targets only
        if i not in unnamed and i + 1 not in unnamed:
            out.append((i, i + 1, rng.uniform(-3, 3), None))
    for f in rng.choice(named, 10, replace=False).tolist() + sorted(special):
        out.append((f, f, 0.0, np.eye(4, dtype=F32)))
    for s in sorted(special):  # every special frame on both sides
        for r in rng.choice([i for i in named[:100] if i not in special], 2, replace=False).tolist():
            out.append((s, r, rng.uniform(-5, 5), None))
            out.append((r, s, rng.uniform(-5, 5), None))
    pool = [i for i in named if i < 100 and len(pack.clouds[i]) <= 1500]  # (short frames: the checker's time)
    pool += [H + i for i in pool]
    while len(out) < 2 * PROBLEMS_PER_LAUNCH + 320:
        q, t = rng.choice(pool, 2, replace=False).tolist()
        out.append((q, t, rng.uniform(-20, 20), None))
    out = [out[k] for k in rng.permutation(len(out))]
    for _ in range(40):  # exact duplicates of earlier matches
        k = int(rng.integers(0, len(out)))
        out.insert(int(rng.integers(k + 1, len(out) + 1)), out[k])
    m = np.zeros(len(out), MATCH_DTYPE)
    m["query_idx"] = [o[0] for o in out]
    m["match_idx"] = [o[1] for o in out]
    m["angle_guess"] = np.array([o[2] for o in out], F32)
    return m, [o[3] for o in out]


def slot_positions(matches) -> dict:
    """frame -> slot of the batched fine call: the order of first appearance, the source of a match before its target
    (bev_fine_registration_device_resident)."""
    pos = {}
    for q, t in zip(matches["query_idx"].tolist(), matches["match_idx"].tolist()):
        for f in (q, t):
            if f not in pos:
                pos[f] = len(pos)
    return pos


def synthetic_coarse(matches, truth, seed: int = 11):
    """Made-up outputs of the coarse entry for the top-part fine call: (coarse (n, 2) ICP_RESULT_DTYPE, best (n,) int32,
    guesses: the 4 x 4 the fine stage must start from, coarse[k, best[k]].T).  The chosen record is a rigid motion near the
    truth (near the yaw guess where the truth is unknown), the other one far off; a few chosen records hold NaN or are
    not rigid."""
    rng = np.random.default_rng([int(seed), 3])
    n = len(matches)
    coarse = np.zeros((n, 2), ICP_RESULT_DTYPE)
    best = rng.integers(0, 2, n).astype(np.int32)
    for k in range(n):
        if truth[k] is not None:
            T = rigid(rng.uniform(-1, 1), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)) @ truth[k]
        else:
            T = rigid(float(matches["angle_guess"][k]), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5))
        off = rigid(float(matches["angle_guess"][k]) + 90.0, 5.0, -5.0)
        coarse[k, best[k]]["T"] = T.astype(F32).reshape(16)
        coarse[k, 1 - best[k]]["T"] = off.reshape(16)
        coarse[k]["fitness"] = rng.uniform(0, 2, 2)
        coarse[k]["converged"], coarse[k]["iterations"], coarse[k]["state"] = 1, 10, 1
    for j, k in enumerate(rng.choice(n, 12, replace=False).tolist()):
        T = coarse[k, best[k]]["T"].reshape(4, 4).copy()
        if j % 3 == 0:
            T[j % 3, (j // 3) % 4] = np.nan
        elif j % 3 == 1:
            T[:3, :3] *= F32(1.3)  # a scale
        else:
            T[0, 1] += F32(0.4)    # a shear
        coarse[k, best[k]]["T"] = T.reshape(16)
    # one of them past the first launch of 1024 problems
    assert n > PROBLEMS_PER_LAUNCH
    guesses = [coarse[k, best[k]]["T"].reshape(4, 4).copy() for k in range(n)]
    return coarse, best, guesses


# ---- PointNormal frames for the coarse entry ---------------------------------------------------------------------------
def point_normals(xyz, seed: int) -> np.ndarray:
    """(n, 12) pcl::PointNormal rows: the points with unit normals in the plane from a seeded angle."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    ang = np.random.default_rng([int(seed), 4]).uniform(0, 2 * np.pi, len(xyz))
    out = np.zeros((len(xyz), 12), F32)
    out[:, :3] = xyz
    out[:, 4], out[:, 5] = np.cos(ang), np.sin(ang)
    return out


def coarse_frames(pack, chain, n_pairs: int = 150, seed: int = 13):
    """PointNormal frames for the coarse entry: chain(cloud) (the front end's checker) of n_pairs base frames of the pack
    with enough points above ground and of their moved copies, then hand-made frames.  Returns .frames, .stride (smaller
    than the longest frame), .counts (the true lengths), .matches, .hand (name -> index)."""
    rng = np.random.default_rng([int(seed), 5])
    H = pack.half
    special = set(pack.special.values())
    src = [i for i in range(H) if i not in special and len(pack.clouds[i]) >= 1200][:n_pairs]
    assert len(src) == n_pairs
    frames = [chain(pack.clouds[i]) for i in src] + [chain(pack.clouds[H + i]) for i in src]
    P = n_pairs
    big = frames[0]
    hand = {}
    for name, fr in [
        ("rows0", np.zeros((0, 12), F32)), ("rows1", big[:1].copy()), ("rows2", big[5:7].copy()),
        ("nan_normals", big.copy()), ("bad_points", frames[1].copy()), ("ground_only", chain(pack.clouds[pack.special["ground_only"]])),
    ]:
        hand[name] = len(frames)
        frames.append(np.ascontiguousarray(fr, F32))
    frames[hand["nan_normals"]][::3, 4:7] = np.nan
    frames[hand["bad_points"]][::7, 0] = np.nan
    frames[hand["bad_points"]][1::11, 1] = np.inf
    counts = np.array([len(f) for f in frames], np.int32)
    stride = int(np.sort(counts)[int(0.75 * len(counts))])  # a quarter of the frames are longer
    out = []
    for k, i in enumerate(src):
        out.append((k, P + k, float(pack.yaw[i]) + rng.uniform(-2, 2)))
        out.append((P + k, k, -float(pack.yaw[i]) + rng.uniform(-2, 2)))
    for k in rng.choice(2 * P, 20, replace=False).tolist():
        out.append((k, k, rng.uniform(-5, 5)))
    for name, h in hand.items():  # empty and tiny frames as source and as target
        for r in rng.choice(2 * P, 3, replace=False).tolist():
            out.append((h, r, rng.uniform(-5, 5)))
            out.append((r, h, rng.uniform(-5, 5)))
    out.append((hand["rows0"], hand["rows0"], 0.0))
    while len(out) < PROBLEMS_PER_LAUNCH + 120:
        q, t = rng.choice(2 * P, 2, replace=False).tolist()
        out.append((q, t, rng.uniform(-180, 180)))
    out = [out[k] for k in rng.permutation(len(out))]
    m = np.array(out, MATCH_DTYPE)
    return SimpleNamespace(frames=frames, stride=stride, counts=counts, matches=m, hand=hand)


def strided(frames, stride: int) -> np.ndarray:
    """(F, stride, 12) float32: the d_pn layout, every frame cut at stride rows."""
    out = np.zeros((len(frames), stride, 12), F32)
    for f, fr in enumerate(frames):
        k = min(len(fr), stride)
        out[f, :k] = fr[:k]
    return out


# ---- skewed geometry for the grid search -----------------------------------------------------------------------------------
SKEW_N = 3000
ONE_CELL = ("outlier", "vertical_line", "identical", "subnormal_extent")  # every point but one in one cell of the grid


def skewed_targets(seed: int = 5):
    """[(name, (3000, 3) float32)]: target clouds on which the search grid of reg_grid_build degenerates."""
    rng = np.random.default_rng([int(seed), 6])
    n = SKEW_N
    far = np.c_[1e5 + rng.uniform(-2.5, 2.5, n), -1e5 + rng.uniform(-2.5, 2.5, n), rng.uniform(-0.5, 0.5, n)]
    outlier = rng.uniform(-5, 5, (n, 3))
    outlier[1234] = [1e6, -1e6, 0.0]
    strip = np.c_[rng.uniform(0, 1000, n), rng.uniform(0, 1, n), rng.uniform(0, 0.5, n)]
    vline = np.c_[np.full(n, 2.5), np.full(n, -1.25), rng.uniform(0, 30, n)]
    same = np.tile([[4.0, 5.0, 6.0]], (n, 1))
    sub = np.zeros((n, 3), F32)
    sub[:, 0] = (np.arange(n) % 10).astype(F32) * F32(1e-39)  # extent 9e-39: the cell size's reciprocal overflows
    sub[:, 2] = rng.uniform(-1, 1, n)
    two = np.r_[rng.uniform(-0.5, 0.5, (n // 2, 3)) + [-40, 0, 0], rng.uniform(-0.5, 0.5, (n - n // 2, 3)) + [40, 0, 0]]
    g = np.stack(np.meshgrid(np.arange(55), np.arange(55)), -1).reshape(-1, 2)[:n] - 27
    lattice = np.c_[g, np.zeros(n)]
    out = [("far", far), ("outlier", outlier), ("strip", strip), ("vertical_line", vline), ("identical", same),
           ("subnormal_extent", sub), ("two_clusters", two), ("lattice", lattice)]
    return [(name, np.ascontiguousarray(a, F32)) for name, a in out]


SOURCE_KINDS = ("near", "outside", "itself")


def skewed_source(name: str, tgt: np.ndarray, kind: str, D: float, seed: int = 9) -> np.ndarray:
    """near: the target with a jitter of 0.3 (on the lattice half of the points instead moved by exactly half a step: ties);
    outside: the target's y and z at x beyond the target's box by less than min(D, 100) / 2; itself."""
    rng = np.random.default_rng([int(seed), 7, SOURCE_KINDS.index(kind), len(name)])
    if kind == "itself":
        return tgt.copy()
    if kind == "near":
        src = (tgt + rng.uniform(-0.3, 0.3, tgt.shape)).astype(F32)
        if name == "lattice":
            src[::2] = tgt[::2] + np.array([0.5, 0.0, 0.0], F32)
        return src
    fin = tgt[np.isfinite(tgt).all(axis=1)]
    src = tgt.copy()
    src[:, 0] = (fin[:, 0].max() + rng.uniform(0.05, 0.45, len(tgt)) * min(float(D), 100.0)).astype(F32)
    return src


def brute_nn(tgt, q):
    """numpy float32 brute force with the kernel's expression (dx*dx + dy*dy) + dz*dz: (index of the nearest finite target,
    lowest on ties; its squared distance)."""
    tgt = np.asarray(tgt, F32).reshape(-1, 3)
    q = np.asarray(q, F32).reshape(-1, 3)
    ok = np.isfinite(tgt).all(axis=1)
    idx = np.zeros(len(q), np.uint32)
    dist = np.zeros(len(q), F32)
    with np.errstate(all="ignore"):
        for k in range(len(q)):
            dx, dy, dz = q[k, 0] - tgt[:, 0], q[k, 1] - tgt[:, 1], q[k, 2] - tgt[:, 2]
            d = (dx * dx + dy * dy) + dz * dz
            d = np.where(ok, d, F32(np.inf))
            j = int(np.argmin(d))  # the first of equal values
            idx[k], dist[k] = j, d[j]
    return idx, dist


# ---- packed frames for the front end -----------------------------------------------------------------------------------
def _cell_points(rng, gx: int, gy: int, n: int, label=1) -> np.ndarray:
    """n records of label `label` inside cell (gx, gy) of extractTopAndFlatten (20 m cells, centre -100 + 20 g)."""
    c = np.zeros(n, POINT_DTYPE)
    c["x"] = (-100 + 20 * gx + rng.uniform(-9, 9, n)).astype(F32)
    c["y"] = (-100 + 20 * gy + rng.uniform(-9, 9, n)).astype(F32)
    c["z"] = rng.uniform(0, 5, n).astype(F32)
    c["label"] = label
    c["intensity"] = rng.uniform(0, 1, n).astype(F32)
    return c


def front_pack(pack, seed: int = 17):
    """Packed frames for the front end: .clouds, .names.  Two cells of more than 8192 points in one frame (two regions of
    the global sort scratch); cells of exactly 8192, 8193, 19 and 20 points; a frame whose 100 cells hold 5 k + 3 points
    each; the ragged pack's special frames; plain scenes."""
    rng = np.random.default_rng([int(seed), 8])
    mix = lambda parts: np.concatenate(parts)[rng.permutation(sum(len(p) for p in parts))]
    two_big = mix([_cell_points(rng, 5, 5, 9000), _cell_points(rng, 2, 7, 12000), _cell_points(rng, 7, 1, 300),
                   _cell_points(rng, 4, 4, 2000, label=0)])
    exact = mix([_cell_points(rng, 3, 3, RF_LDS_KEYS), _cell_points(rng, 6, 6, RF_LDS_KEYS + 1),
                 _cell_points(rng, 0, 9, RF_MIN_CELL - 1), _cell_points(rng, 9, 0, RF_MIN_CELL)])
    worst = mix([_cell_points(rng, c // 10, c % 10, 5 * (4 + c % 7) + 3) for c in range(100)])
    clouds = [two_big, exact, worst] + [pack.clouds[i] for i in pack.special.values()]
    names = ["two_big_cells", "cells_8192_8193_19_20", "cells_5k_plus_3"] + list(pack.special)
    for k, n in enumerate([5000, 0, 1, 3000, 20, 2049, 800, 4096, 1500]):
        clouds.append(scene(n, 7000 + k))
        names.append(f"scene{n}")
    clouds.append(moved(scene(3000, 3), 30.0, 40.0, 40.0))  # x, y > 0: one voxel at leaf 500
    names.append("one_quadrant")
    return SimpleNamespace(clouds=clouds, names=names)


def small_frames(n_frames: int = 1100, seed: int = 19):
    """More than 1024 small frames (the offsets table of the packed front end grows past its first size)."""
    rng = np.random.default_rng([int(seed), 9])
    out = []
    for k in range(n_frames):
        c = scene(int(rng.integers(0, 90)), 9000 + k)
        c["x"] *= F32(0.2)  # a few cells with 20 points or more
        c["y"] *= F32(0.2)
        out.append(c)
    return out


def cell_counts(cloud) -> np.ndarray:
    """Points per cell of extractTopAndFlatten (100 counts), restated in numpy (round half away from zero)."""
    ok = (cloud["label"] != 0) & np.isfinite(cloud["x"]) & np.isfinite(cloud["y"]) & np.isfinite(cloud["z"])
    gx = np.trunc((cloud["x"][ok] + F32(100)) / F32(20) + F32(0.5) * np.sign(cloud["x"][ok] + F32(100)))
    gy = np.trunc((cloud["y"][ok] + F32(100)) / F32(20) + F32(0.5) * np.sign(cloud["y"][ok] + F32(100)))
    inside = (gx >= 0) & (gx < 10) & (gy >= 0) & (gy < 10)
    return np.bincount((gx[inside] * 10 + gy[inside]).astype(np.int64), minlength=100)
