"""The seeded cases of the pair calls' search grids sized to the cloud (bev_set_pair_search_grid; DESIGN.md §6t;
test_pair_search_grid_gpu.py, test_cli_pair_search_grid_gpu.py): the smallest targets that cross the fixed grids' caps, 128 x 128
cells in the fine stage (18 000 points: ceil(sqrt) = 135) and 64 x 64 in the coarse one (5 400 rows: 74), the slot structures, the
calls past one launch and one build group, and the degenerate targets.  Sources are moved copies of their targets under the
tools' yaw-guess convention.  The expected values are the sequential checkers' (fineicp_lib, icp_lib), computed once per case:
the results do not depend on the grid.  The rule of the grid's size and the grid's restatement are submap_grid_cases'.
Tests only."""
from __future__ import annotations

import functools
import os

import numpy as np

import fineicp_lib as fl
import icp_lib as il
import reg_cases as rc
import submap_coarse_cases as cc
import submap_grid_cases as gc
import submap_reg_cases as sc
import submap_vox_cases as vc
from bev_amd import POINT_DTYPE

F32 = np.float32
THREADS = min(16, os.cpu_count() or 4)
FINE_CAP, COARSE_CAP, CAP_MAX = gc.FINE_CAP, gc.COARSE_CAP, 1024   # kFineGridMax, kIcpGridMax, BEV_PAIR_SEARCH_GRID_MAX
FINE_DIMS = (0, 8, 128, 130, 256, 1024)
COARSE_DIMS = (0, 4, 64, 70, 256)
BUILD_GROUP = 256                                                  # bevpair::kBuildGroup
PROBLEMS_PER_LAUNCH = rc.PROBLEMS_PER_LAUNCH


def xyz_of(cloud) -> np.ndarray:
    """(n, 3) float32 positions of POINT_DTYPE records or PointNormal rows"""
    if getattr(cloud, "dtype", None) == POINT_DTYPE:
        return np.c_[cloud["x"], cloud["y"], cloud["z"]].astype(F32)
    return np.asarray(cloud, F32).reshape(-1, 12)[:, :3]


def grid_expected(cloud, cap: int):
    """what the hook must say of a target's grid under the cap (the stage's own for D = 0): (cells on the long axis, searchable
    points, largest count of one cell), from the rule and the target's points"""
    xyz = xyz_of(cloud)
    xyz = xyz[np.isfinite(xyz).all(axis=1)]
    if len(xyz) == 0:
        return 1, 0, 0
    # the rule counts every point of the target, searchable or not
    nx, ny, largest = _grid_of(xyz, gc.grid_dim(len(xyz_of(cloud)), cap))
    return max(nx, ny), len(xyz), largest


def _grid_of(xyz, dim: int):
    """submap_grid_cases.grid_of for a given count of cells per axis"""
    mn, mx = xyz[:, :2].min(axis=0), xyz[:, :2].max(axis=0)
    ex, ey = F32(mx[0] - mn[0]), F32(mx[1] - mn[1])
    with np.errstate(all="ignore"):
        s = F32(max(ex, ey) / F32(dim))
        if not (s > 0 and np.isfinite(s) and np.isfinite(F32(1) / s)):
            return 1, 1, len(xyz)
        inv = F32(F32(1) / s)
        nx, ny = min(dim, int(F32(ex * inv)) + 1), min(dim, int(F32(ey * inv)) + 1)
        cx = np.clip(((xyz[:, 0] - mn[0]) * inv).astype(F32), 0, F32(nx - 1)).astype(np.int64)
        cy = np.clip(((xyz[:, 1] - mn[1]) * inv).astype(F32), 0, F32(ny - 1)).astype(np.int64)
    return nx, ny, int(np.bincount(cy * nx + cx).max())


def hook_matches(row, cloud, D: int, stage_cap: int) -> bool:
    nx, ny, n, largest = (int(v) for v in row)
    return (max(nx, ny), n, largest) == grid_expected(cloud, D if D else stage_cap)


# ---- fine: one problem on an 18 000-point target ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fine_pair():
    """dict: tgt (18 000 records: submap_grid_cases' five lattices under their poses, as one cloud), src (every fourth of them,
    moved), guess (the yaw guess near the motion), exp_top / exp_whole (the checker under both tools' settings)"""
    S = gc.fine_case()
    tgt = sc.target(S["clouds"], S["maps"].entries(0))
    src = rc.moved(tgt[::4], 1.0, 0.05, 0.05)
    guess = fl.tool_guess(-0.6)
    assert len(tgt) == 18000
    return dict(tgt=tgt, src=src, guess=guess, exp_top=fl.run(src, tgt, guess, fl.params(**fl.FINE)),
                exp_whole=fl.run(src, tgt, guess, fl.params(**fl.WHOLE)))


def pad(cloud, S: int) -> np.ndarray:
    """the cloud as a frame of d_ordered: S records, the rest not finite"""
    out = np.zeros(S, POINT_DTYPE)
    out["x"] = np.nan
    out[: len(cloud)] = cloud
    return out


@functools.lru_cache(maxsize=None)
def fine_frames(S: int):
    """dict: clouds (packed form: A and B whose voxel clouds have 18 000 and 17 000 points, a moved part of each, a small one),
    ordered (the same clouds as frames of S records), m, coarse / best / guesses (a made-up coarse table), exp_whole, exp_top"""
    a, b = vc.lattice(18000, 610), vc.lattice(17000, 611)
    clouds = [a, b, rc.moved(a[::5], 1.5, 0.1, -0.05), rc.moved(b[::5], -2.0, -0.1, 0.1), vc.lattice(900, 612)]
    m = sc.matches([(2, 0, -1.0), (3, 1, 2.5), (2, 0, -2.5), (4, 1, 0.0), (2, 1, 0.3), (3, 0, 1.0)])
    coarse, best, guesses = vc.coarse_table(m, seed=31)
    exp_whole = fl.fine(clouds, m, None, fl.params(**fl.WHOLE), threads=THREADS)
    exp_top = fl.fine(clouds, m, guesses, fl.params(**fl.FINE), threads=THREADS)
    assert max(len(c) for c in clouds) <= S
    return dict(clouds=clouds, ordered=[pad(c, S) for c in clouds], m=m, coarse=coarse, best=best, guesses=guesses,
                exp_whole=exp_whole, exp_top=exp_top, targets={0: a, 1: b})


# ---- coarse: a 5 400-row target ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coarse_pair():
    tgt = cc.frame(5400, 9700)
    src = cc.move(tgt[::3], sc.planar(1.5, 0.2, -0.1))
    guess = il.tool_guess(-1.0, 0)
    return dict(tgt=tgt, src=src, guess=guess, exp=il.run(src, tgt, guess))


@functools.lru_cache(maxsize=None)
def coarse_frames():
    """dict: frames (targets of 5 400 and 5 000 rows, a moved part of each), stride, m, exp = (results (n, 2), best)"""
    t0, t1 = cc.frame(5400, 9701), cc.frame(5000, 9702)
    frames = [t0, t1, cc.move(t0[::3], sc.planar(1.0, 0.3, -0.2)), cc.move(t1[::3], sc.planar(-2.0, -0.2, 0.1))]
    m = sc.matches([(2, 0, -1.0), (3, 1, 2.0), (2, 1, 0.5), (3, 0, 3.0)])
    return dict(frames=frames, stride=5400, m=m, exp=il.coarse(frames, m, threads=THREADS), targets={0: t0, 1: t1})


# ---- slot structure -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def structure_case():
    """small clouds: frame 0 the target of several matches; frame 1 a query and a target; frame 2 against itself; frame 3 a
    query only (no grid is built for it); the targets are frames 0, 1, 2.  dict with the fine and the coarse form"""
    clouds = [vc.lattice(700, 620), vc.lattice(500, 621), vc.lattice(300, 622), rc.moved(vc.lattice(700, 620)[::2], 1.0, 0.1, 0.1)]
    m = sc.matches([(3, 0, -1.0), (1, 0, 0.0), (3, 0, 0.5), (0, 1, 0.2), (2, 2, 0.4), (3, 1, 0.0)])
    frames = [cc.frame(600, 9710), cc.frame(400, 9711), cc.frame(300, 9712)]
    frames.append(cc.move(frames[0][::2], sc.planar(1.0, 0.2, 0.1)))
    return dict(clouds=clouds, m=m, exp_fine=fl.fine(clouds, m, None, fl.params(**fl.WHOLE), threads=THREADS),
                frames=frames, stride=640, exp_coarse=il.coarse(frames, m, threads=THREADS), n_targets=3, n_slots=4)


# ---- more problems than one launch, more targets than one build group ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_case():
    """300 tiny clouds; 1 030 fine matches and 520 coarse ones (1 040 problems at two guesses each), each list naming more than
    256 distinct targets"""
    rng = np.random.default_rng(20281)
    n = 300
    clouds = [vc.lattice(int(k), 700 + i) for i, k in enumerate(rng.integers(30, 90, n))]
    frames = [cc.frame(int(k), 9800 + i) for i, k in enumerate(rng.integers(30, 80, n))]

    def match_list(count):
        t = np.r_[np.arange(n), rng.integers(0, n, count - n)]
        q = (t + rng.integers(1, n, count)) % n
        return sc.matches(list(zip(q, t, rng.uniform(-3, 3, count))))

    mf, mc = match_list(PROBLEMS_PER_LAUNCH + 6), match_list(PROBLEMS_PER_LAUNCH // 2 + 8)
    assert len(mf) == 1030 and len(mc) == 520 and len(set(mf["match_idx"])) > BUILD_GROUP and len(set(mc["match_idx"])) > BUILD_GROUP
    return dict(clouds=clouds, mf=mf, exp_fine=fl.fine(clouds, mf, None, fl.params(**fl.WHOLE), threads=THREADS),
                frames=frames, stride=80, mc=mc, exp_coarse=il.coarse(frames, mc, threads=THREADS), n_targets=n)


# ---- degenerate targets -----------------------------------------------------------------------------------------------------------
def _rows(xyz, seed):
    return rc.point_normals(np.asarray(xyz, F32).reshape(-1, 3), seed)


@functools.lru_cache(maxsize=None)
def degenerate_case():
    """[(name, fine (src, tgt), coarse (src, tgt))]: targets on which the rule's branches end, for the per-cloud calls"""
    rng = np.random.default_rng(20282)
    base = rng.uniform(-10, 10, (600, 3)).astype(F32)
    line = np.c_[np.arange(200) * 0.5, np.full(200, 3.0), np.zeros(200)].astype(F32)
    clump = np.r_[np.c_[rng.uniform(0, 0.01, (4000, 2)), rng.uniform(0, 1, 4000)], [[1000.0, 0.0, 0.0]]].astype(F32)
    near = (clump[:300] + F32(0.02)).astype(F32)
    out = []
    for name, src, tgt in (("empty", base, base[:0]), ("non_finite", base, np.full((50, 3), np.nan, F32)),
                           ("one_point", base[:40] * F32(0.01), base[:1] * F32(0.01)), ("all_y_equal", line + F32(0.1), line),
                           ("clump", near, clump), ("query_outside", base + F32(500.0), base)):
        out.append((name, (rc.points(src), rc.points(tgt)), (_rows(src, 5), _rows(tgt, 6))))
    return out


@functools.lru_cache(maxsize=None)
def mirror_ties():
    """the mirror-tie targets of both stages as single clouds: ((fine src, [tgt in one entry order, the other]), (coarse ...)).
    Equal distances everywhere: the lowest target index must win, so the two orders give different results"""
    clouds, maps, _ = sc.mirror_tie()
    frames, cmaps, _ = cc.mirror_tie()
    fine = (clouds[1], [sc.target(clouds, maps.entries(g)) for g in (0, 1)])
    coarse = (frames[1], [np.concatenate([cc.move(frames[f], mm) for f, mm in cmaps.entries(g)]) for g in (0, 1)])
    return fine, coarse
