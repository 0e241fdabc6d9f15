"""The seeded cases of the scan-to-map search grids sized to the map (bev_set_submap_search_grid; DESIGN.md §6s;
test_submap_search_grid_gpu.py, test_cli_submap_search_grid_gpu.py): the smallest targets that cross the fixed grids' caps,
128 x 128 cells in the fine stage and 64 x 64 in the coarse one, and the rule of the grid's size restated in Python.  The
expected values are the existing checkers' (submap_reg_cases, submap_vox_cases, submap_coarse_cases, submap_pn_vox_cases,
submap_top_cases): the results do not depend on the grid.  Tests only."""
from __future__ import annotations

import functools
import math

import numpy as np

import reg_cases as rc
import submap_coarse_cases as cc
import submap_reg_cases as sc
import submap_top_cases as tc
import submap_vox_cases as vc

F32 = np.float32
FINE_CAP, COARSE_CAP, CAP_MAX = 128, 64, 1024   # kFineGridMax, kIcpGridMax, BEV_SUBMAP_SEARCH_GRID_MAX
PART_BYTES = 256 * 16 + 256 * 4                 # bevsubreg::kGridPartBytes: the build's partial bounds and sums per map


def grid_dim(n: int, cap: int) -> int:
    """bevsubreg::grid_dim restated: min(cap, max(1, ceil(sqrt(n)))); exact in integers for every n below 2^23"""
    r = math.isqrt(n)
    return min(cap, max(1, r if r * r == n else r + 1))


def grid_cells(capacity: int, cap: int) -> int:
    return grid_dim(capacity, cap) ** 2


def fine_map_bytes(capacity: int, cap: int) -> int:
    """bevsubreg::map_bytes(capacity, false, cap) restated: the moved and the searchable points, the grid, two headers"""
    if cap == 0:
        return 32 * capacity + 4 * (sc.GRID_CELLS + 1) + 32
    return 32 * capacity + 8 * (grid_cells(capacity, cap) + 1) + PART_BYTES + 64


def fine_group_count(capacities, cap: int, group_bytes: int):
    """the plan's greedy rule restated for the used maps' capacities in ascending map order: (launch groups, the maps of the
    last group)"""
    groups, cur, last = 0, 0, 0
    for c in capacities:
        b = fine_map_bytes(c, cap)
        if cur and cur + b > group_bytes:
            groups, cur, last = groups + 1, 0, 0
        cur += b
        last += 1
    return groups + (1 if cur else 0), last


def grid_of(xyz, cap: int):
    """reg_grid_build's header and counts restated in float32 for finite points: (nx, ny, largest count of one cell)"""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    n = len(xyz)
    mn, mx = xyz[:, :2].min(axis=0), xyz[:, :2].max(axis=0)
    ex, ey = F32(mx[0] - mn[0]), F32(mx[1] - mn[1])
    dim = grid_dim(n, cap)
    s = F32(max(ex, ey) / F32(dim))
    if not (s > 0 and np.isfinite(s) and np.isfinite(F32(1) / s)):
        return 1, 1, n
    inv = F32(F32(1) / s)
    nx, ny = min(dim, int(F32(ex * inv)) + 1), min(dim, int(F32(ey * inv)) + 1)
    cx = np.clip(((xyz[:, 0] - mn[0]) * inv).astype(F32), 0, F32(nx - 1)).astype(np.int64)
    cy = np.clip(((xyz[:, 1] - mn[1]) * inv).astype(F32), 0, F32(ny - 1)).astype(np.int64)
    return nx, ny, int(np.bincount(cy * nx + cx).max())


# ---- fine: 18 000 points, ceil(sqrt) = 135 > 128 -------------------------------------------------------------------------------
# (yaw in degrees, tx, ty): the five lattices nearly on top of each other, as the sweeps of a map are: the nodes' clusters stay
# inside one cell of every grid from 128 to 135 cells per axis, so that the largest cell does not grow with the grid's size (the
# cells of two grids are not nested: under poses that spread the lattices, 128 cells per axis gave 4 and 135 gave 5, on the CPU)
FINE_POSES = [(0.0, 0.0, 0.0), (0.02, 0.04, 0.03), (-0.03, 0.08, 0.06), (0.05, 0.12, 0.09), (-0.04, 0.16, 0.12)]


@functools.lru_cache(maxsize=None)
def fine_case():
    """dict: clouds (five lattices of 3600 points, one point per voxel at leaf 0.2, and a query of 700), maps (map 0: the five
    under five planar poses: 18 000 points), m (twelve matches: the query under several yaw guesses, the map's own frames), coarse / best / guesses
    (a made-up coarse table for the top-part tool's settings)"""
    clouds = [vc.lattice(3600, 310 + k) for k in range(5)]
    clouds.append(rc.moved(vc.lattice(700, 310), 1.0, 0.05, 0.05))
    maps = sc.Maps()
    g = maps.add([(k, sc.planar(*FINE_POSES[k])) for k in range(5)])
    m = sc.matches([(5, g, 0.5), (5, g, -1.0), (0, g, 0.3), (5, g, 2.0), (1, g, 0.0), (2, g, -0.4), (3, g, 0.2), (4, g, 0.0),
                    (5, g, 1.0), (5, g, 1.5), (0, g, -0.2), (5, g, 0.0)])
    coarse, best, guesses = vc.coarse_table(m, seed=29)
    return dict(clouds=clouds, maps=maps, m=m, coarse=coarse, best=best, guesses=guesses, n=18000)


# ---- coarse: 5 400 rows, ceil(sqrt) = 74 > 64 ----------------------------------------------------------------------------------
COARSE_STRIDE = 1000


@functools.lru_cache(maxsize=None)
def coarse_case():
    """dict: frames (six of 900 PointNormal rows and a moved copy of the first as the query), stride (above every count), maps
    (map 0: the six under planar and full 3-D poses: 5 400 rows), m"""
    frames = [cc.frame(900, 9800 + k) for k in range(6)]
    poses = [sc.IDENTITY, sc.planar(1.0, 0.3, -0.2), cc.pose3d(1.0, -1.0, 2.0, 0.2, 0.1, 0.05), sc.planar(-2.0, -0.4, 0.3),
             cc.pose3d(-1.5, 0.5, -1.0, -0.1, 0.3, -0.05), sc.planar(0.5, 0.1, 0.1)]
    frames.append(cc.move(frames[0], sc.planar(1.5, 0.2, -0.1)))
    maps = sc.Maps()
    g = maps.add([(k, poses[k]) for k in range(6)])
    m = sc.matches([(6, g, -1.0), (0, g, 0.5), (6, g, 3.0)])
    return dict(frames=frames, stride=COARSE_STRIDE, maps=maps, m=m, n=5400)


@functools.lru_cache(maxsize=None)
def top_case():
    """dict: clouds (six full labelled clouds of 3000 records and a moved copy of the first), pn (the front end's rows of each),
    maps (map 0: the six under planar poses), m"""
    clouds = [tc.wall_cloud(3000, 9900 + k) for k in range(6)]
    clouds.append(rc.moved(clouds[0], 1.0, 0.2, -0.1))
    maps = sc.Maps()
    g = maps.add([(k, sc.planar(0.3 * k, 0.05 * k, -0.04 * k)) for k in range(6)])
    m = sc.matches([(6, g, -1.0), (0, g, 0.5)])
    return dict(clouds=clouds, pn=tc.queries(clouds), maps=maps, m=m)


# ---- degenerate targets ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def degenerate_case():
    """(clouds, maps, m, names): fine targets on which the rule's branches end: no entries; every point non-finite; one
    point; all y equal; and a query wholly outside a plain target's bounds"""
    a = vc.lattice(300, 401)
    one = tc.records([[1.0, 2.0, 0.5]])
    line = tc.records(np.c_[np.arange(200) * 0.5, np.full(200, 3.0), np.zeros(200)])
    query = rc.moved(a, 1.0, 0.05, 0.05)
    near_line = tc.records(np.c_[np.arange(100) * 0.5 + 0.1, np.full(100, 3.1), np.zeros(100)])
    outside = query.copy()
    outside["x"] += F32(500.0)
    clouds = [a, one, line, query, near_line, outside]
    A, ONE, LINE, Q, NL, OUT = range(6)
    maps, names = sc.Maps(), {}
    names["none"] = maps.add([])
    names["non_finite"] = maps.add([(A, np.array([np.inf, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32))])
    names["one_point"] = maps.add([(ONE, sc.IDENTITY)])
    names["collinear"] = maps.add([(LINE, sc.IDENTITY)])
    names["plain"] = maps.add([(A, sc.IDENTITY)])
    m = sc.matches([(Q, names["none"], 0.0), (Q, names["non_finite"], 0.0), (ONE, names["one_point"], 0.0),
                    (Q, names["one_point"], 0.0), (NL, names["collinear"], 0.0), (OUT, names["plain"], 0.0),
                    (Q, names["plain"], -1.0)])
    return clouds, maps, m, names


@functools.lru_cache(maxsize=None)
def clump_case():
    """(frames, stride, maps, m): coarse targets: 4000 rows within 1 cm and one row 1 km away, so that one counter takes
    nearly every add and one cell holds nearly every row; a one-row map; a map without entries"""
    rng = np.random.default_rng(20270)
    clump = cc.frame(4001, 9850)
    clump[:4000, :2] = rng.uniform(0, 0.01, (4000, 2)).astype(F32)
    clump[4000, :3] = (1000.0, 0.0, 0.0)
    query = cc.frame(300, 9851)
    query[:, :2] = (query[:, :2] * F32(0.02)).astype(F32)       # within half a metre of the clump
    one = cc.frame(1, 9852)
    frames = [clump, query, one]
    maps = sc.Maps()
    g_clump, g_one, g_none = maps.add([(0, sc.IDENTITY)]), maps.add([(2, sc.IDENTITY)]), maps.add([])
    m = sc.matches([(1, g_clump, 0.0), (0, g_clump, 1.0), (1, g_one, 0.0), (2, g_one, 0.0), (1, g_none, 0.0)])
    return frames, 4096, maps, m


# ---- groups and bases -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def groups_case():
    """(clouds, maps, m, capacities): maps of 1, 300, 5 400 and 18 000 points and one that no match names (map 2), the matches
    in mixed order"""
    S = fine_case()
    clouds = list(S["clouds"]) + [tc.records([[0.5, 0.5, 0.5]]), vc.lattice(300, 402), vc.lattice(1800, 403)]
    ONE, SMALL, MID = 6, 7, 8
    maps = sc.Maps()
    g_one = maps.add([(ONE, sc.IDENTITY)])
    g_small = maps.add([(SMALL, sc.planar(1.0, 0.1, 0.1))])
    maps.add([(0, sc.IDENTITY), (1, sc.IDENTITY)])                                          # named by no match
    g_mid = maps.add([(MID, sc.planar(0.2 * k, 0.03 * k, 0.02 * k)) for k in range(3)])
    g_big = maps.add([(k, sc.planar(*FINE_POSES[k])) for k in range(5)])
    m = sc.matches([(5, g_big, 0.5), (SMALL, g_mid, 0.0), (ONE, g_one, 0.0), (5, g_small, 1.0), (5, g_mid, -0.5), (SMALL, g_small, -1.0),
                    (0, g_big, 0.2), (5, g_one, 0.0)])
    return clouds, maps, m, (1, 300, 5400, 18000)
