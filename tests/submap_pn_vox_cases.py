"""The checker and the seeded cases of scan-to-map coarse ICP against maps thinned over their union (DESIGN.md §6q;
test_submap_pn_vox_cpu.py, test_submap_pn_vox_gpu.py, test_cli_submap_pn_leaf_gpu.py).  The checker is a composition of what
exists: submap_coarse_cases.target (the moved rows, concatenated in entry order), the front end's sequential voxel grid and
2-D normals (regfront_lib.voxel / .normals) over the positions of that union, 12-float rows of the two; where the voxel grid
reports its "leaf too small" branch the target is the concatenation itself.  Results are the coarse stage's sequential ICP per
guess (icp_lib.run) and its choice (icp_lib.best).  Tests only."""
from __future__ import annotations

import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import icp_lib
import regfront_lib as rf
import submap_coarse_cases as cc
import submap_reg_cases as sc
from bev_amd import ICP_NO_CORRESPONDENCES, ICP_RESULT_DTYPE

F32 = np.float32
GRID_CELLS = 64 * 64            # kIcpCells
TILE = 4096                     # bevsubvox::kTile
RADIUS = 2.0                    # the front end's settings: what the tool hands to the call
LEAVES = (0.2, 0.5, 1.0)
ODD_PAIRS = ((0.5, 0.3), (0.3, 2.0))   # (leaf, radius): the radius below the leaf; a ratio that is no integer


def point_normals(xyz, nrm) -> np.ndarray:
    """12-float PointNormal rows of (n, >= 3) positions and (n, 8) pcl::Normal records"""
    out = np.zeros((len(xyz), 12), F32)
    out[:, :3] = np.asarray(xyz, F32)[:, :3]
    out[:, 4:7] = nrm[:, :3]
    out[:, 8] = nrm[:, 4]
    return out


def thin(rows, leaf, radius=RADIUS, viewpoint=(0.0, 0.0, 0.0)):
    """(target rows, overflow flag) of the concatenation rows: leaf 0: the rows themselves"""
    rows = np.ascontiguousarray(np.asarray(rows, F32).reshape(-1, 12))
    if leaf == 0:
        return rows, False
    xyz = np.zeros((len(rows), 4), F32)
    xyz[:, :3] = rows[:, :3]
    v, info = rf.voxel(xyz, leaf, want_info=True)
    if info[0]:
        return rows, True
    return point_normals(v, rf.normals(v, radius, viewpoint)), False


def target(frames, entries, stride, leaf, radius=RADIUS, viewpoint=(0.0, 0.0, 0.0)) -> np.ndarray:
    return thin(cc.target(frames, entries, stride), leaf, radius, viewpoint)[0]


def expected(frames, maps: sc.Maps, m, leaf, radius=RADIUS, viewpoint=(0.0, 0.0, 0.0), prm=None, stride=None, threads=16,
             targets=None):
    """(results (n, 2) ICP_RESULT_DTYPE, best (n,) int32): the checker's results of every match and guess"""
    used = sorted({int(g) for g in m["match_idx"]})
    tgt = targets if targets is not None else {g: target(frames, maps.entries(g), stride, leaf, radius, viewpoint) for g in used}
    res = np.zeros((len(m), 2), ICP_RESULT_DTYPE)

    def one(k):
        i, g = divmod(k, 2)
        res[i, g] = icp_lib.run(frames[int(m["query_idx"][i])][:stride], tgt[int(m["match_idx"][i])],
                                icp_lib.tool_guess(float(m["angle_guess"][i]), g), prm)

    with ThreadPoolExecutor(max(1, threads)) as ex:
        list(ex.map(one, range(2 * len(m))))
    best = np.array([icp_lib.best(float(r[0]["fitness"]), float(r[1]["fitness"])) for r in res], np.int32).reshape(-1)
    return res, best


def all_targets(frames, maps: sc.Maps, stride, leaf, radius=RADIUS, viewpoint=(0.0, 0.0, 0.0)):
    """every map's target, what bev_submap_pn_cloud_device_resident writes"""
    return [target(frames, maps.entries(g), stride, leaf, radius, viewpoint) for g in range(len(maps))]


def group_count(maps: sc.Maps, m, stride: int, cap: int):
    """the plan's greedy rule restated for thinned PointNormal maps: (launch groups, maps alone above the cap)"""
    used = sorted({int(g) for g in m["match_idx"]})
    groups, cur, alone = 0, 0, 0
    for g in used:
        c = len(maps.entries(g)) * stride
        slots = 0 if c == 0 else 1 << (c - 1).bit_length()
        b = 136 * c + 8 * slots + 4 + 4 * (GRID_CELLS + 1) + 64
        if cur and cur + b > cap:
            groups, cur = groups + 1, 0
        alone += b > cap
        cur += b
    return groups + (1 if cur else 0), alone


# ---- flat frames: what the front end emits ------------------------------------------------------------------------------------
def flat_xyz(n: int, seed: int) -> np.ndarray:
    """n positions on five jittered wall segments at z = 0, in a seeded order"""
    rng = np.random.default_rng([int(seed), 0x51])
    ends = rng.uniform(-22, 22, (5, 2, 2))
    seg = rng.integers(0, 5, n)
    t = rng.uniform(0, 1, n)[:, None]
    out = np.zeros((n, 3), F32)
    out[:, :2] = ends[seg, 0] * (1 - t) + ends[seg, 1] * t + rng.normal(0, 0.02, (n, 2))
    return out


def flat_frame(n: int, seed: int) -> np.ndarray:
    """the PointNormal rows of flat_xyz under the front end's normals (radius 2, viewpoint 0): z = 0, nz = 0"""
    xyz = flat_xyz(n, seed)
    return point_normals(xyz, rf.normals(xyz, RADIUS))


def mild_pose(rng) -> np.ndarray:
    """+-2 degrees of roll and pitch, +-1 of yaw, +-0.3 m: a union of many z layers"""
    return cc.pose3d(rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-1, 1), *rng.uniform(-0.3, 0.3, 3))


LIST_SIZES = (63, 64, 65, 255, 256, 257, 511, 512)
LIST_STRIDE = 500   # the frames of 511 and 512 rows stay above it


@functools.lru_cache(maxsize=None)
def seeded_list():
    """dict: frames (40: 20 flat frames and a moved copy of each), stride, maps (20: map i holds 1 .. 6 overlapping copies of
    frame i; i % 3 == 0: planar poses, one z layer; 1: planar poses and one entry 0.05 m lower, two layers; 2: mild 3-D poses,
    many layers), m (40 matches: frame i and its moved copy against map i; two guesses each: 80 problems)"""
    rng = np.random.default_rng(20263)
    sizes = list(LIST_SIZES) + rng.integers(100, 513, 12).tolist()
    H = len(sizes)
    base = [flat_frame(n, 8100 + k) for k, n in enumerate(sizes)]
    near = [sc.planar(rng.uniform(-3, 3), *rng.uniform(-0.7, 0.7, 2)) for _ in range(H)]
    frames = base + [cc.move(base[i], near[i]) for i in range(H)]
    maps = sc.Maps()
    for i in range(H):
        entries = []
        for k in range(1 + i % 6):
            if i % 3 == 2:
                pose = mild_pose(rng)
            else:
                pose = sc.planar(rng.uniform(-1, 1), *rng.uniform(-0.3, 0.3, 2))
                if i % 3 == 1 and k == 0:
                    pose[11] = F32(-0.05)
            entries.append((i if k % 2 == 0 else H + i, pose))
        maps.add(entries)
    rows = []
    for i in range(H):
        rows.append((H + i, i, rng.uniform(-3, 3)))
        rows.append((i, i, rng.uniform(-3, 3)))
    return dict(frames=frames, stride=LIST_STRIDE, maps=maps, m=sc.matches(rows), H=H)


@functools.lru_cache(maxsize=None)
def seeded_targets(leaf, radius=RADIUS):
    S = seeded_list()
    return all_targets(S["frames"], S["maps"], S["stride"], leaf, radius)


@functools.lru_cache(maxsize=None)
def seeded_expected(leaf, radius=RADIUS, threads=16):
    S = seeded_list()
    tgt = dict(enumerate(seeded_targets(leaf, radius)))
    return expected(S["frames"], S["maps"], S["m"], leaf, radius, stride=S["stride"], threads=threads, targets=tgt)


def condition_share(res) -> float:
    """the share of PROBLEMS (match, guess) that end with a state other than NO_CORRESPONDENCES after two or more iterations"""
    ok = (res["state"] != ICP_NO_CORRESPONDENCES) & (res["iterations"] >= 2)
    return float(ok.mean())


def z_layers(frames, maps: sc.Maps, stride, leaf) -> list:
    """div_z of every map's union grid"""
    out = []
    for g in range(len(maps)):
        c = cc.target(frames, maps.entries(g), stride)
        xyz = np.zeros((len(c), 4), F32)
        xyz[:, :3] = c[:, :3]
        out.append(int(rf.voxel(xyz, leaf, want_info=True)[1][3]))
    return out


# ---- the entry-order pair -------------------------------------------------------------------------------------------------------
ORDER_LEAF = 1.0
ORDER_XS = (F32(0.1), F32(0.7), F32(0.70000005))   # three float32 in one voxel of 1 m: (a + b) + c != (b + c) + a ... see below


def order_pair():
    """(frames, maps, matches): three frames of one point each at x = ORDER_XS, y = 0.5, z = 0, besides a shared frame of walls;
    map 0 holds the single points in the order 0 1 2, map 1 in the order 2 1 0, both then the walls: the same union, but the
    voxel of the three points is summed in another order and its centroid differs in the last bit (the CPU test asserts that
    the float32 sums differ before this is used on the GPU)."""
    walls = flat_frame(300, 8300)
    walls[:, 0] += F32(5.0)         # clear of the three points' voxel
    pts = []
    for x in ORDER_XS:
        p = np.zeros((1, 12), F32)
        p[0, 0], p[0, 1] = x, F32(0.5)
        pts.append(p)
    frames = pts + [walls, cc.move(walls, sc.planar(1.0, 0.2, 0.1))]
    maps = sc.Maps()
    maps.add([(0, sc.IDENTITY), (1, sc.IDENTITY), (2, sc.IDENTITY), (3, sc.IDENTITY)])
    maps.add([(2, sc.IDENTITY), (1, sc.IDENTITY), (0, sc.IDENTITY), (3, sc.IDENTITY)])
    return frames, maps, sc.matches([(4, 0, 1.0), (4, 1, 1.0)])


def order_sums():
    """the two float32 sums of ORDER_XS in the two entry orders"""
    a, b, c = ORDER_XS
    return F32(F32(a + b) + c), F32(F32(c + b) + a)
