"""The checker and the seeded cases of scan-to-map coarse ICP against the thinned top part over the union of a map's moved full
clouds (test_submap_top_cpu.py, test_submap_top_gpu.py, test_submap_top_ground_truth_gpu.py,
test_cli_submap_top_union_gpu.py).  The checker is a composition of what exists and shares nothing with the device code:
submap_reg_cases.target (oracle_lib.transform_cloud per entry, concatenated in entry order) over the FULL clouds, the front
end's sequential top part, voxel grid and 2-D normals over that union (regfront_lib.top_part / .voxel / .normals; where the
voxel grid reports its "leaf too small" branch the positions are the top part itself), 12-float rows, the coarse stage's
sequential ICP per guess (icp_lib.run) and its choice (icp_lib.best).  Tests only."""
from __future__ import annotations

import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import icp_lib
import oracle_lib as orc
import regfront_lib as rf
import submap_coarse_cases as cc
import submap_pn_vox_cases as pv
import submap_reg_cases as sc
from bev_amd import ICP_NO_CORRESPONDENCES, ICP_RESULT_DTYPE, POINT_DTYPE

F32 = np.float32
RADIUS = 2.0                    # the front end's settings: what the tool hands to the call
LEAVES = (0.2, 0.5)
ODD_PAIR = (0.5, 0.3)           # (leaf, radius): the radius below the leaf
MAX_UNION = 1 << 24             # BEV_SUBMAP_TOP_MAX_UNION, restated
TILE = 4096                     # bevsubvox::kTile
GRID_CELLS = 64 * 64            # kIcpCells


def max_out(n: int) -> int:
    """bev_submap_top_part_max_out, restated: sum over 100 cells of round(0.2 n_c) <= n / 5 + 50"""
    return n // 5 + 51


def records(xyz, label=1) -> np.ndarray:
    """POINT_DTYPE records at the (n, 3) positions; label: one value or n of them; the other fields seeded by position"""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    out = np.zeros(len(xyz), POINT_DTYPE)
    out["x"], out["y"], out["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out["label"] = label
    out["intensity"] = (np.arange(len(xyz)) % 7).astype(F32)
    out["t"] = np.arange(len(xyz))
    return out


def union(clouds, entries) -> np.ndarray:
    return sc.target(clouds, entries)


def top(clouds, entries) -> np.ndarray:
    """(m, 4) float32: bev_top_part_flatten of the union"""
    return rf.top_part(union(clouds, entries))


def rows_of_top(t) -> np.ndarray:
    """what the cloud call writes with pn_leaf == 0: x y 0 0 | 0 0 0 0 | 0 0 0 0"""
    out = np.zeros((len(t), 12), F32)
    out[:, :3] = np.asarray(t, F32).reshape(-1, 4)[:, :3]
    return out


def thin(t, leaf, radius=RADIUS, viewpoint=(0.0, 0.0, 0.0)):
    """(target rows, overflow flag) of the top part t"""
    t = np.ascontiguousarray(np.asarray(t, F32).reshape(-1, 4))
    if leaf == 0:
        return rows_of_top(t), False
    v, info = rf.voxel(t, leaf, want_info=True)
    over = bool(info[0])
    if over:
        v = t
    return pv.point_normals(v, rf.normals(v, radius, viewpoint)), over


def target(clouds, entries, leaf, radius=RADIUS, viewpoint=(0.0, 0.0, 0.0)) -> np.ndarray:
    return thin(top(clouds, entries), leaf, radius, viewpoint)[0]


def all_targets(clouds, maps: sc.Maps, leaf, radius=RADIUS, viewpoint=(0.0, 0.0, 0.0)):
    """every map's target, what bev_submap_top_part_cloud_device_resident writes"""
    return [target(clouds, maps.entries(g), leaf, radius, viewpoint) for g in range(len(maps))]


def queries(clouds):
    """the front end's rows of every full cloud (leaf 0.2, radius 2, viewpoint 0): the d_pn frames"""
    return [rf.chain(c) for c in clouds]


def expected(pn, clouds, maps: sc.Maps, m, leaf, radius=RADIUS, viewpoint=(0.0, 0.0, 0.0), prm=None, threads=16, targets=None):
    """(results (n, 2) ICP_RESULT_DTYPE, best (n,) int32) of every match and guess; pn: the query rows per frame"""
    used = sorted({int(g) for g in m["match_idx"]})
    tgt = targets if targets is not None else {g: target(clouds, maps.entries(g), leaf, radius, viewpoint) for g in used}
    res = np.zeros((len(m), 2), ICP_RESULT_DTYPE)

    def one(k):
        i, g = divmod(k, 2)
        res[i, g] = icp_lib.run(pn[int(m["query_idx"][i])], tgt[int(m["match_idx"][i])],
                                icp_lib.tool_guess(float(m["angle_guess"][i]), g), prm)

    with ThreadPoolExecutor(max(1, threads)) as ex:
        list(ex.map(one, range(2 * len(m))))
    best = np.array([icp_lib.best(float(r[0]["fitness"]), float(r[1]["fitness"])) for r in res], np.int32).reshape(-1)
    return res, best


def union_cap(clouds, maps: sc.Maps, g) -> int:
    return sum(len(clouds[f]) for f, _ in maps.entries(g))


def map_bytes(c: int) -> int:
    """bevsubreg::map_top_union_bytes restated in plain numbers: a key per record of the union, the cells' table (100 cells of
    three words and two double words, four more words), the histograms (100 x 64 words), and a thinned PointNormal map of
    max_out(c) rows (136 bytes a row, its padded keys, the last voxel start, the 64 x 64 grid, two headers)"""
    r = max_out(c)
    slots = 1 << (r - 1).bit_length()
    return 8 * c + (100 * 28 + 16) + 100 * 64 * 4 + 136 * r + 8 * slots + 4 + 4 * (GRID_CELLS + 1) + 64


def group_count(clouds, maps: sc.Maps, used, cap: int):
    """the plan's greedy rule restated: (launch groups, maps alone above the cap)"""
    groups, cur, alone = 0, 0, 0
    for g in used:
        b = map_bytes(union_cap(clouds, maps, g))
        if cur and cur + b > cap:
            groups, cur = groups + 1, 0
        alone += b > cap
        cur += b
    return groups + (1 if cur else 0), alone


# ---- full labelled clouds: wall segments with height over ground records of label 0 -------------------------------------------
def wall_cloud(n: int, seed: int) -> np.ndarray:
    """n records in a seeded order: four fifths on five wall segments inside +-22 m, 0 .. 3 m high (label 1), one fifth ground
    at z near -1.7 (label 0, which the top part skips)"""
    rng = np.random.default_rng([int(seed), 0x77])
    ends = rng.uniform(-22, 22, (5, 2, 2))
    seg = rng.integers(0, 5, n)
    t = rng.uniform(0, 1, n)[:, None]
    xyz = np.zeros((n, 3), F32)
    xyz[:, :2] = ends[seg, 0] * (1 - t) + ends[seg, 1] * t + rng.normal(0, 0.02, (n, 2))
    xyz[:, 2] = rng.uniform(0, 3, n)
    ground = rng.uniform(0, 1, n) < 0.2
    xyz[ground, :2] = rng.uniform(-25, 25, (int(ground.sum()), 2))
    xyz[ground, 2] = rng.normal(-1.7, 0.02, int(ground.sum()))
    return records(xyz, np.where(ground, 0, 1))


LIST_SIZES = (1999, 2048, 2049, 3000)
LIST_SEED = 20266   # chosen on the CPU so that every problem of the list meets condition() at LEAVES and ODD_PAIR


@functools.lru_cache(maxsize=None)
def seeded_list():
    """dict: clouds (32: 16 wall clouds and a moved copy of each), pn (their front-end rows: the queries), maps (16: map i
    holds 1 .. 6 overlapping copies of cloud i; i % 3 == 0: planar poses; 1: planar poses and one entry 0.05 m lower; 2:
    +-2 degrees of roll and pitch), m (32 matches: cloud i and its moved copy against map i; two guesses each)"""
    rng = np.random.default_rng(LIST_SEED)
    sizes = list(LIST_SIZES) + rng.integers(1500, 3500, 12).tolist()
    H = len(sizes)
    base = [wall_cloud(n, 9100 + k) for k, n in enumerate(sizes)]
    near = [sc.planar(rng.uniform(-3, 3), *rng.uniform(-0.7, 0.7, 2)) for _ in range(H)]
    clouds = base + [orc.transform_cloud(base[i], near[i]) for i in range(H)]
    maps = sc.Maps()
    for i in range(H):
        entries = []
        for k in range(1 + i % 6):
            if i % 3 == 2:
                pose = pv.mild_pose(rng)
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
    return dict(clouds=clouds, pn=queries(clouds), maps=maps, m=sc.matches(rows), H=H)


@functools.lru_cache(maxsize=None)
def seeded_tops():
    S = seeded_list()
    return [top(S["clouds"], S["maps"].entries(g)) for g in range(len(S["maps"]))]


@functools.lru_cache(maxsize=None)
def seeded_targets(leaf, radius=RADIUS):
    return [thin(t, leaf, radius)[0] for t in seeded_tops()]


@functools.lru_cache(maxsize=None)
def seeded_expected(leaf, radius=RADIUS, threads=16):
    S = seeded_list()
    tgt = dict(enumerate(seeded_targets(leaf, radius)))
    return expected(S["pn"], S["clouds"], S["maps"], S["m"], leaf, radius, threads=threads, targets=tgt)


def condition(res) -> np.ndarray:
    """per PROBLEM (match, guess): it ends with a state other than NO_CORRESPONDENCES after two or more iterations"""
    return (res["state"] != ICP_NO_CORRESPONDENCES) & (res["iterations"] >= 2)


# ---- edge clouds: one cell each unless said otherwise; the cell of (0, 0) is cell 55 ----------------------------------------
def column(zs, x=0.0, y=0.0, label=1) -> np.ndarray:
    """records at (x + 0.01 i, y, zs[i]): distinct x, so a selected row names its record"""
    zs = np.asarray(zs, F32).reshape(-1)
    xyz = np.zeros((len(zs), 3), F32)
    xyz[:, 0] = F32(x) + F32(0.01) * np.arange(len(zs), dtype=F32)
    xyz[:, 1] = F32(y)
    xyz[:, 2] = zs
    return records(xyz, label)


def edge_cases():
    """name -> (clouds, maps): what the selection must get right, each small enough for the sequential checker"""
    rng = np.random.default_rng(771)
    I = sc.IDENTITY
    out = {}

    def one_map(clouds, entries):
        mp = sc.Maps()
        mp.add(entries)
        return clouds, mp

    # exactly 19 and 20 records; 20 reached only by the union of two entries of 10
    c19, c10a, c10b = column(rng.uniform(0, 3, 19)), column(rng.uniform(0, 3, 10)), column(rng.uniform(0, 3, 10), x=1.0)
    mp = sc.Maps()
    mp.add([(0, I)])
    mp.add([(1, I), (2, I)])
    mp.add([(1, I)])
    out["cell_counts_19_20"] = ([c19, c10a, c10b], mp)
    # round(0.2f * n): n = 22 -> 4 (4.4), n = 23 -> 5 (4.6), n = 27 -> 5 (5.4), n = 28 -> 6 (5.6)
    cl = [column(rng.uniform(0, 3, n)) for n in (22, 23, 27, 28)]
    mp = sc.Maps()
    for f in range(4):
        mp.add([(f, I)])
    out["rank_rounding"] = (cl, mp)
    # one frame of ONE z twice under one pose: every z is tied and the selection is the first entry's first records; the frame
    # and a copy at other x in both orders: the rows say which entry they came from; then the same with 40 distinct z, where
    # each z is tied once across the entries and the earlier entry's record comes first of the two
    a = column(np.full(40, 1.5))
    b = a.copy()
    b["x"] += F32(5.0)
    c = column(rng.uniform(0, 3, 40))
    d = c.copy()
    d["x"] += F32(5.0)
    mp = sc.Maps()
    mp.add([(0, I), (0, I)])
    mp.add([(0, I), (1, I)])
    mp.add([(1, I), (0, I)])
    mp.add([(2, I), (3, I)])
    mp.add([(3, I), (2, I)])
    out["tie_rule"] = ([a, b, c, d], mp)
    # the threshold rank inside a run of equal z: 30 records, rank 6, z: 4 high ones then 10 equal ones then lower
    zs = np.concatenate([[9, 8, 7, 6], np.full(10, 5.0), rng.uniform(0, 3, 16)]).astype(F32)
    out["threshold_in_tie_run"] = one_map([column(rng.permutation(zs))], [(0, I)])
    # degenerate digits: all one z; z differing in the last mantissa bit; -0 and +0; negative and mixed signs
    ulp = np.float32(1.5).view(np.uint32) + np.arange(25, dtype=np.uint32)
    cl = [column(np.full(50, 1.25)), column(rng.permutation(ulp).view(F32)),
          column(np.where(np.arange(30) % 2 == 0, F32(-0.0), F32(0.0))), column(-rng.uniform(0.5, 3, 30)),
          column(np.concatenate([-rng.uniform(0, 1e-3, 15), rng.uniform(0, 1e-3, 14), [0.0]]))]
    mp = sc.Maps()
    for f in range(len(cl)):
        mp.add([(f, I)])
    mp.add([(2, I), (2, sc.shift(dz=0.0))])
    out["degenerate_digits"] = (cl, mp)
    # poses: out of the grid and into it; x in [-110, -90) is cell row 0, x >= 90 is dropped; an overflowing matrix; a roll
    # that reverses which entry is higher
    base = column(rng.uniform(0, 3, 60))
    far = base.copy()
    far["x"] += F32(500.0)
    big = np.eye(3, 4, dtype=F32)
    big[0, 0], big[0, 3] = F32(3e38), F32(3.4e38)           # x = 0 stays finite and far off, every other x overflows
    roll = cc.pose3d(180.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    low = base.copy()
    low["z"] -= F32(4.0)
    low["x"] += F32(3.0)                                     # (so a row says which of the two it came from)
    mp = sc.Maps()
    mp.add([(0, sc.shift(dx=300.0))])                       # moved out: empty
    mp.add([(1, sc.shift(dx=-500.0))])                      # moved in
    mp.add([(0, sc.shift(dx=-105.0)), (0, sc.shift(dx=-95.0))])   # both cell row 0
    mp.add([(0, sc.shift(dx=89.0)), (0, sc.shift(dx=95.0))])      # the second dropped (and part of the first: x + 0.01 i)
    mp.add([(2, big.reshape(12)), (0, I)])                  # the first entry's x overflows: skipped
    mp.add([(0, I), (3, I)])                                # base above low
    mp.add([(0, roll), (3, roll)])                          # rolled over: low above base
    ten = column(np.full(30, 1.0) * 1e1)
    out["poses"] = ([base, far, ten, low], mp)
    # empty targets: an empty map; no kept cell; a frame no map names (frame 1)
    mp = sc.Maps()
    mp.add([])
    mp.add([(0, I)])
    out["empty_targets"] = ([column(rng.uniform(0, 3, 19)), column(rng.uniform(0, 3, 100))], mp)
    # labels: label 0 skipped, so the count that matters is the labelled one
    lab = column(rng.uniform(0, 3, 60), label=np.where(np.arange(60) % 3 == 0, 0, 1))
    nan = column(rng.uniform(0, 3, 40))
    nan["z"][::5] = np.nan
    nan["x"][1::7] = np.inf
    out["labels_and_non_finite"] = one_map([lab, nan], [(0, I), (1, I)])
    return out


def edge_expected(name):
    clouds, maps = edge_cases()[name]
    return [rows_of_top(top(clouds, maps.entries(g))) for g in range(len(maps))]
