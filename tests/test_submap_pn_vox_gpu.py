"""GPU: scan-to-map coarse ICP against maps thinned over their union, normals recomputed
(bev_submap_coarse_voxel_registration_device_resident, bev_submap_pn_cloud_device_resident).  Every comparison is
of bytes: whole bev_icp_result_t records, the choice between the guesses, and whole PointNormal rows and counts of the maps,
against the checker composition of submap_pn_vox_cases.py (the moved rows concatenated, the front end's sequential voxel grid
and 2-D normals over the union, the coarse stage's sequential ICP per guess):

  a. the seeded list at leaves 0.2, 0.5, 1.0 (radius 2), at a radius below the leaf and at a ratio that is no integer: results,
     best, every map's rows and count; the same under a forced group cap;
  b. pn_leaf = 0 on the coarse stage's own seeded list equals the old entry point's bytes; the cloud call writes concat(g);
  c. capacities of 0, 1, 4095, 4096, 4097 and 8193 rows, a map of 257 entries of tiny frames, all points in one voxel, every
     point in a voxel of its own (thinned maps of 255, 256, 257 and 1500 points), neighbour counts of exactly 1, 2 and 3, a
     window that covers neither the rows nor the layers of the union's grid, normals workgroups that cross a layer, candidate
     ranges of several staged chunks;
  d. the overflow branch (pn_leaf = 1e-6 on a map 40 m wide) equals the pn_leaf = 0 call;
  e. the entry-order pair; entry bookkeeping; a viewpoint off the origin; non-finite positions and an overflowing matrix;
  f. front end, this call and the fine stage chained without a synchronisation; calls of different sizes with the pair call
     between them;
  g. every refused argument, the outputs untouched.
"""
import ctypes as C
import os

import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import icp_lib
import reg_cases as rc
import regfront_lib as rf
import submap_coarse_cases as cc
import submap_pn_vox_cases as pv
import submap_reg_cases as sc
from bev_amd import ICP_RESULT_DTYPE
from submap_reg_gpu_lib import F32, INVALID, OK, R, THREADS, TOO_LARGE, _ctx, _dev, _same

pytestmark = pytest.mark.gpu
GROUP_CAP = 150000  # bytes
NOCORR = bev_amd.ICP_NO_CORRESPONDENCES


@pytest.fixture(scope="module", autouse=True)
def _checkers():
    icp_lib.build()
    fl.build()
    rf.build()


def _check(name, got, exp):
    (gr, gb), (er, eb) = got, exp
    gr, er = np.asarray(gr).reshape(-1), np.asarray(er).reshape(-1)
    assert len(gr) == len(er), f"{name}: {len(gr)} records, expected {len(er)}"
    bad = [k for k in range(len(er)) if not _same(gr[k], er[k])]
    assert not bad, f"{name}: {len(bad)} of {len(er)} results differ, first match {bad[0] // 2} guess {bad[0] % 2}: {gr[bad[0]]} != {er[bad[0]]}"
    assert np.array_equal(np.asarray(gb), np.asarray(eb)), f"{name}: best differs at {np.flatnonzero(np.asarray(gb) != np.asarray(eb))[:5]}"


def _check_clouds(name, got, exp):
    rows, counts = got
    assert counts.tolist() == [len(e) for e in exp], f"{name}: counts {counts.tolist()} != {[len(e) for e in exp]}"
    for g, e in enumerate(exp):
        if not _same(rows[g], e):
            bad = np.flatnonzero((rows[g].view(np.uint32) != e.view(np.uint32)).any(axis=1))
            raise AssertionError(f"{name}: map {g}: {len(bad)} of {len(e)} rows differ, first {bad[0]}: {rows[g][bad[0]]} != {e[bad[0]]}")


def _counts(frames):
    return np.array([len(f) for f in frames], np.uint32)


def _read(d_res, d_best, n):
    return d_res.cpu().numpy().view(ICP_RESULT_DTYPE).reshape(-1, 2)[:n], d_best.cpu().numpy().view(np.int32)[:n]


def _upload(frames, stride):
    return _dev(rc.strided(frames, stride)), _dev(_counts(frames))


def _outputs(n, fill=0):
    import torch

    dev = torch.device("cuda:0")
    return (torch.full((max(n, 1) * 2 * R,), fill, dtype=torch.uint8, device=dev),
            torch.full((max(n, 1) * 4,), fill, dtype=torch.uint8, device=dev))


def _call(ctx, frames, stride, maps, m, leaf, radius=pv.RADIUS, vp=None, prm=None, d=None):
    import torch

    d_pn, d_cnt = d if d is not None else _upload(frames, stride)
    d_res, d_best = _outputs(len(m))
    torch.cuda.synchronize()
    ctx.submap_coarse_voxel_registration_device(len(frames), d_pn.data_ptr(), stride, d_cnt.data_ptr(), *maps.arrays(), m,
                                                d_res.data_ptr(), d_best.data_ptr(), leaf, radius, vp, prm)
    ctx.synchronize()
    return _read(d_res, d_best, len(m))


def _clouds(ctx, frames, stride, maps, leaf, radius=pv.RADIUS, vp=None, d=None):
    """every map's rows and count through the cloud call; rows past a count must stay as they were"""
    import torch

    d_pn, d_cnt = d if d is not None else _upload(frames, stride)
    G = len(maps)
    cap = max(1, max(len(maps.entries(g)) for g in range(G)) * stride)
    dev = torch.device("cuda:0")
    d_out = torch.full((G * cap * 48,), 0xCD, dtype=torch.uint8, device=dev)
    d_n = torch.full((G * 4,), 0xCD, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.submap_pn_cloud_device(len(frames), d_pn.data_ptr(), stride, d_cnt.data_ptr(), *maps.arrays(), leaf, cap, d_out.data_ptr(),
                               d_n.data_ptr(), radius, vp)
    ctx.synchronize()
    out = d_out.cpu().numpy().reshape(G, cap, 48)
    n = d_n.cpu().numpy().view(np.uint32)
    assert (n <= cap).all(), n
    for g in range(G):
        assert (out[g, n[g]:] == 0xCD).all(), f"map {g}: rows past the count were written"
    return [np.ascontiguousarray(out[g, : n[g]]).view(F32).reshape(-1, 12) for g in range(G)], n


def _run_and_check(name, frames, stride, maps, m, leaf, radius=pv.RADIUS, vp=None, prm=None, clouds=True):
    """the registration call and the cloud call against the checker; returns (results, targets)"""
    view = vp if vp is not None else (0.0, 0.0, 0.0)
    tgt = pv.all_targets(frames, maps, stride, leaf, radius, view)
    exp = pv.expected(frames, maps, m, leaf, radius, view, prm, stride, THREADS, targets=dict(enumerate(tgt)))
    ctx = _ctx()
    try:
        d = _upload(frames, stride)
        got = _call(ctx, frames, stride, maps, m, leaf, radius, vp, prm, d=d)
        got_clouds = _clouds(ctx, frames, stride, maps, leaf, radius, vp, d=d) if clouds else None
    finally:
        ctx.close()
    print(f"{name}: thinned {[len(t) for t in tgt]} states {exp[0]['state'].tolist()} iterations {exp[0]['iterations'].tolist()}")
    if clouds:
        _check_clouds(name, got_clouds, tgt)
    _check(name, got, exp)
    return exp, tgt


def _bare(xyz) -> np.ndarray:
    """PointNormal rows of positions alone: a thinned map reads nothing else of its entries, a query nothing else at all"""
    out = np.zeros((len(xyz), 12), F32)
    out[:, :3] = np.asarray(xyz, F32)[:, :3]
    return out


# ---- a. the seeded list ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf,radius", [(l, pv.RADIUS) for l in pv.LEAVES] + list(pv.ODD_PAIRS))
def test_the_seeded_list_equals_the_checker(leaf, radius):
    S = pv.seeded_list()
    exp, tgt = pv.seeded_expected(leaf, radius, THREADS), pv.seeded_targets(leaf, radius)
    share = pv.condition_share(exp[0])
    print(f"leaf {leaf} radius {radius}: {share:.3f} of {exp[0].size} problems keep correspondences for two iterations or more; "
          f"{sum(len(t) for t in tgt)} thinned rows, {sum(int(np.isnan(t[:, 4]).sum()) for t in tgt)} NaN normals")
    if radius == pv.RADIUS:
        assert share >= 0.9                                  # the condition on the inputs, on the checker's results alone
    assert (_counts(S["frames"]) > S["stride"]).any()
    ctx = _ctx()
    try:
        d = _upload(S["frames"], S["stride"])
        got = _call(ctx, S["frames"], S["stride"], S["maps"], S["m"], leaf, radius, d=d)
        got_clouds = _clouds(ctx, S["frames"], S["stride"], S["maps"], leaf, radius, d=d)
    finally:
        ctx.close()
    _check_clouds(f"leaf {leaf}: the maps", got_clouds, tgt)
    _check(f"leaf {leaf}: the results", got, exp)


def test_a_forced_group_cap_gives_the_same_results():
    S = pv.seeded_list()
    leaf = 0.2
    n_groups, alone = pv.group_count(S["maps"], S["m"], S["stride"], GROUP_CAP)
    assert n_groups >= 10 and alone >= 1                    # many groups, and maps alone above the cap
    saved = os.environ.get("BEV_SUBMAP_REG_GROUP")
    launches = {}
    try:
        for cap in (None, str(GROUP_CAP)):
            if cap is None:
                os.environ.pop("BEV_SUBMAP_REG_GROUP", None)
            else:
                os.environ["BEV_SUBMAP_REG_GROUP"] = cap
            ctx = _ctx()
            try:
                ctx.profile_enable(True)
                got = _call(ctx, S["frames"], S["stride"], S["maps"], S["m"], leaf)
                launches[cap] = {k["name"]: k["launches"] for k in ctx.profile_get()}
                got_clouds = _clouds(ctx, S["frames"], S["stride"], S["maps"], leaf)
            finally:
                ctx.close()
            _check(f"cap {cap}", got, pv.seeded_expected(leaf, pv.RADIUS, THREADS))
            _check_clouds(f"cap {cap}", got_clouds, pv.seeded_targets(leaf))
    finally:
        if saved is None:
            os.environ.pop("BEV_SUBMAP_REG_GROUP", None)
        else:
            os.environ["BEV_SUBMAP_REG_GROUP"] = saved
    assert launches[None]["k_submap_pn_normals"] == 1 and launches[None]["k_submap_pn_move"] == 1, launches
    assert "k_submap_pn_target" not in launches[None], launches
    for k in ("k_submap_pn_move", "k_submap_pn_keys", "k_submap_pn_finish", "k_submap_pn_normals", "k_submap_pn_grid"):
        assert launches[str(GROUP_CAP)][k] == n_groups, (k, launches)


# ---- b. pn_leaf = 0 ----------------------------------------------------------------------------------------------------------------
def test_leaf_zero_is_the_old_entry_point_byte_for_byte_and_the_cloud_call_writes_the_concatenation():
    import torch

    S = cc.seeded_list()
    frames, stride, maps, m = S["frames"], S["stride"], S["maps"], S["m"]
    ctx = _ctx()
    try:
        d = _upload(frames, stride)
        new = _call(ctx, frames, stride, maps, m, 0.0, radius=float("nan"), d=d)   # radius and viewpoint are not read
        d_res, d_best = _outputs(len(m))
        torch.cuda.synchronize()
        ctx.submap_coarse_registration_device(len(frames), d[0].data_ptr(), stride, d[1].data_ptr(), *maps.arrays(), m,
                                              d_res.data_ptr(), d_best.data_ptr())
        ctx.synchronize()
        old = _read(d_res, d_best, len(m))
        got_clouds = _clouds(ctx, frames, stride, maps, 0.0, radius=-1.0, d=d)
    finally:
        ctx.close()
    _check("pn_leaf 0 against the old entry point", new, old)
    _check("pn_leaf 0 against the checker", new, cc.seeded_expected(THREADS))
    _check_clouds("concat", got_clouds, [cc.target(frames, maps.entries(g), stride) for g in range(len(maps))])


# ---- c. shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 4095, 4096, 4097, 8193])
def test_capacities_around_the_sort_tile_equal_the_checker(cap):
    xyz = pv.flat_xyz(cap, 9000 + cap)
    frames = [_bare(xyz), cc.move(_bare(xyz[: min(cap, 300)]), sc.planar(1.0, 0.2, -0.1))]
    maps = sc.Maps()
    g_none = maps.add([])                                    # capacity 0
    g_one = maps.add([(0, cc.pose3d(0.5, -0.5, 1.0, 0.1, 0.1, 0.05))])
    m = sc.matches([(1, g_one, 1.0), (1, g_none, 0.0), (0, g_one, 0.0)])
    exp, tgt = _run_and_check(f"capacity {cap}", frames, cap, maps, m, 0.2)
    assert len(tgt[g_none]) == 0 and 0 < len(tgt[g_one]) <= cap
    assert (exp[0]["state"][1] == NOCORR).all()
    assert cap < 100 or (exp[0]["state"][0] != NOCORR).all()


def test_a_map_of_257_entries_of_tiny_frames_equals_the_checker():
    rng = np.random.default_rng(9300)
    body = _bare(pv.flat_xyz(600, 9301))
    tiny = [np.ascontiguousarray(body[k: k + n]) for k, n in zip(range(0, 600, 2), rng.integers(0, 4, 300).tolist())]
    frames = tiny + [cc.move(body[:200], sc.planar(1.0, 0.1, 0.1))]
    maps = sc.Maps()
    g = maps.add([(k, sc.shift(0.01 * (k % 7), 0, 0.03 * (k % 5))) for k in range(257)])   # the scan's second round: entry 256
    g2 = maps.add([(k, sc.IDENTITY) for k in range(299, 40, -1)])
    m = sc.matches([(300, g, 1.0), (300, g2, 1.0), (5, g, 0.0)])
    assert len(maps.entries(g)) == 257 and len(cc.target(frames, maps.entries(g), 4)) > 256 and len(tiny[256]) > 0
    exp, _ = _run_and_check("257 entries", frames, 4, maps, m, 0.5)
    assert (exp[0]["state"][:2, 0] != NOCORR).all()


def _lattice(n, seed):
    """n points 0.5 m apart along a bent line, jittered by less than 0.1: at leaf 0.2 every point has a voxel of its own"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    xyz = np.zeros((n, 3), F32)
    xyz[:, 0] = (k % 100) * 0.5 + 0.1 + rng.uniform(0, 0.05, n)
    xyz[:, 1] = (k // 100) * 0.5 + 0.1 + rng.uniform(0, 0.05, n)
    return xyz[rng.permutation(n)]


def test_one_voxel_and_one_point_per_voxel_equal_the_checker():
    sizes = (255, 256, 257, 1500)
    lat = [_bare(_lattice(n, 9400 + n)) for n in sizes]
    blob = _bare(np.random.default_rng(9401).uniform(0.0, 0.19, (300, 3)))       # all in the voxel [0, 0.2)^3
    frames = lat + [blob, cc.move(lat[3][:400], sc.planar(0.5, 0.1, 0.1))]
    Q = len(frames) - 1
    maps = sc.Maps()
    gs = [maps.add([(k, sc.IDENTITY)]) for k in range(4)]
    g_halves = maps.add([(3, sc.IDENTITY), (3, sc.shift(0.0, 0.0, 0.0))])        # every voxel holds two equal points
    g_blob = maps.add([(4, sc.IDENTITY)])
    m = sc.matches([(Q, g, 0.5) for g in gs] + [(Q, g_halves, 0.5), (Q, g_blob, 0.0)])
    exp, tgt = _run_and_check("voxels", frames, 1500, maps, m, 0.2)
    assert [len(tgt[g]) for g in gs] == list(sizes) and len(tgt[g_halves]) == 1500 and len(tgt[g_blob]) == 1
    assert np.isnan(tgt[g_blob][0, 4:7]).all()                # a lone voxel: |N| = 1
    assert (exp[0]["state"][:5, 0] != NOCORR).all()


def test_neighbour_counts_of_exactly_one_two_and_three_equal_the_checker():
    groups = [[(0, 0)], [(20, 0), (21, 0.5)], [(40, 0), (41, 0.3), (40.5, 1.0)], [(60, 0), (61, 0), (60, 1), (61, 1.2)]]
    xyz = np.array([(x, y, 0.0) for grp in groups for x, y in grp], F32)
    walls = _bare(pv.flat_xyz(300, 9500) + np.array([0, 60, 0], F32))
    frames = [_bare(xyz), walls, cc.move(walls, sc.planar(1.0, 0.2, 0.1))]
    maps = sc.Maps()
    g = maps.add([(0, sc.IDENTITY)])
    g_both = maps.add([(1, sc.IDENTITY), (0, cc.pose3d(1.0, 1.0, 0.0, 0.0, 0.0, 0.0))])
    m = sc.matches([(2, g_both, 1.0), (0, g, 0.0)])
    exp, tgt = _run_and_check("neighbour counts", frames, 300, maps, m, 0.2)
    nn = rf.normals(tgt[g][:, :4].copy(), pv.RADIUS, want_nn=True)[1]
    assert sorted(nn.tolist()) == [1, 2, 2, 3, 3, 3, 4, 4, 4, 4]
    assert exp[0]["state"][0, 0] != NOCORR


def test_a_window_smaller_than_the_grid_in_rows_and_layers_equals_the_checker():
    leaf, radius = 0.1, 0.25                                  # the window is ceil(2.5) + 2 = 5 rows and layers each way
    base = _bare(pv.flat_xyz(900, 9600))
    frames = [base, cc.move(base, sc.planar(1.0, 0.2, 0.1))]
    maps = sc.Maps()
    g = maps.add([(0, cc.pose3d(2.0, -2.0, 0.5, 0.1, 0.0, 0.2)), (0, cc.pose3d(-2.0, 1.5, -0.5, 0.0, 0.1, -0.2)), (1, sc.IDENTITY)])
    m = sc.matches([(1, g, 1.0), (0, g, 0.0)])
    c = cc.target(frames, maps.entries(g), 900)
    info = rf.voxel(np.c_[c[:, :3], np.zeros(len(c), F32)], leaf, want_info=True)[1]
    assert info[0] == 0 and info[2] > 11 and info[3] > 11, info  # more rows and layers than the window: it is clipped inside
    exp, tgt = _run_and_check("window", frames, 900, maps, m, leaf, radius)
    lo, hi = tgt[g][:, 2].argmin(), tgt[g][:, 2].argmax()     # queries in the first and the last layer, and rows
    assert tgt[g][lo, 2] < -0.5 and tgt[g][hi, 2] > 0.5


def test_workgroups_that_cross_a_layer_and_ranges_longer_than_a_staged_chunk_equal_the_checker():
    """the normals workgroup's union window: two row ranges per layer where its 256 queries cross from one layer into the next,
    and a candidate range of more than 1024 points (several staged chunks)"""
    leaf, radius, win = 0.2, 0.5, 5                           # ceil(2.5) + 2
    base = _bare(pv.flat_xyz(2500, 9650))
    blob = _bare(np.c_[np.random.default_rng(9651).uniform(0.0, 5.0, (5000, 2)), np.zeros(5000)])
    frames = [base, cc.move(base[:400], sc.planar(1.0, 0.2, 0.1)), blob, cc.move(blob[:400], sc.planar(1.0, 0.05, 0.05))]
    maps = sc.Maps()
    g = maps.add([(0, sc.IDENTITY), (0, sc.shift(0.05, 0.05, -0.25))])
    g_blob = maps.add([(2, sc.IDENTITY)])
    m = sc.matches([(1, g, 1.0), (3, g_blob, 1.0)])
    exp, tgt = _run_and_check("two layers", frames, 5000, maps, m, leaf, radius)
    t = tgt[g]
    z = t[:, 2]
    assert set(np.unique(z).tolist()) == {-0.25, 0.0} and (np.diff(z) >= 0).all()      # two layers, the lower one first
    cross = [b for b in range(0, len(t), 256) if z[b] != z[min(b + 255, len(t) - 1)]]
    assert len(cross) == 1 and cross[0] > 0
    b = cross[0]
    assert t[b, 1] - t[min(b + 255, len(t) - 1), 1] > (2 * win + 3) * leaf               # the two row ranges do not meet
    # the blob at leaf 0.1 and radius 2: a window of 22 rows each way covers at least 45 of its 50 rows, more than a staged chunk
    exp2, tgt2 = _run_and_check("chunks", frames, 5000, maps, m, 0.1, 2.0)
    rows = np.floor(tgt2[g_blob][:, 1] / 0.1)
    assert len(tgt2[g_blob]) > 1500 and np.bincount(rows.astype(int), minlength=50)[:50].min() > 25    # 45 rows: above 1024 points
    assert exp[0]["state"][0, 0] != NOCORR and exp2[0]["state"][1, 0] != NOCORR


# ---- d. the overflow branch ----------------------------------------------------------------------------------------------------
def test_a_leaf_too_small_keeps_the_concatenation_and_equals_leaf_zero():
    a = pv.flat_frame(400, 9700)
    frames = [a, cc.move(a, sc.planar(2.0, 0.3, 0.1))]
    maps = sc.Maps()
    g = maps.add([(0, sc.IDENTITY), (0, cc.pose3d(1.0, -1.0, 0.5, 0.1, 0.0, 0.05))])
    m = sc.matches([(1, g, 2.0), (0, g, 0.0)])
    assert np.ptp(a[:, 0]) > 30 and pv.thin(cc.target(frames, maps.entries(g), 400), 1e-6)[1]   # 40 m / 1e-6: above INT32_MAX voxels
    exp, tgt = _run_and_check("overflow", frames, 400, maps, m, 1e-6)
    assert len(tgt[g]) == 800 and (tgt[g][400:, 6] != 0).any()   # the moved normals, nz included
    ctx = _ctx()
    try:
        zero = _call(ctx, frames, 400, maps, m, 0.0)
    finally:
        ctx.close()
    _check("overflow against pn_leaf 0", zero, exp)
    assert (exp[0]["state"][:, 0] != NOCORR).all()


# ---- e. order, bookkeeping, values ------------------------------------------------------------------------------------------------
def test_the_entry_order_pair_follows_the_order_of_the_sums():
    frames, maps, m = pv.order_pair()
    exp, tgt = _run_and_check("entry order", frames, 300, maps, m, pv.ORDER_LEAF)
    assert len(tgt[0]) == len(tgt[1]) and not _same(tgt[0], tgt[1])


def test_entry_bookkeeping_equals_the_checker():
    a, b, c = pv.flat_frame(500, 9801), pv.flat_frame(400, 9802), pv.flat_frame(300, 9803)
    zero = np.zeros((0, 12), F32)
    only_query, only_entry, unnamed = cc.move(a, sc.planar(3.0, 0.2, 0.1)), pv.flat_frame(350, 9804), pv.flat_frame(100, 9805)
    frames = [a, b, c, zero, only_query, only_entry, unnamed, zero.copy()]
    A, B, Cc, ZERO, OQ, OE, UN, ZERO2 = range(8)
    stride = 450                                             # a's count stays above it
    maps = sc.Maps()
    g_none = maps.add([])
    g_gaps = maps.add([(ZERO, sc.IDENTITY), (A, sc.IDENTITY), (ZERO2, sc.planar(1, 0, 0)), (ZERO, cc.pose3d(1, 1, 5, 1, 1, 0)), (B, sc.planar(2, 0.1, 0))])
    g_twice = maps.add([(A, sc.IDENTITY), (A, cc.pose3d(0.3, -0.2, 0.5, 0.05, 0.0, 0.02)), (A, sc.IDENTITY)])
    g_unused = maps.add([(B, sc.IDENTITY), (UN, sc.IDENTITY)])   # named by no match: costs the registration call nothing
    g_only_empty = maps.add([(ZERO, sc.IDENTITY), (ZERO2, sc.IDENTITY)])
    g_shared = maps.add([(A, sc.planar(1, 0, 0)), (OE, sc.IDENTITY), (Cc, cc.pose3d(-1, 0.5, -1, 0, 0.1, 0))])
    g_a_again = maps.add([(Cc, sc.IDENTITY), (A, sc.planar(-1, 0.1, 0.1))])
    rows = [(OQ, g_gaps, 3.0), (OQ, g_none, 0.0), (OQ, g_twice, 2.0), (Cc, g_only_empty, 0.0), (OQ, g_shared, 3.0),
            (B, g_shared, 0.0), (Cc, g_shared, 1.0), (OQ, g_shared, -3.0), (A, g_gaps, 0.0), (ZERO, g_twice, 0.0), (OQ, g_a_again, 3.0)]
    m = sc.matches(rows)
    assert g_unused not in m["match_idx"] and len(a) > stride
    exp, _ = _run_and_check("bookkeeping", frames, stride, maps, m, 0.5)
    st = exp[0]["state"]
    assert (st[[1, 3, 9]] == NOCORR).all() and (st[[0, 4]] != NOCORR).all()


def test_a_viewpoint_off_the_origin_equals_the_checker():
    a = pv.flat_frame(400, 9901)
    frames = [a, cc.move(a, sc.planar(2.0, 0.3, 0.1))]
    maps = sc.Maps()
    g = maps.add([(0, sc.IDENTITY), (1, sc.planar(-1.0, 0.1, 0.0))])
    m = sc.matches([(1, g, 2.0)])
    vp = (15.0, -8.0, 3.0)
    _, tgt = _run_and_check("viewpoint", frames, 400, maps, m, 0.5, vp=vp)
    assert not _same(tgt[g], pv.target(frames, maps.entries(g), 400, 0.5))   # it flips some normals the other way


def test_non_finite_positions_and_an_overflowing_matrix_equal_the_checker():
    a, b = pv.flat_frame(500, 9951), pv.flat_frame(400, 9952)
    bad = b.copy()
    bad[::7, 0] = np.nan
    bad[1::11, 1] = np.inf
    bad[2::13, 2] = -np.inf
    frames = [a, b, bad, cc.move(a, sc.planar(2.0, 0.2, -0.1)), cc.move(b, sc.planar(-2.0, 0.1, 0.1))]
    A, B, BAD, QA, QB = range(5)
    overflow = np.array([1e38, 0, 0, 0, 0, 1e38, 0, 0, 0, 0, 1, 0], F32)
    nan_mat = np.array([1, 0, 0, np.nan, 0, 1, 0, 0, 0, 0, 1, 0], F32)
    huge = np.array([1, 0, 0, 3e38, 0, 1, 0, 0, 0, 0, 1, 0], F32)
    maps = sc.Maps()
    g_bad = maps.add([(BAD, sc.planar(1, 0.1, -0.1)), (A, sc.IDENTITY), (BAD, sc.IDENTITY)])
    g_inf = maps.add([(A, overflow), (B, sc.IDENTITY)])
    g_all_nan = maps.add([(A, nan_mat), (B, nan_mat)])       # no finite position: an empty target
    g_far = maps.add([(A, huge), (B, sc.IDENTITY)])          # finite but 3e38 away: the grid overflows
    m = sc.matches([(QB, g_bad, -2.0), (QB, g_inf, -2.0), (QA, g_all_nan, 0.0), (QB, g_far, -2.0), (BAD, g_bad, 0.0)])
    exp, tgt = _run_and_check("values", frames, 512, maps, m, 0.5)
    assert len(tgt[g_all_nan]) == 0 and np.isfinite(tgt[g_bad][:, :3]).all()
    assert (exp[0]["state"][2] == NOCORR).all() and (exp[0]["state"][[0, 1], 0] != NOCORR).all()


# ---- f. chains and sequences ------------------------------------------------------------------------------------------------------
def test_front_end_thinned_coarse_and_fine_stage_chained_without_a_synchronisation():
    import torch

    base = [rc.scene(n, 9600 + k) for k, n in enumerate((3000, 2600, 3400))]
    clouds = base + [rc.moved(base[0], 3.0, 0.4, -0.2), rc.moved(base[1], -2.0, -0.3, 0.3), rc.moved(base[2], 1.5, 0.2, 0.2)]
    F = len(clouds)
    maps = sc.Maps()
    maps.add([(0, sc.IDENTITY), (1, sc.planar(0.5, 0.1, 0.0))])
    maps.add([(2, sc.planar(-0.5, 0.0, 0.1)), (1, sc.IDENTITY), (0, sc.planar(0.3, -0.1, 0.0))])
    maps.add([(2, sc.IDENTITY)])
    m = sc.matches([(3, 0, 3.5), (4, 1, -2.5), (5, 2, 1.0), (5, 1, 1.0), (3, 0, 183.0)])
    offs = np.zeros(F + 1, np.uint64)
    offs[1:] = np.cumsum([len(c) for c in clouds])
    stride = bev_amd.regfront_max_out(max(len(c) for c in clouds))
    leaf = 0.5
    pn = [rf.chain(c) for c in clouds]
    coarse = pv.expected(pn, maps, m, leaf, stride=stride, threads=THREADS)
    guesses = [coarse[0][k, coarse[1][k]]["T"].reshape(4, 4).copy() for k in range(len(m))]
    fine = sc.expected(clouds, maps, m, fl.params(**fl.FINE), guesses, threads=THREADS)
    dev = torch.device("cuda:0")
    ctx = _ctx(max_points=4096)
    try:
        d_clouds = _dev(rc.packed(clouds))
        d_pn = torch.zeros(F * stride * 48, dtype=torch.uint8, device=dev)
        d_cnt = torch.zeros(F, dtype=torch.int32, device=dev)
        d_res, d_best = _outputs(len(m), 0xEE)
        d_fine = torch.zeros(len(m) * R, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.registration_front_device(F, d_clouds.data_ptr(), offs, d_pn.data_ptr(), stride, d_cnt.data_ptr())
        ctx.submap_coarse_voxel_registration_device(F, d_pn.data_ptr(), stride, d_cnt.data_ptr(), *maps.arrays(), m, d_res.data_ptr(),
                                                    d_best.data_ptr(), leaf)
        ctx.submap_voxel_registration_device(F, d_clouds.data_ptr(), offs, *maps.arrays(), m, d_fine.data_ptr(), 0.0,
                                             d_res.data_ptr(), d_best.data_ptr())
        ctx.synchronize()
        assert d_cnt.cpu().numpy().tolist() == [len(p) for p in pn]
        _check("coarse", _read(d_res, d_best, len(m)), coarse)
        got = d_fine.cpu().numpy().view(ICP_RESULT_DTYPE)
        bad = [k for k in range(len(m)) if not _same(got[k], fine[k])]
        assert not bad, f"fine: {bad}: {got[bad[0]]} != {fine[bad[0]]}"
    finally:
        ctx.close()
    print(f"coarse states {coarse[0]['state'].tolist()} best {coarse[1].tolist()}; fine states {fine['state'].tolist()}")
    assert (coarse[0]["state"][:4] != NOCORR).all() and (fine["state"][:4] != NOCORR).all()


def test_calls_of_different_sizes_with_the_pair_call_between_equal_the_checker():
    import torch

    S = pv.seeded_list()
    frames, stride, maps = S["frames"], S["stride"], S["maps"]
    big_m, small_m = S["m"], S["m"][:3]
    exp_big = pv.seeded_expected(0.2, pv.RADIUS, THREADS)
    exp_half = pv.seeded_expected(0.5, pv.RADIUS, THREADS)
    pair_m = sc.matches([(S["H"] + i, i, 1.0) for i in range(S["H"])])
    ctx = _ctx()
    try:
        d = _upload(frames, stride)
        outs = [_outputs(len(mm)) for mm in (small_m, big_m, small_m, big_m)]
        pair_a, pair_b = _outputs(len(pair_m)), _outputs(len(pair_m))
        torch.cuda.synchronize()
        call = lambda mm, o, leaf: ctx.submap_coarse_voxel_registration_device(
            len(frames), d[0].data_ptr(), stride, d[1].data_ptr(), *maps.arrays(), mm, o[0].data_ptr(), o[1].data_ptr(), leaf)
        pair = lambda o: ctx.coarse_registration_device(len(frames), d[0].data_ptr(), stride, d[1].data_ptr(), pair_m, o[0].data_ptr(),
                                                        o[1].data_ptr())
        call(small_m, outs[0], 0.5)   # a small call first: the next one grows the workspace and the table of a context in use
        call(big_m, outs[1], 0.2)
        pair(pair_a)                  # the pair call shares the buffer and the table
        call(small_m, outs[2], 0.2)
        call(big_m, outs[3], 0.5)
        pair(pair_b)
        ctx.synchronize()
        _check("0: small, 0.5", _read(*outs[0], 3), (exp_half[0][:3], exp_half[1][:3]))
        _check("1: the list, 0.2", _read(*outs[1], len(big_m)), exp_big)
        _check("2: small, 0.2", _read(*outs[2], 3), (exp_big[0][:3], exp_big[1][:3]))
        _check("3: the list, 0.5", _read(*outs[3], len(big_m)), exp_half)
        _check("the pair calls", _read(*pair_a, len(pair_m)), _read(*pair_b, len(pair_m)))
    finally:
        ctx.close()


# ---- g. refused arguments -----------------------------------------------------------------------------------------------------------
def test_every_refused_argument_leaves_the_outputs_untouched():
    import torch

    lib = bev_amd.load_lib()
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    stride = 64
    frames = [pv.flat_frame(40, 9991), cc.move(pv.flat_frame(40, 9991), sc.planar(1.0, 0.1, 0.1))]
    maps = sc.Maps()
    maps.add([(0, sc.IDENTITY), (0, sc.shift(0.1))])
    maps.add([(1, sc.IDENTITY)])
    moffs, eframe, epose = maps.arrays()
    m = sc.matches([(1, 0, 1.0), (0, 1, -1.0)])
    prm = bev_amd.icp_params()
    cap = 2 * stride
    n_at = cc.COARSE_MAX_TARGET // 4096
    one_more = sc.Maps()
    one_more.add([(0, sc.IDENTITY)] * (n_at + 1))
    one_more.add([(1, sc.IDENTITY)])
    ctx = _ctx()
    try:
        d_pn, d_cnt = _upload(frames, stride)
        d_res, d_best = _outputs(len(m), 0xA5)
        dev = torch.device("cuda:0")
        d_out = torch.full((2 * cap * 48,), 0xA5, dtype=torch.uint8, device=dev)
        d_n = torch.full((8,), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        h, pn, cnt = ctx._h, C.c_void_p(d_pn.data_ptr()), C.c_void_p(d_cnt.data_ptr())
        res, best = C.c_void_p(d_res.data_ptr()), C.c_void_p(d_best.data_ptr())
        out, n_out = C.c_void_p(d_out.data_ptr()), C.c_void_p(d_n.data_ptr())
        ptr = lambda a: a.ctypes.data if a is not None else None

        def reg(leaf=0.5, radius=2.0, n_frames=2, pn_=pn, stride_=stride, cnt_=cnt, n_maps=2, moffs_=moffs, eframe_=eframe, epose_=epose,
                n_matches=2, m_=m, prm_=prm, res_=res, best_=best):
            return lib.bev_submap_coarse_voxel_registration_device_resident(
                h, n_frames, pn_, stride_, cnt_, leaf, radius, None, n_maps, u64(moffs_) if moffs_ is not None else None, ptr(eframe_),
                ptr(epose_), n_matches, ptr(m_), C.byref(prm_) if prm_ is not None else None, res_, best_)

        def cloud(leaf=0.5, radius=2.0, n_frames=2, pn_=pn, stride_=stride, cnt_=cnt, n_maps=2, moffs_=moffs, eframe_=eframe,
                  epose_=epose, out_stride=cap, out_=out, n_out_=n_out):
            return lib.bev_submap_pn_cloud_device_resident(
                h, n_frames, pn_, stride_, cnt_, leaf, radius, None, n_maps, u64(moffs_) if moffs_ is not None else None, ptr(eframe_),
                ptr(epose_), out_stride, out_, n_out_)

        def other(a, k, v):
            a = a.copy()
            a[k] = v
            return a

        def match(k, field, v):
            mm = m.copy()
            mm[field][k] = v
            return mm

        nan, inf = float("nan"), float("inf")
        refused = {
            "leaf -1": (reg(leaf=-1.0), INVALID), "leaf nan": (reg(leaf=nan), INVALID), "leaf inf": (reg(leaf=inf), INVALID),
            "radius 0": (reg(radius=0.0), INVALID), "radius -1": (reg(radius=-1.0), INVALID), "radius nan": (reg(radius=nan), INVALID),
            "radius inf": (reg(radius=inf), INVALID),
            "n_frames < 0": (reg(n_frames=-1), INVALID), "n_maps < 0": (reg(n_maps=-1), INVALID), "n_matches < 0": (reg(n_matches=-1), INVALID),
            "iterations 0": (reg(prm_=bev_amd.icp_params(max_iterations=0)), INVALID), "stride 0": (reg(stride_=0), INVALID),
            "NULL frames": (reg(pn_=None), INVALID), "NULL counts": (reg(cnt_=None), INVALID), "NULL matches": (reg(m_=None), INVALID),
            "NULL results": (reg(res_=None), INVALID), "NULL best": (reg(best_=None), INVALID),
            "NULL map offsets": (reg(moffs_=None), INVALID), "NULL entry frames": (reg(eframe_=None), INVALID),
            "NULL entry poses": (reg(epose_=None), INVALID),
            "decreasing map offsets": (reg(moffs_=np.array([0, 3, 2], np.uint64)), INVALID),
            "entry frame 2": (reg(eframe_=other(eframe, 1, 2)), INVALID), "query 2": (reg(m_=match(0, "query_idx", 2)), INVALID),
            "map 2": (reg(m_=match(1, "match_idx", 2)), INVALID),
            "a map one entry above the capacity bound": (reg(stride_=4096, moffs_=one_more.arrays()[0], eframe_=one_more.arrays()[1],
                                                             epose_=one_more.arrays()[2]), TOO_LARGE),
            "cloud: leaf -1": (cloud(leaf=-1.0), INVALID), "cloud: leaf nan": (cloud(leaf=nan), INVALID),
            "cloud: radius 0": (cloud(radius=0.0), INVALID), "cloud: radius nan": (cloud(radius=nan), INVALID),
            "cloud: n_frames < 0": (cloud(n_frames=-1), INVALID), "cloud: n_maps < 0": (cloud(n_maps=-1), INVALID),
            "cloud: stride 0": (cloud(stride_=0), INVALID), "cloud: NULL frames": (cloud(pn_=None), INVALID),
            "cloud: NULL counts": (cloud(cnt_=None), INVALID), "cloud: NULL out": (cloud(out_=None), INVALID),
            "cloud: NULL counts out": (cloud(n_out_=None), INVALID), "cloud: NULL map offsets": (cloud(moffs_=None), INVALID),
            "cloud: entry frame -1": (cloud(eframe_=other(eframe, 0, -1)), INVALID),
            "cloud: out_stride below the largest capacity": (cloud(out_stride=cap - 1), INVALID),
            "cloud: the same at leaf 0": (cloud(leaf=0.0, out_stride=cap - 1), INVALID),
            "cloud: a map above the capacity bound": (cloud(stride_=4096, moffs_=one_more.arrays()[0], eframe_=one_more.arrays()[1],
                                                            epose_=one_more.arrays()[2], out_stride=1 << 23), TOO_LARGE),
        }
        ctx.synchronize()
        wrong = {k: v for k, v in refused.items() if v[0] != v[1]}
        assert not wrong, wrong
        for d_x in (d_res, d_best, d_out, d_n):
            assert (d_x.cpu().numpy() == 0xA5).all(), "a refused call wrote its outputs"
        assert reg(n_matches=0, m_=None, res_=None, best_=None, pn_=None, cnt_=None, stride_=0) == OK
        assert reg(n_frames=0, n_maps=0, n_matches=0, pn_=None, cnt_=None, moffs_=None, eframe_=None, epose_=None, m_=None, res_=None,
                   best_=None) == OK
        assert cloud(n_frames=0, n_maps=0, pn_=None, cnt_=None, moffs_=None, eframe_=None, epose_=None, out_=None, n_out_=None) == OK
        assert reg(leaf=0.0, radius=nan) == OK                # radius is not read without a grid
        ctx.synchronize()
        for d_x in (d_out, d_n):
            assert (d_x.cpu().numpy() == 0xA5).all()
        exp0 = cc.expected(frames, maps, m, None, stride, threads=2)
        _check("leaf 0", _read(d_res, d_best, len(m)), exp0)
        assert reg() == OK and cloud() == OK                 # the accepted calls, at the exact out_stride
        ctx.synchronize()
        tgt = pv.all_targets(frames, maps, stride, 0.5)
        _check("accepted", _read(d_res, d_best, len(m)), pv.expected(frames, maps, m, 0.5, stride=stride, threads=2, targets=dict(enumerate(tgt))))
        rows = d_out.cpu().numpy().reshape(2, cap, 48)
        n = d_n.cpu().numpy().view(np.uint32)
        _check_clouds("accepted", ([np.ascontiguousarray(rows[g, : n[g]]).view(F32).reshape(-1, 12) for g in range(2)], n), tgt)
    finally:
        ctx.close()
