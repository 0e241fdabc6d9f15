"""GPU: the top part over the union of a map's moved full clouds, thinned, as the coarse stage's target
(bev_submap_top_part_cloud_device_resident, bev_submap_top_part_coarse_registration_device_resident).  Every
comparison is of bytes: whole PointNormal rows and counts of the maps, whole bev_icp_result_t records and the choice between the
guesses, against the checker composition of submap_top_cases.py.  Cases that pin only the selection use the cloud call with
pn_leaf = 0, so the checker's O(n^2) normals are not involved:

  a. the seeded list at leaves 0.2 and 0.5 (radius 2) and at a radius below the leaf: results, best, every map's rows and count;
     the same bytes under a group cap that forces several launch groups;
  b. the selection: cell counts of 19 and 20, rank rounding, the tie rule, a threshold inside a run of equal z, degenerate
     digits, poses, empty targets, labels and non-finite records (submap_top_cases.edge_cases); one cell of about 70,000 records
     from three entries; selections of 4095, 4096 and 4097 keys; 257 entries;
  c. the voxel grid's overflow branch; out_stride exactly the bound, a guard region behind d_out, rows past a count untouched;
  d. front end, this call and the fine stage chained without a synchronisation; calls of different sizes on one context with
     §6q's call between them;
  e. every refused argument, the outputs untouched;
  f. §6q's and §6m's seeded lists through their own entry points still give the checker's bytes.
"""
import ctypes as C
import math
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
import submap_top_cases as tc
from bev_amd import ICP_RESULT_DTYPE
from submap_reg_gpu_lib import F32, INVALID, OK, R, THREADS, TOO_LARGE, _ctx, _dev, _offsets, _same

pytestmark = pytest.mark.gpu
GROUP_CAP = 600000  # bytes
NOCORR = bev_amd.ICP_NO_CORRESPONDENCES
FILL = 0xCD


@pytest.fixture(scope="module", autouse=True)
def _checkers():
    icp_lib.build()
    fl.build()
    rf.build()


@pytest.fixture(scope="module")
def ctx():
    c = _ctx(max_points=4096)
    yield c
    c.close()


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


def _bound(clouds, maps):
    return tc.max_out(max([tc.union_cap(clouds, maps, g) for g in range(len(maps))] + [0]))


def _clouds(ctx, clouds, maps, leaf, radius=tc.RADIUS, vp=None, d=None):
    """every map's rows and count through the cloud call, out_stride exactly the bound; rows past a count and a guard region
    behind d_out must stay as they were"""
    import torch

    d_clouds = d if d is not None else _dev(rc.packed(clouds))
    G, cap, guard = len(maps), _bound(clouds, maps), 4096
    dev = torch.device("cuda:0")
    d_out = torch.full((G * cap * 48 + guard,), FILL, dtype=torch.uint8, device=dev)
    d_n = torch.full((G * 4,), FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.submap_top_part_cloud_device(len(clouds), d_clouds.data_ptr(), _offsets(clouds), *maps.arrays(), leaf, cap, d_out.data_ptr(),
                                     d_n.data_ptr(), radius, vp)
    ctx.synchronize()
    raw = d_out.cpu().numpy()
    assert (raw[G * cap * 48:] == FILL).all(), "the guard region behind d_out was written"
    counts = d_n.cpu().numpy().view(np.uint32)
    body = raw[: G * cap * 48].reshape(G, cap, 48)
    rows = []
    for g in range(G):
        assert counts[g] <= cap
        assert (body[g, counts[g]:] == FILL).all(), f"map {g}: rows past its count {counts[g]} were written"
        rows.append(body[g, : counts[g]].copy().view(F32).reshape(-1, 12))
    return rows, counts


def _outputs(n, fill=0):
    import torch

    dev = torch.device("cuda:0")
    return (torch.full((max(n, 1) * 2 * R,), fill, dtype=torch.uint8, device=dev),
            torch.full((max(n, 1) * 4,), fill, dtype=torch.uint8, device=dev))


def _read(d_res, d_best, n):
    return d_res.cpu().numpy().view(ICP_RESULT_DTYPE).reshape(-1, 2)[:n], d_best.cpu().numpy().view(np.int32)[:n]


def _stride(pn):
    return max(1, max(len(p) for p in pn))


def _reg(ctx, clouds, pn, maps, m, leaf, radius=tc.RADIUS, vp=None, prm=None):
    import torch

    stride = _stride(pn)
    d_clouds, d_pn = _dev(rc.packed(clouds)), _dev(rc.strided(pn, stride))
    d_cnt = _dev(np.array([len(p) for p in pn], np.uint32))
    d_res, d_best = _outputs(len(m))
    torch.cuda.synchronize()
    ctx.submap_top_part_coarse_registration_device(len(clouds), d_clouds.data_ptr(), _offsets(clouds), d_pn.data_ptr(), stride,
                                                   d_cnt.data_ptr(), *maps.arrays(), m, d_res.data_ptr(), d_best.data_ptr(), leaf,
                                                   radius, vp, prm)
    ctx.synchronize()
    return _read(d_res, d_best, len(m))


# ---- a. the seeded list -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf,radius", [(l, tc.RADIUS) for l in tc.LEAVES] + [tc.ODD_PAIR])
def test_the_seeded_list_equals_the_checker(ctx, leaf, radius):
    S = tc.seeded_list()
    exp = tc.seeded_expected(leaf, radius, THREADS)
    assert tc.condition(exp[0]).all()
    _check_clouds(f"maps at leaf {leaf}", _clouds(ctx, S["clouds"], S["maps"], leaf, radius), tc.seeded_targets(leaf, radius))
    _check(f"leaf {leaf} radius {radius}", _reg(ctx, S["clouds"], S["pn"], S["maps"], S["m"], leaf, radius), exp)


def test_the_seeded_list_selection_equals_the_checker(ctx):
    S = tc.seeded_list()
    _check_clouds("top(g)", _clouds(ctx, S["clouds"], S["maps"], 0.0), [tc.rows_of_top(t) for t in tc.seeded_tops()])


def test_a_group_cap_that_forces_several_launch_groups_gives_the_same_bytes():
    S = tc.seeded_list()
    used = list(range(len(S["maps"])))
    n_groups, alone = tc.group_count(S["clouds"], S["maps"], used, GROUP_CAP)
    assert n_groups >= 4 and alone >= 1
    saved = os.environ.get("BEV_SUBMAP_REG_GROUP")
    os.environ["BEV_SUBMAP_REG_GROUP"] = str(GROUP_CAP)
    try:
        capped = _ctx(max_points=4096)
    finally:
        if saved is None:
            os.environ.pop("BEV_SUBMAP_REG_GROUP", None)
        else:
            os.environ["BEV_SUBMAP_REG_GROUP"] = saved
    try:
        capped.profile_enable(True)
        capped.profile_reset()
        _check_clouds("capped maps", _clouds(capped, S["clouds"], S["maps"], 0.5), tc.seeded_targets(0.5))
        launches = {s["name"]: s["launches"] for s in capped.profile_get()}
        assert launches.get("k_submap_top_keys") == n_groups, launches
        _check("capped", _reg(capped, S["clouds"], S["pn"], S["maps"], S["m"], 0.5), tc.seeded_expected(0.5, tc.RADIUS, THREADS))
    finally:
        capped.close()


# ---- b. the selection ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.edge_cases()))
def test_the_selection_on_the_edge_clouds_equals_the_checker(ctx, name):
    clouds, maps = tc.edge_cases()[name]
    exp = tc.edge_expected(name)
    _check_clouds(name, _clouds(ctx, clouds, maps, 0.0), exp)
    print(name, [len(e) for e in exp])


def _rank(n):
    return int(math.floor(float(np.float32(0.2) * np.float32(n)) + 0.5))


def test_one_cell_of_seventy_thousand_records_from_three_entries(ctx):
    rng = np.random.default_rng(5150)
    clouds = []
    for n in (30000, 25001, 15000):
        xyz = np.zeros((n, 3), F32)
        xyz[:, :2] = rng.uniform(-9, 9, (n, 2))
        # coarse z values: long runs of equal z across the entries, and a few hundred distinct ones
        xyz[:, 2] = np.round(rng.normal(1.0, 0.5, n) * 64) / 64
        clouds.append(tc.records(xyz, np.where(rng.uniform(0, 1, n) < 0.02, 0, 1)))
    maps = sc.Maps()
    maps.add([(0, sc.IDENTITY), (1, sc.shift(dz=0.125)), (2, sc.planar(1.0, 0.1, -0.1))])
    exp = [tc.rows_of_top(tc.top(clouds, maps.entries(0)))]
    assert len(exp[0]) > 8192 * 1.5
    _check_clouds("70,000", _clouds(ctx, clouds, maps, 0.0), exp)


def test_selections_of_4095_4096_and_4097_keys(ctx):
    rng = np.random.default_rng(4096)
    sizes = [next(n for n in range(5 * k - 5, 5 * k + 6) if _rank(n) == k) for k in (tc.TILE - 1, tc.TILE, tc.TILE + 1)]
    clouds = []
    for n in sizes:
        xyz = np.zeros((n, 3), F32)
        xyz[:, :2] = rng.uniform(-9, 9, (n, 2))
        xyz[:, 2] = rng.uniform(0, 3, n)
        clouds.append(tc.records(xyz))
    maps = sc.Maps()
    for f in range(3):
        maps.add([(f, sc.IDENTITY)])
    exp = [tc.rows_of_top(tc.top(clouds, maps.entries(g))) for g in range(3)]
    assert [len(e) for e in exp] == [tc.TILE - 1, tc.TILE, tc.TILE + 1]
    _check_clouds("tile", _clouds(ctx, clouds, maps, 0.0), exp)


def test_a_map_of_257_entries(ctx):
    rng = np.random.default_rng(257)
    clouds = [tc.column(rng.uniform(0, 3, 30)), tc.column(rng.uniform(0, 3, 7), y=2.0)]
    maps = sc.Maps()
    maps.add([(k % 2, sc.shift(dx=0.001 * k, dz=float(rng.uniform(-0.5, 0.5)))) for k in range(257)])
    exp = [tc.rows_of_top(tc.top(clouds, maps.entries(0)))]
    assert len(exp[0]) == _rank(129 * 30 + 128 * 7)
    _check_clouds("257 entries", _clouds(ctx, clouds, maps, 0.0), exp)


# ---- c. overflow and bookkeeping ------------------------------------------------------------------------------------------------
def test_the_voxel_overflow_branch_keeps_the_top_part_and_computes_its_normals(ctx):
    a = tc.wall_cloud(600, 9301)
    clouds = [a, tc.orc.transform_cloud(a, sc.planar(2.0, 0.3, 0.1))]
    maps = sc.Maps()
    g = maps.add([(0, sc.IDENTITY), (1, sc.planar(-1.0, 0.1, 0.0))])
    leaf = 1e-6
    t = tc.top(clouds, maps.entries(g))
    rows, over = tc.thin(t, leaf)
    assert over and len(rows) == len(t) and np.isfinite(rows[:, 4:6]).any()
    _check_clouds("overflow", _clouds(ctx, clouds, maps, leaf), [rows])
    pn = tc.queries(clouds)
    m = sc.matches([(1, g, 2.0)])
    _check("overflow", _reg(ctx, clouds, pn, maps, m, leaf), tc.expected(pn, clouds, maps, m, leaf, targets={g: rows}))


def test_a_viewpoint_off_the_origin_equals_the_checker(ctx):
    a = tc.wall_cloud(1500, 9302)
    clouds = [a]
    maps = sc.Maps()
    g = maps.add([(0, sc.IDENTITY), (0, sc.planar(-1.0, 0.1, 0.0))])
    vp = (15.0, -8.0, 3.0)
    exp = tc.all_targets(clouds, maps, 0.5, viewpoint=vp)
    assert not _same(exp[g], tc.target(clouds, maps.entries(g), 0.5))
    _check_clouds("viewpoint", _clouds(ctx, clouds, maps, 0.5, vp=vp), exp)


# ---- d. chaining and call order -------------------------------------------------------------------------------------------------
def test_front_end_this_call_and_the_fine_stage_chained_without_a_synchronisation(ctx):
    import torch

    base = [tc.wall_cloud(n, 9600 + k) for k, n in enumerate((3000, 2600, 3400))]
    clouds = base + [tc.orc.transform_cloud(base[k], sc.planar(a, x, y)) for k, (a, x, y) in
                     enumerate(((3.0, 0.4, -0.2), (-2.0, -0.3, 0.3), (1.5, 0.2, 0.2)))]
    F = len(clouds)
    maps = sc.Maps()
    maps.add([(0, sc.IDENTITY), (1, sc.planar(0.5, 0.1, 0.0))])
    maps.add([(2, sc.planar(-0.5, 0.0, 0.1)), (1, sc.IDENTITY), (0, sc.planar(0.3, -0.1, 0.0))])
    maps.add([(2, sc.IDENTITY)])
    m = sc.matches([(3, 0, 3.5), (4, 1, -2.5), (5, 2, 1.0), (5, 1, 1.0), (3, 0, 183.0)])
    offs = _offsets(clouds)
    stride = bev_amd.regfront_max_out(max(len(c) for c in clouds))
    leaf = 0.5
    pn = tc.queries(clouds)
    coarse = tc.expected(pn, clouds, maps, m, leaf, threads=THREADS)
    guesses = [coarse[0][k, coarse[1][k]]["T"].reshape(4, 4).copy() for k in range(len(m))]
    fine = sc.expected(clouds, maps, m, fl.params(**fl.FINE), guesses, threads=THREADS)
    dev = torch.device("cuda:0")
    d_clouds = _dev(rc.packed(clouds))
    d_pn = torch.zeros(F * stride * 48, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(F, dtype=torch.int32, device=dev)
    d_res, d_best = _outputs(len(m), 0xEE)
    d_fine = torch.zeros(len(m) * R, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.registration_front_device(F, d_clouds.data_ptr(), offs, d_pn.data_ptr(), stride, d_cnt.data_ptr())
    ctx.submap_top_part_coarse_registration_device(F, d_clouds.data_ptr(), offs, d_pn.data_ptr(), stride, d_cnt.data_ptr(),
                                                   *maps.arrays(), m, d_res.data_ptr(), d_best.data_ptr(), leaf)
    ctx.submap_voxel_registration_device(F, d_clouds.data_ptr(), offs, *maps.arrays(), m, d_fine.data_ptr(), 0.0,
                                         d_res.data_ptr(), d_best.data_ptr())
    ctx.synchronize()
    assert d_cnt.cpu().numpy().tolist() == [len(p) for p in pn]
    _check("coarse", _read(d_res, d_best, len(m)), coarse)
    got = d_fine.cpu().numpy().view(ICP_RESULT_DTYPE)
    bad = [k for k in range(len(m)) if not _same(got[k], fine[k])]
    assert not bad, f"fine: {bad}: {got[bad[0]]} != {fine[bad[0]]}"
    assert (coarse[0]["state"][:4] != NOCORR).all() and (fine["state"][:4] != NOCORR).all()


def test_calls_of_different_sizes_with_the_thinned_concatenation_call_between_equal_the_checker(ctx):
    S = tc.seeded_list()
    small_clouds, small_maps = tc.edge_cases()["tie_rule"]
    small = tc.edge_expected("tie_rule")
    P = pv.seeded_list()
    for _ in range(2):
        _check_clouds("small", _clouds(ctx, small_clouds, small_maps, 0.0), small)
        _check("large", _reg(ctx, S["clouds"], S["pn"], S["maps"], S["m"], 0.5), tc.seeded_expected(0.5, tc.RADIUS, THREADS))
        _check("between", _old_pn_call(ctx, P, 0.5), pv.seeded_expected(0.5, pv.RADIUS, THREADS))
    _check_clouds("large maps", _clouds(ctx, S["clouds"], S["maps"], 0.2), tc.seeded_targets(0.2))


def test_an_empty_target_ends_as_the_coarse_stage_ends_on_one(ctx):
    clouds, maps = tc.edge_cases()["empty_targets"]
    clouds = clouds + [tc.wall_cloud(1500, 9401)]
    pn = tc.queries(clouds)
    m = sc.matches([(2, 0, 0.0), (2, 1, 1.0)])
    exp = tc.expected(pn, clouds, maps, m, 0.5)
    assert (exp[0]["state"] == NOCORR).all()
    _check("empty targets", _reg(ctx, clouds, pn, maps, m, 0.5), exp)


# ---- e. refusals ------------------------------------------------------------------------------------------------------------------
def test_every_refused_argument_leaves_the_outputs_untouched(ctx):
    import torch

    lib = bev_amd.load_lib()
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64)) if a is not None else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    clouds = [tc.column(np.linspace(0, 3, 40)), tc.column(np.linspace(0, 2, 30), x=1.0)]
    pn = [pv.flat_frame(40, 9991), pv.flat_frame(40, 9992)]
    stride = 64
    maps = sc.Maps()
    maps.add([(0, sc.IDENTITY), (0, sc.shift(0.1))])
    maps.add([(1, sc.IDENTITY)])
    moffs, eframe, epose = maps.arrays()
    offs = _offsets(clouds)
    m = sc.matches([(1, 0, 1.0), (0, 1, -1.0)])
    prm = bev_amd.icp_params()
    cap = _bound(clouds, maps)
    # a union above 2^24 records: frame offsets that claim 2^23 + 1 records for frame 0, named twice (nothing is read: refused)
    huge = np.array([0, (1 << 23) + 1, (1 << 23) + 31], np.uint64)
    dev = torch.device("cuda:0")
    d_clouds, d_pn = _dev(rc.packed(clouds)), _dev(rc.strided(pn, stride))
    d_cnt = _dev(np.array([40, 40], np.uint32))
    d_res, d_best = _outputs(len(m), 0xA5)
    d_out = torch.full((2 * cap * 48,), 0xA5, dtype=torch.uint8, device=dev)
    d_n = torch.full((8,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    h, cl, pnp, cnt = ctx._h, C.c_void_p(d_clouds.data_ptr()), C.c_void_p(d_pn.data_ptr()), C.c_void_p(d_cnt.data_ptr())
    res, best = C.c_void_p(d_res.data_ptr()), C.c_void_p(d_best.data_ptr())
    out, n_out = C.c_void_p(d_out.data_ptr()), C.c_void_p(d_n.data_ptr())

    def reg(leaf=0.5, radius=2.0, n_frames=2, cl_=cl, offs_=offs, pn_=pnp, stride_=stride, cnt_=cnt, n_maps=2, moffs_=moffs,
            eframe_=eframe, epose_=epose, n_matches=2, m_=m, prm_=prm, res_=res, best_=best):
        return lib.bev_submap_top_part_coarse_registration_device_resident(
            h, n_frames, cl_, u64(offs_), pn_, stride_, cnt_, leaf, radius, None, n_maps, u64(moffs_), ptr(eframe_), ptr(epose_),
            n_matches, ptr(m_), C.byref(prm_) if prm_ is not None else None, res_, best_)

    def cloud(leaf=0.5, radius=2.0, n_frames=2, cl_=cl, offs_=offs, n_maps=2, moffs_=moffs, eframe_=eframe, epose_=epose,
              out_stride=cap, out_=out, n_out_=n_out):
        return lib.bev_submap_top_part_cloud_device_resident(h, n_frames, cl_, u64(offs_), leaf, radius, None, n_maps, u64(moffs_),
                                                             ptr(eframe_), ptr(epose_), out_stride, out_, n_out_)

    def other(a, k, v):
        a = a.copy()
        a[k] = v
        return a

    bad_prm = bev_amd.icp_params(max_iterations=0)
    bad_m = m.copy()
    bad_m["match_idx"][0] = 2
    bad_q = m.copy()
    bad_q["query_idx"][1] = -1
    for both in (reg, cloud):
        assert both(leaf=-0.5) == INVALID and both(leaf=float("nan")) == INVALID and both(leaf=float("inf")) == INVALID
        assert both(radius=0.0) == INVALID and both(radius=float("nan")) == INVALID and both(radius=-1.0) == INVALID
        assert both(n_frames=-1) == INVALID and both(n_maps=-1) == INVALID
        assert both(cl_=None) == INVALID and both(moffs_=None) == INVALID and both(eframe_=None) == INVALID
        assert both(epose_=None) == INVALID
        assert both(eframe_=other(eframe, 1, 2)) == INVALID and both(eframe_=other(eframe, 0, -1)) == INVALID
        assert both(moffs_=other(moffs, 1, 5)) == INVALID
        assert both(offs_=other(offs, 1, 1000)) == INVALID          # decreasing offsets
        assert both(offs_=huge) == INVALID                            # a map above the capacity cap
    assert lib.bev_submap_top_part_cloud_device_resident(None, 2, cl, u64(offs), 0.5, 2.0, None, 2, u64(moffs), ptr(eframe),
                                                         ptr(epose), cap, out, n_out) == INVALID
    assert reg(leaf=0.0) == INVALID
    assert reg(n_matches=-1) == INVALID and reg(m_=None) == INVALID and reg(res_=None) == INVALID and reg(best_=None) == INVALID
    assert reg(pn_=None) == INVALID and reg(cnt_=None) == INVALID and reg(stride_=0) == INVALID
    assert reg(prm_=bad_prm) == INVALID and reg(m_=bad_m) == INVALID and reg(m_=bad_q) == INVALID
    assert cloud(out_stride=cap - 1) == INVALID and cloud(out_=None) == INVALID and cloud(n_out_=None) == INVALID
    ctx.synchronize()
    for t in (d_res, d_best, d_out, d_n):
        assert (t.cpu().numpy() == 0xA5).all(), "a refused call wrote to an output"
    assert reg(n_matches=0, m_=None, res_=None, best_=None) == OK and cloud(n_maps=0, out_=None, n_out_=None) == OK
    assert cloud(leaf=0.0, radius=float("nan")) == OK                  # radius is not read without a leaf
    assert reg() == OK and cloud() == OK
    ctx.synchronize()
    assert bev_amd.submap_top_part_max_out(0) == 51 and bev_amd.submap_top_part_max_out(1 << 24) == (1 << 24) // 5 + 51


# ---- f. old behaviour -------------------------------------------------------------------------------------------------------------
def _old_pn_call(ctx, P, leaf):
    import torch

    frames, stride, maps, m = P["frames"], P["stride"], P["maps"], P["m"]
    d_pn, d_cnt = _dev(rc.strided(frames, stride)), _dev(np.array([len(f) for f in frames], np.uint32))
    d_res, d_best = _outputs(len(m))
    torch.cuda.synchronize()
    ctx.submap_coarse_voxel_registration_device(len(frames), d_pn.data_ptr(), stride, d_cnt.data_ptr(), *maps.arrays(), m,
                                                d_res.data_ptr(), d_best.data_ptr(), leaf)
    ctx.synchronize()
    return _read(d_res, d_best, len(m))


def test_the_thinned_concatenation_and_the_plain_concatenation_still_give_their_bytes(ctx):
    P = pv.seeded_list()
    _check("thinned concatenation", _old_pn_call(ctx, P, 0.5), pv.seeded_expected(0.5, pv.RADIUS, THREADS))
    Q = cc.seeded_list()
    _check("plain concatenation", _old_pn_call(ctx, Q, 0.0), cc.seeded_expected(THREADS))
