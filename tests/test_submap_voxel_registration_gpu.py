"""GPU: scan-to-map registration against maps thinned by a voxel grid over their union
(bev_submap_voxel_registration_device_resident, bev_submap_voxel_registration_batch, bev_submap_voxel_cloud_device_resident;
DESIGN.md §6l).  Every result is compared byte for byte, as a whole bev_icp_result_t or as x, y, z, 0 records, with the
checker composition of submap_vox_cases.py (§6k's target, the fine stage's sequential voxel grid over it at map_leaf, the
fine stage's sequential ICP):

  a. the main case: 400 matches against 31 maps of 0 .. 8 entries at map_leaf 0.2 and 0.5 under the whole tool's settings
     and the top-part tool's with an uploaded coarse table; map_leaf 0 equals bev_submap_registration_device_resident; a
     forced group cap (several launch groups, one map alone above the cap) changes nothing;
  b. the sort's boundaries: concatenations of 1, 255, 257, T - 1, T, T + 1, 2 T + 1 and 8 T + 1234 points (T = 4096);
  c. a thinned target above 16384 points (the grid's dimension saturates);
  d. the voxel grid's branches: a union that overflows (target = concatenation, a NaN record holding its index), a map_leaf
     of 1e6 (one point), an empty map, a map of empty voxel clouds, empty clouds first and in the middle, a matrix that
     overflows, a frame twice under one pose, a frame in many maps, matches sharing a map;
  e. the cloud call on all of those maps: counts, records, nothing behind the count; map_leaf 0 gives the concatenation;
  f. ordering: d_ordered input behind bev_process_device_resident; calls of different sizes and leaves and the pair call
     without a synchronisation; a call behind a non-blocking upload and a fill;
  g. every refused argument, outputs untouched; the batch form;
  h. which status a call gets that is wrong in two ways at once, for every scan-to-map entry point.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import reg_cases as rc
import submap_reg_cases as sc
import submap_vox_cases as vc
from bev_amd import POINT_DTYPE, synth
from submap_reg_gpu_lib import F32, INVALID, OK, R, THREADS, TOO_LARGE, _check, _ctx, _dev, _offsets, _results, _same
from submap_reg_gpu_lib import _fine_call as _call

pytestmark = pytest.mark.gpu
GROUP_CAP = 300000  # bytes: a few small maps per launch group, the map of 8 x 512 records alone above it


@pytest.fixture(scope="module", autouse=True)
def _checker():
    fl.build()


def _capacity(clouds, maps, g):
    return sum(len(clouds[f]) for f, _ in maps.entries(g))


def _cloud_call(ctx, clouds, maps, map_leaf, stride=None, fill=0xA5):
    """bev_submap_voxel_cloud_device_resident, synchronised: ([rows of map g], counts, the whole pre-filled output)"""
    import torch

    G = len(maps)
    stride = stride if stride is not None else max([_capacity(clouds, maps, g) for g in range(G)] + [1]) + 3
    d_clouds = _dev(rc.packed(clouds))
    d_out = torch.full((G * stride * 16,), fill, dtype=torch.uint8, device=d_clouds.device)
    d_cnt = torch.full((G * 4,), fill, dtype=torch.uint8, device=d_clouds.device)
    torch.cuda.synchronize()
    ctx.submap_voxel_cloud_device(len(clouds), d_clouds.data_ptr(), _offsets(clouds), *maps.arrays(), map_leaf, stride,
                                  d_out.data_ptr(), d_cnt.data_ptr())
    ctx.synchronize()
    raw = d_out.cpu().numpy().reshape(G, stride, 16)
    counts = d_cnt.cpu().numpy().view(np.uint32)
    return raw, counts


def _one_nan(rows):
    """the rows with every NaN as one bit pattern: IEEE 754 fixes neither the sign nor the payload of the NaN that 0 * inf
    makes in a transform, and the host checker's differs from the device's; every other value is compared bit for bit"""
    rows = np.array(rows, F32)
    rows[np.isnan(rows)] = np.nan
    return rows


def _check_clouds(name, ctx, clouds, maps, map_leaf, fill=0xA5):
    tg = vc.targets(clouds, maps, range(len(maps)), map_leaf, threads=THREADS)
    raw, counts = _cloud_call(ctx, clouds, maps, map_leaf, fill=fill)
    for g in range(len(maps)):
        exp = vc.rows(tg[g][1])
        assert counts[g] == len(exp), f"{name}: map {g} at {map_leaf}: {counts[g]} records, expected {len(exp)}"
        got = raw[g, : len(exp)].copy().view(F32).reshape(-1, 4)
        assert _same(_one_nan(got), _one_nan(exp)), f"{name}: map {g} at {map_leaf}: records differ"
        assert (raw[g, len(exp):] == fill).all(), f"{name}: map {g} at {map_leaf}: records behind the count were written"
    return tg


# ---- a. the main case --------------------------------------------------------------------------------------------------------
def _main_call(ctx, S, settings, map_leaf, d_clouds=None):
    if settings == "whole":
        return _call(ctx, S["clouds"], S["maps"], S["m"], bev_amd.icp_whole_defaults(), map_leaf, d_clouds)
    return _call(ctx, S["clouds"], S["maps"], S["m"], None, map_leaf, d_clouds, S["coarse"], S["best"])


@pytest.mark.parametrize("map_leaf", vc.MAP_LEAVES)
@pytest.mark.parametrize("settings", ["whole", "top"])
def test_the_main_case_equals_the_checker(settings, map_leaf):
    S = vc.main_case()
    exp = vc.main_expected(settings, map_leaf, THREADS)
    ctx = _ctx()
    try:
        got = _main_call(ctx, S, settings, map_leaf)
    finally:
        ctx.close()
    print(f"{settings} at {map_leaf}: {len(exp)} matches, states {np.bincount(exp['state'], minlength=6)}")
    _check(f"{settings} at {map_leaf}", got, exp)
    states = np.bincount(exp["state"], minlength=6)
    assert states[bev_amd.ICP_NO_CORRESPONDENCES] >= 2 and (states[1:5] > 0).sum() >= 2
    empty = exp[S["m"]["match_idx"] == S["empty"]]
    assert len(empty) == 2 and (empty["state"] == bev_amd.ICP_NO_CORRESPONDENCES).all()
    assert (empty["fitness"] == np.finfo(np.float64).max).all() and (empty["converged"] == 0).all()
    assert not _same(exp, vc.main_expected(settings, 0.0, THREADS))        # the second grid changes results


@pytest.mark.parametrize("settings", ["whole", "top"])
def test_map_leaf_0_equals_the_call_without_a_second_grid(settings):
    import torch

    S = vc.main_case()
    ctx = _ctx()
    try:
        d_clouds = _dev(rc.packed(S["clouds"]))
        got = _main_call(ctx, S, settings, 0.0, d_clouds)
        d_res = torch.zeros(len(S["m"]) * R, dtype=torch.uint8, device=d_clouds.device)
        kw = dict(params=bev_amd.icp_whole_defaults())
        if settings == "top":
            d_coarse, d_best = _dev(S["coarse"]), _dev(S["best"])
            kw = dict(d_coarse=d_coarse.data_ptr(), d_best=d_best.data_ptr())
        torch.cuda.synchronize()
        ctx.submap_registration_device(len(S["clouds"]), d_clouds.data_ptr(), _offsets(S["clouds"]), *S["maps"].arrays(), S["m"],
                                       d_res.data_ptr(), **kw)
        ctx.synchronize()
        _check(f"{settings}: map_leaf 0 against the existing entry point", got, _results(d_res))
    finally:
        ctx.close()
    _check(f"{settings}: map_leaf 0 against the checker", got, vc.main_expected(settings, 0.0, THREADS))


def test_a_forced_group_cap_gives_the_same_results():
    S = vc.main_case()
    maps, used = S["maps"], sorted({int(g) for g in S["m"]["match_idx"]})
    pow2 = lambda n: 0 if n == 0 else 1 << (n - 1).bit_length()
    # bevsubreg::map_bytes(cap, true), restated
    bytes_of = lambda g: (lambda c: 48 * c + 8 * pow2(c) + 4 * (c + 1) + 4 * (sc.GRID_CELLS + 1) + 64)(_capacity(S["clouds"], maps, g))
    groups, cur, alone = 0, 0, 0
    for g in used:
        b = bytes_of(g)
        if cur and cur + b > GROUP_CAP:
            groups, cur = groups + 1, 0
        alone += b > GROUP_CAP
        cur += b
    groups += 1 if cur else 0
    assert groups >= 4 and alone == 1, (groups, alone)     # several groups, the largest map alone above the cap
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
                got = _main_call(ctx, S, "whole", 0.2)
                launches[cap] = {k["name"]: k["launches"] for k in ctx.profile_get()}
            finally:
                ctx.close()
            _check(f"cap {cap}", got, vc.main_expected("whole", 0.2, THREADS))
    finally:
        if saved is None:
            os.environ.pop("BEV_SUBMAP_REG_GROUP", None)
        else:
            os.environ["BEV_SUBMAP_REG_GROUP"] = saved
    one, cut = launches[None], launches[str(GROUP_CAP)]
    assert one["k_submap_vox_move"] == one["k_submap_vox_keys"] == one["k_submap_vox_finish"] == 1 and "k_submap_target" not in one, one
    assert one["k_submap_vox_tile"] == 1 and "k_submap_vox_global" not in one, one      # 8 * 512 records: one tile per map
    assert cut["k_submap_vox_move"] == cut["k_submap_vox_finish"] == groups and cut["k_submap_icp"] >= groups - 1, cut


# ---- b. the sort's boundaries ------------------------------------------------------------------------------------------------
def test_every_kind_of_sort_stage_equals_the_checker():
    clouds, maps, m, counts = vc.sort_case()
    vox = vc.voxel_clouds(clouds, range(len(clouds)), threads=THREADS)
    tg = vc.targets(clouds, maps, range(len(maps)), 0.2, vox=vox, threads=THREADS)
    assert tuple(len(tg[g][0]) for g in range(len(maps))) == counts
    assert sum(len(tg[g][1]) < len(tg[g][0]) for g in range(len(maps))) >= 6        # voxels of two points, the largest map's too
    assert len(tg[len(maps) - 1][1]) < len(tg[len(maps) - 1][0])
    prm = fl.params(**fl.WHOLE)
    exp = vc.expected(clouds, maps, m, prm, 0.2, threads=THREADS)
    ctx = _ctx()
    try:
        ctx.profile_enable(True)
        got = _call(ctx, clouds, maps, m, prm, 0.2)
        launches = {k["name"]: k["launches"] for k in ctx.profile_get()}
        _check("sort boundaries", got, exp)
        _check_clouds("sort boundaries", ctx, clouds, maps, 0.2)
    finally:
        ctx.close()
    # the largest key array has 16 T keys: one tile launch, then k = 2 T .. 16 T: 1 + 2 + 3 + 4 stages across tiles, 4 merges
    assert launches["k_submap_vox_tile"] == 5 and launches["k_submap_vox_global"] == 10, launches
    assert (exp["state"] != bev_amd.ICP_NO_CORRESPONDENCES).all()


# ---- c. a thinned target larger than the grid's 128 x 128 points -------------------------------------------------------------
def test_a_thinned_target_above_16384_points_equals_the_checker():
    big = [rc.scene(4096, 4100 + k) for k in range(5)]
    for k, c in enumerate(big):                       # spread: each scene in a region of its own
        c["x"] += F32(60.0 * (k % 3))
        c["y"] += F32(60.0 * (k // 3))
    query = rc.moved(big[0][:300], 2.0, 0.2, -0.1)
    clouds = big + [query]
    maps = sc.Maps()
    g = maps.add([(k, sc.planar(0.1 * k, 0.01 * k, 0.0)) for k in range(5)])
    m = sc.matches([(5, g, 2.5), (0, g, 0.0)])
    tg = vc.targets(clouds, maps, [g], 0.2, threads=THREADS)
    assert len(tg[g][1]) > sc.GRID_CELLS and len(tg[g][0]) > 4 * vc.TILE
    prm = fl.params(**fl.WHOLE)
    exp = vc.expected(clouds, maps, m, prm, 0.2, threads=THREADS)
    ctx = _ctx()
    try:
        _check("saturated grid", _call(ctx, clouds, maps, m, prm, 0.2), exp)
        _check_clouds("saturated grid", ctx, clouds, maps, 0.2)
    finally:
        ctx.close()
    assert (exp["state"] != bev_amd.ICP_NO_CORRESPONDENCES).all()


# ---- d. the voxel grid's branches ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _branches():
    a, b, c = rc.scene(900, 5001), rc.scene(700, 5002), rc.scene(300, 5003)
    all_nan = rc._special("all_nan", 2026)
    zero = rc.scene(0, 5004)
    holes = rc._special("overflow", 2026)          # the frame's own voxel grid returns its input: NaN records keep their places
    holes["x"][5::7] = np.nan
    holes["z"][6::11] = np.inf
    query = rc.moved(a, 3.0, 0.2, 0.1)
    a_far = a.copy()
    a_far["x"] += F32(100.0)                       # every |x| above 3.4: 1e38 * x overflows for every point
    clouds = [a, b, c, all_nan, zero, holes, query, rc.moved(holes, -2.0, 0.1, 0.0), a_far]
    A, B, Cc, NAN, ZERO, HOLES, Q, HQ, AFAR = range(9)
    maps = sc.Maps()
    G = dict(
        far=maps.add([(A, sc.IDENTITY), (B, sc.shift(1e6, 0, 0)), (NAN, sc.IDENTITY)]),       # 1e6 apart: the union's grid overflows
        far_nan=maps.add([(Cc, sc.IDENTITY), (HOLES, sc.shift(1e6, 0, 0))]),                   # ... with NaN records in it
        none=maps.add([]),
        only_empty=maps.add([(NAN, sc.IDENTITY), (ZERO, sc.planar(1, 0, 0))]),
        gaps=maps.add([(NAN, sc.IDENTITY), (A, sc.IDENTITY), (ZERO, sc.planar(1, 0, 0)), (NAN, sc.planar(5, 1, 1)), (A, sc.planar(0.2, 0.03, 0))]),
        inf=maps.add([(AFAR, np.array([1e38, 0, 0, 0, 0, 1e38, 0, 0, 0, 0, 1, 0], F32)), (B, sc.IDENTITY), (B, sc.shift(0.02, 0, 0))]),
        holes=maps.add([(HOLES, sc.planar(1, 0.1, -0.1)), (Cc, sc.IDENTITY), (HOLES, sc.IDENTITY)]),  # NaN records: kept at 0.2, dropped at 1e6
        twice=maps.add([(A, sc.planar(0.5, 0.05, 0.0)), (A, sc.planar(0.5, 0.05, 0.0))]),
        shared=maps.add([(A, sc.planar(1, 0, 0)), (B, sc.IDENTITY), (A, sc.planar(1.1, 0.02, 0)), (Cc, sc.planar(-1, 0, 0.1))]),
        many=maps.add([(A, sc.IDENTITY), (Cc, sc.IDENTITY)]),
        octant=maps.add([(Cc, sc.shift(100, 100, 100)), (A, sc.shift(100, 100, 100))]),      # one voxel of a grid of 1e6
    )
    rows = [(Q, G["far"], 3.0), (B, G["far"], 0.0), (HQ, G["far_nan"], -2.0), (Cc, G["far_nan"], 0.0), (Q, G["none"], 0.0),
            (Cc, G["only_empty"], 0.0), (Q, G["gaps"], 3.0), (A, G["gaps"], 0.0), (B, G["inf"], 0.5), (HQ, G["holes"], -2.0),
            (Q, G["twice"], 2.0), (Q, G["shared"], 3.0), (B, G["shared"], 0.0), (Cc, G["shared"], 1.0), (Q, G["shared"], -3.0),
            (Q, G["many"], 3.0), (NAN, G["shared"], 0.0), (ZERO, G["twice"], 0.0), (Q, G["octant"], 0.0)]
    return clouds, maps, sc.matches(rows), G


def test_the_voxel_grid_branches_equal_the_checker():
    clouds, maps, m, G = _branches()
    tg = vc.targets(clouds, maps, range(len(maps)), 0.2, threads=THREADS)
    concat, thin = tg[G["far"]]
    assert _same(concat, thin) and len(thin) > 0                                   # the overflow branch: the target is the concatenation
    concat, thin = tg[G["far_nan"]]
    assert _same(concat, thin) and not np.isfinite(thin["x"]).all()                # ... NaN records in their places
    assert len(tg[G["none"]][1]) == 0 and len(tg[G["only_empty"]][1]) == 0
    concat, thin = tg[G["inf"]]
    n_inf = int((~np.isfinite(concat["x"])).sum())                                 # entry 0 overflows to infinity: dropped
    assert n_inf > 400 and np.isfinite(thin["x"]).all() and 0 < len(thin) < len(concat) - n_inf
    concat, thin = tg[G["holes"]]                                                  # (the frame itself spans 1e6: overflow again)
    assert _same(concat, thin) and not np.isfinite(thin["x"]).all() and not np.isfinite(thin["z"]).all()
    wide = vc.targets(clouds, maps, [G["holes"]], 1e6, threads=1)[G["holes"]][1]   # a grid that fits drops the NaN records
    assert 1 <= len(wide) <= 16 and np.isfinite(wide["x"]).all() and np.isfinite(wide["z"]).all()
    concat, thin = tg[G["twice"]]
    assert len(concat) // 4 < len(thin) <= len(concat) // 2                        # the same frame twice under one pose
    assert len(vc.targets(clouds, maps, [G["octant"]], 1e6, threads=1)[G["octant"]][1]) == 1    # a one-point target
    assert 1 < len(vc.targets(clouds, maps, [G["shared"]], 1e6, threads=1)[G["shared"]][1]) <= 8
    for name, prm in (("whole", fl.params(**fl.WHOLE)), ("top-part", fl.params(**fl.FINE))):
        for leaf in (0.2, 1e6):
            exp = vc.expected(clouds, maps, m, prm, leaf, threads=THREADS)
            ctx = _ctx()
            try:
                got = _call(ctx, clouds, maps, m, prm, leaf)
            finally:
                ctx.close()
            print(f"{name} at {leaf}: states {exp['state'].tolist()}")
            _check(f"{name} at {leaf}", got, exp)
            assert exp["state"][4] == exp["state"][5] == bev_amd.ICP_NO_CORRESPONDENCES
            assert exp["state"][0] != bev_amd.ICP_NO_CORRESPONDENCES and exp["state"][8] != bev_amd.ICP_NO_CORRESPONDENCES


# ---- e. the cloud call --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("map_leaf", [0.0, 0.2, 0.5, 1e6])
def test_the_cloud_call_writes_every_map_and_nothing_behind_its_count(map_leaf):
    S = vc.main_case()
    clouds, maps, _, G = _branches()
    ctx = _ctx()
    try:
        tg = _check_clouds("branches", ctx, clouds, maps, map_leaf)
        _check_clouds("main", ctx, S["clouds"], S["maps"], map_leaf, fill=0x3C)
        if map_leaf == 0.0:
            assert all(_same(tg[g][0], tg[g][1]) for g in tg)
        # the stride may be exactly the largest capacity; no maps at all is fine
        cap = max(_capacity(clouds, maps, g) for g in range(len(maps)))
        raw, counts = _cloud_call(ctx, clouds, maps, map_leaf, stride=cap)
        assert counts.tolist() == [len(tg[g][1]) for g in range(len(maps))]
        none = sc.Maps()
        ctx.submap_voxel_cloud_device(len(clouds), 0, _offsets(clouds), *none.arrays(), map_leaf, 0, 0, 0)
        ctx.synchronize()
    finally:
        ctx.close()


# ---- f. ordering ----------------------------------------------------------------------------------------------------------------
def test_marked_frames_in_the_d_ordered_layout_equal_the_checker():
    import torch

    p = bev_amd.params_for_sensor("HDL_64E")
    F, S = 4, p.slots
    frames = [synth.sweep(p, 900 + i, keep=0.25, n_dup=500) for i in range(F)]
    offs = _offsets(frames)
    dev = torch.device("cuda:0")
    rel = lambda i, j: sc.IDENTITY if i == j else sc.planar(0.2 * (j - i), 0.05 * (j - i), 0.01 * (j - i))
    maps = sc.Maps()
    for i in range(F):  # half-window 1
        maps.add([(j, rel(i, j)) for j in range(max(0, i - 1), min(F - 1, i + 1) + 1)])
    m = sc.matches([(1, 0, 1.0), (0, 1, -1.0), (3, 2, 1.0), (2, 3, -1.0)])
    ctx = bev_amd.BevContext(p, device=0, max_batch=F, max_points=max(len(f) for f in frames))
    try:
        d_in = _dev(np.concatenate(frames))
        d_ord = torch.zeros(F * S * 32, dtype=torch.uint8, device=dev)
        d_multi = torch.zeros(F * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device=dev)
        d_single = torch.zeros(F * p.mat_size ** 2, dtype=torch.uint8, device=dev)
        d_res = torch.zeros(len(m) * R, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.process_device(F, d_in.data_ptr(), offs, d_ord.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
        # straight behind the BEV call, no synchronisation: the marked clouds are read where the pipeline left them
        ctx.submap_voxel_registration_device(F, d_ord.data_ptr(), None, *maps.arrays(), m, d_res.data_ptr(), 0.2,
                                             params=bev_amd.icp_whole_defaults())
        ctx.synchronize()
        ordered = list(d_ord.cpu().numpy().view(POINT_DTYPE).reshape(F, S))
        got = _results(d_res)
    finally:
        ctx.close()
    exp = vc.expected(ordered, maps, m, fl.params(**fl.WHOLE), 0.2, threads=THREADS)
    _check("d_ordered", got, exp)
    assert (exp["state"] != bev_amd.ICP_NO_CORRESPONDENCES).all()


def test_calls_of_different_sizes_and_leaves_without_a_sync_equal_the_checker():
    import torch

    S = vc.main_case()
    clouds, maps, m, _ = _branches()
    prm = fl.params(**fl.WHOLE)
    exp_b = {leaf: vc.expected(clouds, maps, m, prm, leaf, threads=THREADS) for leaf in (0.0, 0.2)}
    pairs = sc.matches([(24 + i, i, 0.0) for i in range(4, 24)])                   # the pair call: frame against frame
    exp_pair = fl.fine(S["clouds"], [tuple(r) for r in pairs], None, prm, threads=THREADS)
    ctx = _ctx()
    try:
        dev = torch.device("cuda:0")
        d_main, d_br = _dev(rc.packed(S["clouds"])), _dev(rc.packed(clouds))
        d_r = [torch.zeros(len(mm) * R, dtype=torch.uint8, device=dev) for mm in (m, S["m"], m, S["m"], m)]
        d_pair = torch.zeros(len(pairs) * R, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        branches = lambda d, leaf: ctx.submap_voxel_registration_device(len(clouds), d_br.data_ptr(), _offsets(clouds), *maps.arrays(),
                                                                        m, d.data_ptr(), leaf, params=bev_amd.icp_whole_defaults())
        main = lambda d, leaf: ctx.submap_voxel_registration_device(len(S["clouds"]), d_main.data_ptr(), _offsets(S["clouds"]),
                                                                    *S["maps"].arrays(), S["m"], d.data_ptr(), leaf,
                                                                    params=bev_amd.icp_whole_defaults())
        branches(d_r[0], 0.2)   # a small call first: the next ones grow the workspace and the table of a context that is in use
        main(d_r[1], 0.5)
        branches(d_r[2], 0.0)
        ctx.fine_registration_device(len(S["clouds"]), d_main.data_ptr(), _offsets(S["clouds"]), pairs, d_pair.data_ptr(),
                                     params=bev_amd.icp_whole_defaults())           # the pair call shares the buffer
        main(d_r[3], 0.2)
        branches(d_r[4], 0.2)
        ctx.synchronize()
        _check("0: branches at 0.2", _results(d_r[0]), exp_b[0.2])
        _check("1: main at 0.5", _results(d_r[1]), vc.main_expected("whole", 0.5, THREADS))
        _check("2: branches at 0", _results(d_r[2]), exp_b[0.0])
        _check("3: the pair call between", _results(d_pair), exp_pair)
        _check("4: main at 0.2", _results(d_r[3]), vc.main_expected("whole", 0.2, THREADS))
        _check("5: branches at 0.2 again", _results(d_r[4]), exp_b[0.2])
    finally:
        ctx.close()


def test_the_call_waits_for_work_queued_on_the_default_stream():
    import torch

    S = vc.main_case()
    host = torch.from_numpy(rc.packed(S["clouds"]).view(np.uint8).reshape(-1).copy()).pin_memory()
    h_coarse = torch.from_numpy(S["coarse"].reshape(-1).view(np.uint8).copy()).pin_memory()
    h_best = torch.from_numpy(S["best"].view(np.uint8).copy()).pin_memory()
    dev = torch.device("cuda:0")
    ctx = _ctx()
    try:
        d_clouds, d_coarse, d_best = (torch.zeros(h.numel(), dtype=torch.uint8, device=dev) for h in (host, h_coarse, h_best))
        d_res = torch.zeros(len(S["m"]) * R, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        d_clouds.copy_(host, non_blocking=True)
        d_coarse.copy_(h_coarse, non_blocking=True)
        d_best.copy_(h_best, non_blocking=True)
        d_res.fill_(0xFF)
        ctx.submap_voxel_registration_device(len(S["clouds"]), d_clouds.data_ptr(), _offsets(S["clouds"]), *S["maps"].arrays(), S["m"],
                                             d_res.data_ptr(), 0.2, d_coarse.data_ptr(), d_best.data_ptr())
        ctx.synchronize()
        _check("behind an upload and a fill", _results(d_res), vc.main_expected("top", 0.2, THREADS))
    finally:
        ctx.close()


# ---- g. refusals and the batch form ---------------------------------------------------------------------------------------------
def test_the_batch_form_equals_the_device_form():
    S = vc.main_case()
    clouds, maps, m, _ = _branches()
    ctx = _ctx()
    try:
        for name, cl, mp, mm, exp in (("branches", clouds, maps, m, None), ("main", S["clouds"], S["maps"], S["m"], vc.main_expected("whole", 0.2, THREADS))):
            dev = _call(ctx, cl, mp, mm, bev_amd.icp_whole_defaults(), 0.2)
            host = ctx.submap_voxel_registration_batch(cl, *mp.arrays(), mm, 0.2, params=bev_amd.icp_whole_defaults())
            if exp is not None:
                _check(f"{name}: device form", dev, exp)
            _check(f"{name}: batch form", host, dev)
        host0 = ctx.submap_voxel_registration_batch(clouds, *maps.arrays(), m, 0.0, params=bev_amd.icp_whole_defaults())
        _check("batch form at map_leaf 0", host0, ctx.submap_registration_batch(clouds, *maps.arrays(), m, params=bev_amd.icp_whole_defaults()))
        assert len(ctx.submap_voxel_registration_batch(clouds, *maps.arrays(), m[:0], 0.2)) == 0
    finally:
        ctx.close()


def test_every_refused_argument_leaves_the_outputs_untouched():
    import torch

    lib = bev_amd.load_lib()
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    big = rc.scene(65536, 7001)                     # really allocated: 64 entries of it are a map of exactly 2^22 records
    small = rc.scene(200, 7002)
    clouds = [big, small]
    offs = _offsets(clouds)
    n_at = sc.REG_MAX_TARGET // len(big)
    maps = sc.Maps()
    maps.add([(1, sc.IDENTITY), (1, sc.shift(0.03))])
    maps.add([(1, sc.IDENTITY)])
    moffs, eframe, epose = maps.arrays()
    m = sc.matches([(1, 0, 0.0), (1, 1, 1.0)])
    prm = bev_amd.icp_whole_defaults()
    bad_prm = bev_amd.icp_params(max_iterations=0)
    STRIDE = 400
    ctx = _ctx()
    try:
        d_clouds = _dev(rc.packed(clouds))
        d_res = torch.full((len(m) * R,), 0xA5, dtype=torch.uint8, device=d_clouds.device)
        d_out = torch.full((2 * STRIDE * 16,), 0xA5, dtype=torch.uint8, device=d_clouds.device)
        d_cnt = torch.full((2 * 4,), 0xA5, dtype=torch.uint8, device=d_clouds.device)
        d_tab = torch.zeros(4 * R, dtype=torch.uint8, device=d_clouds.device)
        torch.cuda.synchronize()
        h, cl, res, tab = ctx._h, C.c_void_p(d_clouds.data_ptr()), C.c_void_p(d_res.data_ptr()), C.c_void_p(d_tab.data_ptr())
        out, cnt = C.c_void_p(d_out.data_ptr()), C.c_void_p(d_cnt.data_ptr())
        ptr = lambda a: a.ctypes.data if a is not None else None

        def call(n_frames=2, clouds_=cl, offs_=offs, leaf=0.2, map_leaf=0.2, n_maps=2, moffs_=moffs, eframe_=eframe, epose_=epose,
                 n_matches=2, m_=m, coarse=None, best=None, prm_=prm, res_=res):
            return lib.bev_submap_voxel_registration_device_resident(
                h, n_frames, clouds_, u64(offs_) if offs_ is not None else None, leaf, map_leaf, n_maps,
                u64(moffs_) if moffs_ is not None else None, ptr(eframe_), ptr(epose_), n_matches, ptr(m_),
                coarse, best, C.byref(prm_) if prm_ is not None else None, res_)

        def cloud(n_frames=2, clouds_=cl, offs_=offs, leaf=0.2, map_leaf=0.2, n_maps=2, moffs_=moffs, eframe_=eframe, epose_=epose,
                  stride=STRIDE, out_=out, cnt_=cnt):
            return lib.bev_submap_voxel_cloud_device_resident(
                h, n_frames, clouds_, u64(offs_) if offs_ is not None else None, leaf, map_leaf, n_maps,
                u64(moffs_) if moffs_ is not None else None, ptr(eframe_), ptr(epose_), stride, out_, cnt_)

        def other(a, k, v):
            a = a.copy()
            a[k] = v
            return a

        def match(k, field, v):
            mm = m.copy()
            mm[field][k] = v
            return mm

        one_more = sc.Maps()
        one_more.add([(0, sc.IDENTITY)] * (n_at + 1))
        one_more.add([(1, sc.IDENTITY)])
        too_many = np.array([0, bev_amd.SUBMAP_MAX_ENTRIES + 1, bev_amd.SUBMAP_MAX_ENTRIES + 2], np.uint64)
        nan, inf = float("nan"), float("inf")
        refused = {
            "n_frames < 0": (call(n_frames=-1), INVALID), "n_maps < 0": (call(n_maps=-1), INVALID),
            "n_matches < 0": (call(n_matches=-1), INVALID), "leaf 0": (call(leaf=0.0), INVALID), "leaf nan": (call(leaf=nan), INVALID),
            "map_leaf < 0": (call(map_leaf=-0.2), INVALID), "map_leaf nan": (call(map_leaf=nan), INVALID),
            "map_leaf inf": (call(map_leaf=inf), INVALID), "map_leaf -inf": (call(map_leaf=-inf), INVALID),
            "params": (call(prm_=bad_prm), INVALID), "coarse without best": (call(coarse=tab), INVALID),
            "best without coarse": (call(best=tab), INVALID), "NULL clouds": (call(clouds_=None), INVALID),
            "NULL matches": (call(m_=None), INVALID), "NULL results": (call(res_=None), INVALID),
            "NULL map offsets": (call(moffs_=None), INVALID), "NULL entry frames": (call(eframe_=None), INVALID),
            "NULL entry poses": (call(epose_=None), INVALID),
            "decreasing frame offsets": (call(offs_=np.array([0, 70000, 65536], np.uint64)), INVALID),
            "decreasing map offsets": (call(moffs_=np.array([0, 5, 3], np.uint64)), INVALID),
            "entry frame 2": (call(eframe_=other(eframe, 1, 2)), INVALID), "entry frame -1": (call(eframe_=other(eframe, 2, -1)), INVALID),
            "query 2": (call(m_=match(0, "query_idx", 2)), INVALID), "query -1": (call(m_=match(1, "query_idx", -1)), INVALID),
            "map 2": (call(m_=match(1, "match_idx", 2)), INVALID), "map -1": (call(m_=match(0, "match_idx", -1)), INVALID),
            "a frame as match_idx of fewer maps": (call(n_maps=1), INVALID),
            "too many entries (arrays not read)": (call(moffs_=too_many), TOO_LARGE),
            "a map one frame above the target bound": (call(moffs_=one_more.arrays()[0], eframe_=one_more.arrays()[1],
                                                            epose_=one_more.arrays()[2]), TOO_LARGE),
            "cloud: n_frames < 0": (cloud(n_frames=-1), INVALID), "cloud: n_maps < 0": (cloud(n_maps=-1), INVALID),
            "cloud: leaf 0": (cloud(leaf=0.0), INVALID), "cloud: map_leaf < 0": (cloud(map_leaf=-1.0), INVALID),
            "cloud: map_leaf nan": (cloud(map_leaf=nan), INVALID), "cloud: map_leaf inf": (cloud(map_leaf=inf), INVALID),
            "cloud: NULL clouds": (cloud(clouds_=None), INVALID), "cloud: NULL out": (cloud(out_=None), INVALID),
            "cloud: NULL counts": (cloud(cnt_=None), INVALID), "cloud: NULL map offsets": (cloud(moffs_=None), INVALID),
            "cloud: NULL entry frames": (cloud(eframe_=None), INVALID), "cloud: NULL entry poses": (cloud(epose_=None), INVALID),
            "cloud: decreasing map offsets": (cloud(moffs_=np.array([0, 5, 3], np.uint64)), INVALID),
            "cloud: entry frame 2": (cloud(eframe_=other(eframe, 1, 2)), INVALID),
            "cloud: a stride one record short": (cloud(stride=2 * len(small) - 1), INVALID),
            "cloud: too many entries": (cloud(moffs_=too_many), TOO_LARGE),
            "cloud: a map one frame above the target bound": (cloud(stride=1 << 23, moffs_=one_more.arrays()[0], eframe_=one_more.arrays()[1],
                                                                   epose_=one_more.arrays()[2]), TOO_LARGE),
        }
        ctx.synchronize()
        wrong = {k: v for k, v in refused.items() if v[0] != v[1]}
        assert not wrong, wrong
        untouched = lambda: all((d.cpu().numpy() == 0xA5).all() for d in (d_res, d_out, d_cnt))
        assert untouched(), "a refused call wrote an output"
        assert call(n_matches=0, m_=None, res_=None, clouds_=None) == OK
        assert cloud(n_maps=0, clouds_=None, moffs_=None, eframe_=None, epose_=None, out_=None, cnt_=None) == OK
        ctx.synchronize()
        assert untouched()
        # and the accepted calls, the stride exactly the largest capacity
        assert call() == OK and cloud(stride=2 * len(small)) == OK
        ctx.synchronize()
        _check("accepted", _results(d_res), vc.expected(clouds, maps, m, fl.params(**fl.WHOLE), 0.2, threads=2))
        tg = vc.targets(clouds, maps, [0, 1], 0.2, threads=2)
        assert d_cnt.cpu().numpy().view(np.uint32).tolist() == [len(tg[0][1]), len(tg[1][1])]
    finally:
        ctx.close()


# ---- h. status precedence ---------------------------------------------------------------------------------------------------------
def test_status_precedence_of_calls_wrong_in_two_ways():
    """Every scan-to-map entry keeps its own order of checks: a call with two faults gets the status of the
    check that comes first.  Nothing is launched; every output stays as it was filled."""
    import torch

    lib = bev_amd.load_lib()
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    ptr = lambda a: a.ctypes.data if a is not None else None
    big, small = rc.scene(65536, 7001), rc.scene(200, 7002)
    clouds = [big, small]
    offs = _offsets(clouds)
    maps = sc.Maps()
    maps.add([(1, sc.IDENTITY), (1, sc.shift(0.03))])
    maps.add([(1, sc.IDENTITY)])
    moffs, eframe, epose = maps.arrays()
    m = sc.matches([(1, 0, 0.0), (1, 1, 1.0)])
    prm = bev_amd.icp_whole_defaults()
    above = sc.Maps()                                   # map 0: one frame above BEV_SUBMAP_REG_MAX_TARGET records, and (at a
    above.add([(0, sc.IDENTITY)] * (sc.REG_MAX_TARGET // len(big) + 1))   # stride of 65,536) above BEV_SUBMAP_COARSE_MAX_TARGET rows
    above.add([(1, sc.IDENTITY)])
    a_offs, a_frame, a_pose = above.arrays()
    too_many = np.array([0, bev_amd.SUBMAP_MAX_ENTRIES + 1, bev_amd.SUBMAP_MAX_ENTRIES + 2], np.uint64)
    decreasing = np.array([0, 70000, 65536], np.uint64)
    STRIDE, PN_STRIDE = 2 * len(small), len(big)

    def match(k, field, v):
        mm = m.copy()
        mm[field][k] = v
        return mm

    ctx = _ctx()
    try:
        dev = torch.device("cuda:0")
        d_clouds = _dev(rc.packed(clouds))
        filled = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
        d_res, d_out, d_cnt, d_cres, d_cbest = filled(len(m) * R), filled(2 * STRIDE * 16), filled(2 * 4), filled(len(m) * 2 * R), filled(len(m) * 4)
        d_pn, d_pcnt = torch.zeros(2 * PN_STRIDE * 48, dtype=torch.uint8, device=dev), _dev(np.array([len(big), len(small)], np.uint32))
        h_res = np.full(len(m) * R, 0xA5, np.uint8)
        torch.cuda.synchronize()
        h, cl = ctx._h, C.c_void_p(d_clouds.data_ptr())
        vp = lambda d: C.c_void_p(d.data_ptr()) if d is not None else None

        def reg(clouds_=cl, offs_=offs, moffs_=moffs, eframe_=eframe, epose_=epose, m_=m):
            return lib.bev_submap_voxel_registration_device_resident(h, 2, clouds_, u64(offs_), 0.2, 0.2, 2, u64(moffs_), ptr(eframe_),
                                                                     ptr(epose_), 2, ptr(m_), None, None, C.byref(prm), vp(d_res))

        def cloud(clouds_=cl, moffs_=moffs, eframe_=eframe, epose_=epose, stride=STRIDE, out_=d_out):
            return lib.bev_submap_voxel_cloud_device_resident(h, 2, clouds_, u64(offs), 0.2, 0.2, 2, u64(moffs_), ptr(eframe_), ptr(epose_),
                                                              stride, vp(out_), vp(d_cnt))

        def coarse(stride=PN_STRIDE, moffs_=moffs, eframe_=eframe, epose_=epose, m_=m):
            return lib.bev_submap_coarse_registration_device_resident(h, 2, vp(d_pn), stride, vp(d_pcnt), 2, u64(moffs_), ptr(eframe_),
                                                                      ptr(epose_), 2, ptr(m_), None, vp(d_cres), vp(d_cbest))

        def batch(moffs_=moffs):
            pts = (C.c_void_p * 2)(big.ctypes.data, None)            # frame 1: 200 records at NULL
            npts = np.array([len(big), len(small)], np.uint32)
            return lib.bev_submap_voxel_registration_batch(h, 2, pts, npts.ctypes.data_as(C.POINTER(C.c_uint32)), 0.2, 0.2, 2, u64(moffs_),
                                                           ptr(eframe), ptr(epose), 2, ptr(m), C.byref(prm), h_res.ctypes.data)

        got = {
            "reg: a map above the target bound, NULL clouds": (reg(clouds_=None, moffs_=a_offs, eframe_=a_frame, epose_=a_pose), TOO_LARGE),
            "reg: query 2, a map above the target bound": (reg(m_=match(0, "query_idx", 2), moffs_=a_offs, eframe_=a_frame, epose_=a_pose), INVALID),
            "reg: decreasing frame offsets, too many entries": (reg(offs_=decreasing, moffs_=too_many), INVALID),
            "reg: too many entries, map 2": (reg(moffs_=too_many, m_=match(1, "match_idx", 2)), TOO_LARGE),
            "reg: NULL matches, too many entries": (reg(m_=None, moffs_=too_many), INVALID),
            "cloud: a map above the target bound, a stride one record short": (cloud(moffs_=a_offs, eframe_=a_frame, epose_=a_pose, stride=STRIDE - 1), TOO_LARGE),
            "cloud: too many entries, NULL clouds": (cloud(moffs_=too_many, clouds_=None), TOO_LARGE),
            "cloud: NULL out, too many entries": (cloud(out_=None, moffs_=too_many), INVALID),
            "coarse: too many entries, map 2": (coarse(moffs_=too_many, m_=match(1, "match_idx", 2)), TOO_LARGE),
            "coarse: map 2, a capacity above the bound": (coarse(m_=match(1, "match_idx", 2), moffs_=a_offs, eframe_=a_frame, epose_=a_pose), INVALID),
            "coarse: stride 0, too many entries": (coarse(stride=0, moffs_=too_many), INVALID),
            "batch: a NULL cloud of 200 records, too many entries": (batch(moffs_=too_many), INVALID),
        }
        ctx.synchronize()
        wrong = {k: v for k, v in got.items() if v[0] != v[1]}
        assert not wrong, wrong
        assert all((d.cpu().numpy() == 0xA5).all() for d in (d_res, d_out, d_cnt, d_cres, d_cbest)) and (h_res == 0xA5).all(), \
            "a refused call wrote an output"
        # each fault alone is the existing tests'; the faults of a pair do not depend on each other
        assert coarse(moffs_=a_offs, eframe_=a_frame, epose_=a_pose) == TOO_LARGE and cloud(stride=STRIDE - 1) == INVALID
    finally:
        ctx.close()
