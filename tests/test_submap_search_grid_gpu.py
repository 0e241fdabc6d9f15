"""GPU: the scan-to-map search grids sized to the map (bev_set_submap_search_grid, bev_debug_get_submap_grid).
The results do not depend on the grid, so every call is compared byte for byte, as whole bev_icp_result_t records, with the
existing sequential checkers and with the call at D = 0; the hook says which grid was really built, so a library that ignored the
setter would not pass.  The cases are submap_grid_cases.py's: the smallest targets that cross the fixed caps.

  1. fine, unthinned: 18 000 points (ceil(sqrt) = 135 > 128) at D = 0, 8, 128, 130, 256, 1024, both tools' settings;
  2. fine, thinned at map_leaf 0.2 and 0.5, D = 0, 130, 256;
  3. coarse: 5 400 rows (ceil(sqrt) = 74 > 64) at D = 0, 4, 64, 70, 256: unthinned, thinned, and the top-part-union call;
  4. ties: the mirror ties of both stages and a frame twice under one pose, D = 256;
  5. degenerate targets at D = 256;
  6. four maps of 1, 300, 5 400 and 18 000 points and an unused one, in one launch group and in three or more;
  7. ordering: a D = 0 call, the setter, the same call again, no synchronisation between;
  and the setter's refusals on a live context.
"""
import os

import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import icp_lib
import reg_cases as rc
import regfront_lib as rf
import submap_coarse_cases as cc
import submap_grid_cases as gc
import submap_pn_vox_cases as pv
import submap_reg_cases as sc
import submap_top_cases as tc
import submap_vox_cases as vc
from bev_amd import ICP_RESULT_DTYPE
from submap_reg_gpu_lib import R, THREADS, _check, _ctx, _dev, _offsets, _results, _same
from submap_reg_gpu_lib import _fine_call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _checkers():
    icp_lib.build()
    fl.build()
    rf.build()


@pytest.fixture(scope="module")
def ctx():
    c = _ctx(max_points=4096)
    yield c
    c.set_submap_search_grid(0, 0)
    c.close()


def _check2(name, got, exp):
    """got, exp: ((n, 2) results, (n,) best)"""
    (gr, gb), (er, eb) = got, exp
    _check(name, np.asarray(gr).reshape(-1), np.asarray(er).reshape(-1))
    assert np.array_equal(np.asarray(gb), np.asarray(eb)), f"{name}: best differs"


def _outputs(n, fill=0):
    import torch

    dev = torch.device("cuda:0")
    return (torch.full((max(n, 1) * 2 * R,), fill, dtype=torch.uint8, device=dev),
            torch.full((max(n, 1) * 4,), fill, dtype=torch.uint8, device=dev))


def _read(d_res, d_best, n):
    return d_res.cpu().numpy().view(ICP_RESULT_DTYPE).reshape(-1, 2)[:n], d_best.cpu().numpy().view(np.int32)[:n]


def _coarse_call(ctx, frames, stride, maps, m, leaf=0.0):
    import torch

    d_pn, d_cnt = _dev(rc.strided(frames, stride)), _dev(np.array([len(f) for f in frames], np.uint32))
    d_res, d_best = _outputs(len(m))
    torch.cuda.synchronize()
    if leaf:
        ctx.submap_coarse_voxel_registration_device(len(frames), d_pn.data_ptr(), stride, d_cnt.data_ptr(), *maps.arrays(), m,
                                                    d_res.data_ptr(), d_best.data_ptr(), leaf)
    else:
        ctx.submap_coarse_registration_device(len(frames), d_pn.data_ptr(), stride, d_cnt.data_ptr(), *maps.arrays(), m,
                                              d_res.data_ptr(), d_best.data_ptr())
    ctx.synchronize()
    return _read(d_res, d_best, len(m))


def _top_call(ctx, clouds, pn, maps, m, leaf):
    import torch

    stride = max(1, max(len(p) for p in pn))
    d_clouds, d_pn = _dev(rc.packed(clouds)), _dev(rc.strided(pn, stride))
    d_cnt = _dev(np.array([len(p) for p in pn], np.uint32))
    d_res, d_best = _outputs(len(m))
    torch.cuda.synchronize()
    ctx.submap_top_part_coarse_registration_device(len(clouds), d_clouds.data_ptr(), _offsets(clouds), d_pn.data_ptr(), stride,
                                                   d_cnt.data_ptr(), *maps.arrays(), m, d_res.data_ptr(), d_best.data_ptr(), leaf)
    ctx.synchronize()
    return _read(d_res, d_best, len(m))


def _fine(ctx, S, settings, map_leaf):
    if settings == "whole":
        return _fine_call(ctx, S["clouds"], S["maps"], S["m"], bev_amd.icp_whole_defaults(), map_leaf)
    return _fine_call(ctx, S["clouds"], S["maps"], S["m"], None, map_leaf, None, S["coarse"], S["best"])


def _fine_expected(S, settings, map_leaf):
    if settings == "whole":
        return vc.expected(S["clouds"], S["maps"], S["m"], fl.params(**fl.WHOLE), map_leaf, threads=THREADS)
    return vc.expected(S["clouds"], S["maps"], S["m"], fl.params(**fl.FINE), map_leaf, S["guesses"], threads=THREADS)


# ---- 1. fine, unthinned --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("settings", ["whole", "top"])
def test_fine_unthinned_results_do_not_depend_on_the_grid(ctx, settings):
    S = gc.fine_case()
    exp = _fine_expected(S, settings, 0.0)
    assert exp["converged"].sum() >= 3 and (exp["state"] != bev_amd.ICP_NO_CORRESPONDENCES).sum() >= 3
    largest = {}
    for D in (0, 8, 128, 130, 256, 1024):
        ctx.set_submap_search_grid(D, 0)
        got = _fine(ctx, S, settings, None if D == 0 else 0.0)     # D = 0 through the entry without a second grid
        nx, ny, n, cell = (int(v) for v in ctx.debug_submap_grid(0, 0, 1)[0])
        print(f"{settings} D {D}: grid {nx} x {ny}, {n} searchable, largest cell {cell}")
        _check(f"{settings} at D {D}", got, exp)
        assert n == S["n"]
        assert max(nx, ny) == min(D, 135) if D else max(nx, ny) <= gc.FINE_CAP, (D, nx, ny)
        largest[D] = cell
    wide = [largest[D] for D in (8, 128, 130, 256, 1024)]
    assert all(a >= b for a, b in zip(wide, wide[1:])), wide                # a finer grid holds no fuller cell
    assert largest[256] == largest[1024] and largest[8] > 20 * largest[256], largest


# ---- 2. fine, thinned ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("map_leaf", [0.2, 0.5])
def test_fine_thinned_results_do_not_depend_on_the_grid(ctx, map_leaf):
    S = gc.fine_case()
    exp = _fine_expected(S, "whole", map_leaf)
    n_thin = len(vc.targets(S["clouds"], S["maps"], [0], map_leaf, threads=THREADS)[0][1])
    assert n_thin < S["n"] and (exp["state"] != bev_amd.ICP_NO_CORRESPONDENCES).sum() >= 3
    for D in (0, 130, 256):
        ctx.set_submap_search_grid(D, 0)
        got = _fine(ctx, S, "whole", map_leaf)
        nx, ny, n, cell = (int(v) for v in ctx.debug_submap_grid(0, 0, 1)[0])
        print(f"map_leaf {map_leaf} D {D}: {n_thin} thinned points, grid {nx} x {ny}, largest cell {cell}")
        _check(f"map_leaf {map_leaf} at D {D}", got, exp)
        assert n == n_thin
        assert max(nx, ny) == gc.grid_dim(n_thin, D if D else gc.FINE_CAP), (D, nx, ny)


# ---- 3. coarse -----------------------------------------------------------------------------------------------------------------
COARSE_DIMS = (0, 4, 64, 70, 256)


def test_coarse_unthinned_results_do_not_depend_on_the_grid(ctx):
    S = gc.coarse_case()
    exp = cc.expected(S["frames"], S["maps"], S["m"], None, S["stride"], threads=THREADS)
    assert cc.condition_share(exp[0]) == 1.0
    for D in COARSE_DIMS:
        ctx.set_submap_search_grid(0, D)
        got = _coarse_call(ctx, S["frames"], S["stride"], S["maps"], S["m"])
        nx, ny, n, cell = (int(v) for v in ctx.debug_submap_grid(1, 0, 1)[0])
        print(f"coarse D {D}: grid {nx} x {ny}, {n} searchable, largest cell {cell}")
        _check2(f"coarse at D {D}", got, exp)
        assert n == S["n"] and max(nx, ny) == gc.grid_dim(S["n"], D if D else gc.COARSE_CAP), (D, nx, ny, n)


def test_coarse_thinned_results_do_not_depend_on_the_grid(ctx):
    S = gc.coarse_case()
    leaf = 0.5
    exp = pv.expected(S["frames"], S["maps"], S["m"], leaf, stride=S["stride"], threads=THREADS)
    n_thin = len(pv.target(S["frames"], S["maps"].entries(0), S["stride"], leaf))
    for D in COARSE_DIMS:
        ctx.set_submap_search_grid(0, D)
        got = _coarse_call(ctx, S["frames"], S["stride"], S["maps"], S["m"], leaf)
        nx, ny, n, cell = (int(v) for v in ctx.debug_submap_grid(1, 0, 1)[0])
        print(f"coarse thinned D {D}: {n_thin} rows, grid {nx} x {ny}, largest cell {cell}")
        _check2(f"coarse thinned at D {D}", got, exp)
        assert n == n_thin and max(nx, ny) == gc.grid_dim(n_thin, D if D else gc.COARSE_CAP), (D, nx, ny, n)


def test_top_part_union_results_do_not_depend_on_the_grid(ctx):
    S = gc.top_case()
    leaf = 0.2
    exp = tc.expected(S["pn"], S["clouds"], S["maps"], S["m"], leaf, threads=THREADS)
    n_rows = len(tc.target(S["clouds"], S["maps"].entries(0), leaf))
    for D in COARSE_DIMS:
        ctx.set_submap_search_grid(0, D)
        got = _top_call(ctx, S["clouds"], S["pn"], S["maps"], S["m"], leaf)
        nx, ny, n, cell = (int(v) for v in ctx.debug_submap_grid(1, 0, 1)[0])
        print(f"top union D {D}: {n_rows} rows, grid {nx} x {ny}, largest cell {cell}")
        _check2(f"top union at D {D}", got, exp)
        assert n == n_rows and max(nx, ny) == gc.grid_dim(n_rows, D if D else gc.COARSE_CAP), (D, nx, ny, n)


# ---- 4. ties -------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lowest_index_whatever_the_order_inside_a_cell(ctx):
    clouds, maps, m = sc.mirror_tie()
    twice = sc.Maps()
    twice.add([(0, sc.planar(0.5, 0.05, 0.0)), (0, sc.planar(0.5, 0.05, 0.0))])        # every distance ties
    m2 = sc.matches([(1, 0, 0.0), (0, 0, 0.5)])
    for name, prm in (("whole", fl.params(**fl.WHOLE)), ("top-part", fl.params(**fl.FINE))):
        exp = sc.expected(clouds, maps, m, prm, threads=THREADS)
        assert not _same(exp[0], exp[1])                                                # the entry order decides
        exp2 = sc.expected(clouds, twice, m2, prm, threads=THREADS)
        for D in (0, 256):
            ctx.set_submap_search_grid(D, D)
            _check(f"fine mirror tie, {name}, D {D}", _fine_call(ctx, clouds, maps, m, prm, 0.0), exp)
            _check(f"a frame twice, {name}, D {D}", _fine_call(ctx, clouds, twice, m2, prm, 0.0), exp2)
    frames, cmaps, cm = cc.mirror_tie()
    cexp = cc.expected(frames, cmaps, cm, None, 400, threads=THREADS)
    assert not _same(cexp[0][0], cexp[0][1])
    ctwice = sc.Maps()
    ctwice.add([(0, sc.planar(0.5, 0.05, 0.0)), (0, sc.planar(0.5, 0.05, 0.0))])
    cexp2 = cc.expected(frames, ctwice, m2, None, 400, threads=THREADS)
    for D in (0, 256):
        ctx.set_submap_search_grid(D, D)
        _check2(f"coarse mirror tie, D {D}", _coarse_call(ctx, frames, 400, cmaps, cm), cexp)
        _check2(f"coarse, a frame twice, D {D}", _coarse_call(ctx, frames, 400, ctwice, m2), cexp2)


# ---- 5. degenerate targets -----------------------------------------------------------------------------------------------------
def test_degenerate_targets(ctx):
    clouds, maps, m, names = gc.degenerate_case()
    prm = fl.params(**fl.WHOLE)
    exp = sc.expected(clouds, maps, m, prm, threads=THREADS)
    assert (exp["state"][:2] == bev_amd.ICP_NO_CORRESPONDENCES).all() and exp["state"][5] == bev_amd.ICP_NO_CORRESPONDENCES
    for D in (0, 256):
        ctx.set_submap_search_grid(D, D)
        _check(f"degenerate fine targets, D {D}", _fine_call(ctx, clouds, maps, m, prm, 0.0), exp)
        grids = ctx.debug_submap_grid(0, 0, len(maps)).tolist()                   # every map is named: the plan's order is theirs
        print(f"D {D}: {dict(zip(names, grids))}")
        assert grids[names["none"]] == [1, 1, 0, 0] and grids[names["non_finite"]] == [1, 1, 0, 0]
        assert grids[names["one_point"]] == [1, 1, 1, 1]
        assert grids[names["collinear"]][1] == 1 and grids[names["collinear"]][2] == 200
        assert grids[names["collinear"]][0] == gc.grid_dim(200, D if D else gc.FINE_CAP)
    frames, stride, cmaps, cm = gc.clump_case()
    cexp = cc.expected(frames, cmaps, cm, None, stride, threads=THREADS)
    for D in (0, 256):
        ctx.set_submap_search_grid(D, D)
        _check2(f"degenerate coarse targets, D {D}", _coarse_call(ctx, frames, stride, cmaps, cm), cexp)
        grids = ctx.debug_submap_grid(1, 0, 3).tolist()
        print(f"coarse D {D}: {grids}")
        assert grids[0][2] == 4001 and grids[0][3] == 4000 and grids[0][1] == 1     # one cell holds the clump
        assert grids[1] == [1, 1, 1, 1] and grids[2] == [1, 1, 0, 0]


# ---- 6. groups and bases -------------------------------------------------------------------------------------------------------
def test_maps_of_different_sizes_in_one_group_and_in_several():
    clouds, maps, m, caps = gc.groups_case()
    prm = fl.params(**fl.WHOLE)
    exp = sc.expected(clouds, maps, m, prm, threads=THREADS)
    D, group_bytes = 256, 100000
    one, last_one = gc.fine_group_count(caps, D, 8 << 30)
    cut, last_cut = gc.fine_group_count(caps, D, group_bytes)
    assert one == 1 and last_one == 4 and cut >= 3, (one, cut)
    saved = os.environ.get("BEV_SUBMAP_REG_GROUP")
    try:
        for cap, groups, last in ((None, one, last_one), (str(group_bytes), cut, last_cut)):
            if cap is None:
                os.environ.pop("BEV_SUBMAP_REG_GROUP", None)
            else:
                os.environ["BEV_SUBMAP_REG_GROUP"] = cap
            c = _ctx(max_points=4096)
            try:
                c.set_submap_search_grid(D, 0)
                c.profile_enable(True)
                got = _fine_call(c, clouds, maps, m, prm, 0.0)
                launches = {k["name"]: k["launches"] for k in c.profile_get()}
                grids = c.debug_submap_grid(0, 0, last).tolist()
                with pytest.raises(bev_amd.BevError):
                    c.debug_submap_grid(0, 0, last + 1)                            # outside the last group
            finally:
                c.close()
            _check(f"group cap {cap}", got, exp)
            print(f"group cap {cap}: {groups} groups, the last group's grids {grids}")
            assert launches["k_subgrid_scan"] == launches["k_submap_vox_move"] == groups, launches
            assert "k_submap_target" not in launches and "k_submap_icp" not in launches and launches["k_submap_icp_wide"] >= groups
            used = caps[len(caps) - last:]
            assert [g[2] for g in grids] == list(used)
            assert [max(g[0], g[1]) for g in grids] == [gc.grid_dim(n, D) for n in used]
    finally:
        if saved is None:
            os.environ.pop("BEV_SUBMAP_REG_GROUP", None)
        else:
            os.environ["BEV_SUBMAP_REG_GROUP"] = saved


# ---- 7. ordering and the setter's refusals -------------------------------------------------------------------------------------
def test_the_setter_needs_no_synchronisation(ctx):
    import torch

    S = gc.fine_case()
    exp = _fine_expected(S, "whole", 0.0)
    d_clouds = _dev(rc.packed(S["clouds"]))
    d_a, d_b = (torch.zeros(len(S["m"]) * R, dtype=torch.uint8, device=d_clouds.device) for _ in range(2))
    call = lambda d: ctx.submap_voxel_registration_device(len(S["clouds"]), d_clouds.data_ptr(), _offsets(S["clouds"]),
                                                          *S["maps"].arrays(), S["m"], d.data_ptr(), 0.0,
                                                          params=bev_amd.icp_whole_defaults())
    ctx.set_submap_search_grid(0, 0)
    torch.cuda.synchronize()
    call(d_a)
    ctx.set_submap_search_grid(256, 0)
    call(d_b)
    ctx.synchronize()
    _check("the call before the setter", _results(d_a), exp)
    _check("the call behind the setter", _results(d_b), exp)
    assert max(ctx.debug_submap_grid(0, 0, 1)[0][:2]) == 135


def test_the_setter_refuses_values_outside_its_range_and_changes_nothing(ctx):
    S = gc.fine_case()
    ctx.set_submap_search_grid(130, 70)
    for fine, coarse in ((-1, 0), (0, -1), (1025, 0), (0, 1025), (-1, 1025)):
        with pytest.raises(bev_amd.BevError):
            ctx.set_submap_search_grid(fine, coarse)
    _fine(ctx, S, "whole", 0.0)
    assert max(ctx.debug_submap_grid(0, 0, 1)[0][:2]) == 130
    with pytest.raises(bev_amd.BevError):
        ctx.debug_submap_grid(2, 0, 1)
    with pytest.raises(bev_amd.BevError):
        ctx.debug_submap_grid(0, 1, 1)
    fresh = _ctx(max_points=4096)
    try:
        with pytest.raises(bev_amd.BevError):
            fresh.debug_submap_grid(0, 0, 0)                                     # before any such call
    finally:
        fresh.close()
