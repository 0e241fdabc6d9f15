"""GPU: the launches of the registration calls with and without search grids sized to the target, and the contracts of the two
test hooks (bev_debug_get_pair_grid, bev_debug_get_submap_grid).

The host paths of §6s and §6t share one driver of the grid's build, one record and one reader of the hooks.  What the device is
given must not change with that: with profiling on, every family of calls below is run once at cap 0 and once at cap 8 on
three small frames, two maps of 1 and 2 entries and two matches, and bev_profile_get's launch and frame counts per kernel are
compared with EXPECTED, a table recorded from the commit BEFORE the fold.  The scan-to-map families also run with
BEV_SUBMAP_REG_GROUP = 1 byte, which puts each map into a launch group of its own, so that the per-group loop runs twice.
"""
import os

import numpy as np
import pytest

import bev_amd
import reg_cases as rc
import submap_coarse_cases as cc
import submap_reg_cases as sc
import submap_top_cases as tc
import submap_vox_cases as vc
from submap_reg_gpu_lib import R, _ctx, _dev, _fine_call, _offsets

pytestmark = pytest.mark.gpu
SIZES = (900, 600, 300)
CAPS = (0, 8)
STRIDE = 900
INVALID_ARG = r"\(status -1\)"                             # BEV_ERR_INVALID_ARG, as BevContext words a refusal


def _maps():
    maps = sc.Maps()
    maps.add([(0, sc.IDENTITY)])
    maps.add([(1, sc.planar(1.0, 0.2, -0.1)), (2, sc.planar(-0.5, 0.1, 0.1))])
    return maps


MATCHES = sc.matches([(2, 0, 0.3), (0, 1, -0.5)])          # frame against frame, or frame against map
CLOUDS = [vc.lattice(n, 830 + k) for k, n in enumerate(SIZES)]                 # the fine stage's records
ROWS = [cc.frame(n, 9830 + k) for k, n in enumerate(SIZES)]                    # the coarse stage's PointNormal rows
FULL = [tc.wall_cloud(n, 9930 + k) for k, n in enumerate(SIZES)]               # full labelled clouds (the top part's unions)


def _coarse_outputs():
    import torch

    dev = torch.device("cuda:0")
    return torch.zeros(len(MATCHES) * 2 * R, dtype=torch.uint8, device=dev), torch.zeros(len(MATCHES), dtype=torch.int32, device=dev)


def pair_fine(ctx):
    import torch

    d_clouds = _dev(rc.packed(CLOUDS))
    d_res = torch.zeros(len(MATCHES) * R, dtype=torch.uint8, device=d_clouds.device)
    torch.cuda.synchronize()
    ctx.fine_registration_device(len(CLOUDS), d_clouds.data_ptr(), _offsets(CLOUDS), MATCHES, d_res.data_ptr(),
                                 params=bev_amd.icp_whole_defaults())
    ctx.synchronize()


def pair_coarse(ctx):
    import torch

    d_pn, d_cnt = _dev(rc.strided(ROWS, STRIDE)), _dev(np.array(SIZES, np.uint32))
    d_res, d_best = _coarse_outputs()
    torch.cuda.synchronize()
    ctx.coarse_registration_device(len(ROWS), d_pn.data_ptr(), STRIDE, d_cnt.data_ptr(), MATCHES, d_res.data_ptr(), d_best.data_ptr())
    ctx.synchronize()


def _submap_fine(ctx, map_leaf):
    _fine_call(ctx, CLOUDS, _maps(), MATCHES, bev_amd.icp_whole_defaults(), map_leaf)


def _submap_coarse(ctx, leaf):
    import torch

    d_pn, d_cnt = _dev(rc.strided(ROWS, STRIDE)), _dev(np.array(SIZES, np.uint32))
    d_res, d_best = _coarse_outputs()
    torch.cuda.synchronize()
    if leaf:
        ctx.submap_coarse_voxel_registration_device(len(ROWS), d_pn.data_ptr(), STRIDE, d_cnt.data_ptr(), *_maps().arrays(), MATCHES,
                                                    d_res.data_ptr(), d_best.data_ptr(), leaf)
    else:
        ctx.submap_coarse_registration_device(len(ROWS), d_pn.data_ptr(), STRIDE, d_cnt.data_ptr(), *_maps().arrays(), MATCHES,
                                              d_res.data_ptr(), d_best.data_ptr())
    ctx.synchronize()


def submap_top(ctx):
    """the queries are any PointNormal rows: the launches do not depend on them"""
    import torch

    d_clouds, d_pn, d_cnt = _dev(rc.packed(FULL)), _dev(rc.strided(ROWS, STRIDE)), _dev(np.array(SIZES, np.uint32))
    d_res, d_best = _coarse_outputs()
    torch.cuda.synchronize()
    ctx.submap_top_part_coarse_registration_device(len(FULL), d_clouds.data_ptr(), _offsets(FULL), d_pn.data_ptr(), STRIDE,
                                                   d_cnt.data_ptr(), *_maps().arrays(), MATCHES, d_res.data_ptr(), d_best.data_ptr(), 0.2)
    ctx.synchronize()


PAIR = {"pair fine": pair_fine, "pair coarse": pair_coarse}
SUBMAP = {"submap fine": lambda c: _submap_fine(c, 0.0), "submap fine thinned": lambda c: _submap_fine(c, 0.5),
          "submap coarse": lambda c: _submap_coarse(c, 0.0), "submap coarse thinned": lambda c: _submap_coarse(c, 0.5),
          "submap top": submap_top}
# (family, cap, launch groups) of every recorded call
CASES = [(f, D, 1) for f in PAIR for D in CAPS] + [(f, D, g) for f in SUBMAP for D in CAPS for g in (1, 2)]


def profile(ctx):
    """{kernel: (launches, frames)} since the last reset; every kernel, where BevContext.profile_get stops at sixteen"""
    arr = (bev_amd.KernelStat * 64)()
    n = ctx.lib.bev_profile_get(ctx._h, arr, 64)
    assert 0 <= n <= 64, n
    return {arr[i].name.decode(): (int(arr[i].launches), int(arr[i].frames)) for i in range(n)}


def launches_of(ctx, family, D):
    ctx.set_pair_search_grid(D, D)
    ctx.set_submap_search_grid(D, D)
    ctx.profile_reset()
    {**PAIR, **SUBMAP}[family](ctx)
    return profile(ctx)


def context(groups):
    """a profiling context whose scan-to-map calls put their two maps into `groups` launch groups"""
    saved = os.environ.get("BEV_SUBMAP_REG_GROUP")
    try:
        if groups == 2:
            os.environ["BEV_SUBMAP_REG_GROUP"] = "1"
        else:
            os.environ.pop("BEV_SUBMAP_REG_GROUP", None)
        c = _ctx(max_points=4096)
    finally:
        if saved is None:
            os.environ.pop("BEV_SUBMAP_REG_GROUP", None)
        else:
            os.environ["BEV_SUBMAP_REG_GROUP"] = saved
    c.profile_enable(True)
    return c


@pytest.fixture(scope="module")
def contexts():
    cs = {g: context(g) for g in (1, 2)}
    yield cs
    for c in cs.values():
        c.close()


BUILD = ("k_subgrid_bounds", "k_subgrid_header", "k_subgrid_count", "k_subgrid_sums", "k_subgrid_scan", "k_subgrid_scatter")


def _expected():
    """{(family, cap, groups): {kernel: (launches, frames)}}, from a run of the commit before the fold.  A
    kernel that runs per launch group counts the group's maps as its frames, an ICP kernel its problems (coarse: two per match)"""
    fine, best = {"k_fine_voxel": (1, 3)}, {"k_icp_best": (1, 2)}
    t = {("pair fine", 0, 1): {**fine, "k_fine_grid": (1, 3), "k_fine_icp": (1, 2)},
         ("pair fine", 8, 1): {**fine, "k_pairgrid_desc": (1, 2), **{k: (1, 2) for k in BUILD}, "k_fine_icp_wide": (1, 2)},
         ("pair coarse", 0, 1): {**best, "k_icp_grid": (1, 2), "k_icp": (1, 4)},
         ("pair coarse", 8, 1): {**best, "k_pairgrid_desc": (1, 2), **{k: (1, 2) for k in BUILD}, "k_icp_wide": (1, 4)}}
    for g in (1, 2):
        def per(*names):
            return {k: (g, 2) for k in names}

        thin = per("k_submap_vox_move", "k_submap_vox_keys", "k_submap_vox_tile", "k_submap_vox_finish")
        pn_thin = per("k_submap_vox_tile", "k_submap_pn_move", "k_submap_pn_keys", "k_submap_pn_finish", "k_submap_pn_normals")
        top = {**per("k_submap_top_keys", "k_submap_top_cells", "k_submap_top_compact", "k_submap_top_rows", "k_submap_pn_keys",
                     "k_submap_pn_finish", "k_submap_top_overflow", "k_submap_pn_normals"),
               "k_submap_vox_tile": (2 * g, 4), "k_submap_top_hist": (10 * g, 20), "k_submap_top_scan": (10 * g, 20)}
        t["submap fine", 0, g] = {**fine, **per("k_submap_target", "k_submap_icp")}
        t["submap fine", 8, g] = {**fine, **per("k_submap_vox_move", *BUILD, "k_submap_icp_wide")}
        t["submap fine thinned", 0, g] = {**fine, **thin, **per("k_submap_icp")}
        t["submap fine thinned", 8, g] = {**fine, **thin, **per(*BUILD, "k_submap_icp_wide")}
        t["submap coarse", 0, g] = {**best, **per("k_submap_pn_target"), "k_submap_coarse_icp": (g, 4)}
        t["submap coarse", 8, g] = {**best, **per("k_submap_pn_move", *BUILD), "k_submap_coarse_icp_wide": (g, 4)}
        t["submap coarse thinned", 0, g] = {**best, **pn_thin, **per("k_submap_pn_grid"), "k_submap_coarse_icp": (g, 4)}
        t["submap coarse thinned", 8, g] = {**best, **pn_thin, **per(*BUILD), "k_submap_coarse_icp_wide": (g, 4)}
        t["submap top", 0, g] = {**best, **top, **per("k_submap_pn_grid"), "k_submap_coarse_icp": (g, 4)}
        t["submap top", 8, g] = {**best, **top, **per(*BUILD), "k_submap_coarse_icp_wide": (g, 4)}
    return t


EXPECTED = _expected()


@pytest.mark.parametrize("family,D,groups", CASES, ids=[f"{f}, cap {D}, {g} group{'s' * (g > 1)}" for f, D, g in CASES])
def test_a_call_launches_what_it_launched_before_the_fold(contexts, family, D, groups):
    got = launches_of(contexts[groups], family, D)
    print(f"{family}, cap {D}, {groups} groups: {got}")
    assert got == EXPECTED[(family, D, groups)]


def test_the_table_tells_the_paths_apart():
    """the recorded table itself: a cap launches the build's six steps once per group and the wide ICP kernels, no cap none of
    them; two groups launch a map's kernels twice"""
    for (family, D, groups), t in EXPECTED.items():
        wide = [k for k in t if k.endswith("_wide")]
        if D == 0:
            assert not wide and not any(k in t for k in BUILD), (family, groups)
        else:
            assert len(wide) == 1 and all(t[k] == (groups, 2) for k in BUILD), (family, groups, t)
    assert sorted(EXPECTED) == sorted(CASES)


# ---- the hooks' contracts --------------------------------------------------------------------------------------------------------
def test_the_hooks_keep_their_contracts(contexts):
    ctx = contexts[1]
    n = len(MATCHES)
    ctx.set_pair_search_grid(8, 8)
    ctx.set_submap_search_grid(8, 8)
    pair_coarse(ctx)
    coarse_rows = ctx.debug_pair_grid(1, 0, n)
    assert (coarse_rows[:, :2] >= 1).all() and (coarse_rows[:, :2] <= 8).all() and coarse_rows[:, 2].tolist() == [SIZES[0], SIZES[1]]
    pair_fine(ctx)
    rows = ctx.debug_pair_grid(0, 0, n)
    assert (rows[:, :2] >= 1).all() and (rows[:, :2] <= 8).all() and rows[:, 2].tolist() == [SIZES[0], SIZES[1]], rows
    with pytest.raises(bev_amd.BevError, match=INVALID_ARG):
        ctx.debug_pair_grid(0, 0, n + 1)                                      # one past the call's matches
    with pytest.raises(bev_amd.BevError, match=INVALID_ARG):
        ctx.debug_pair_grid(0, n, 1)
    _submap_fine(ctx, 0.0)
    with pytest.raises(bev_amd.BevError, match=INVALID_ARG):
        ctx.debug_pair_grid(0, 0, 1)                                          # another call has used the fine stage's workspace
    rows = ctx.debug_submap_grid(0, 0, 2)
    assert (rows[:, :2] >= 1).all() and (rows[:, :2] <= 8).all() and rows[:, 2].tolist() == [SIZES[0], SIZES[1] + SIZES[2]], rows
    with pytest.raises(bev_amd.BevError, match=INVALID_ARG):
        ctx.debug_submap_grid(0, 0, 3)                                        # one past the last group's maps
    with pytest.raises(bev_amd.BevError, match=INVALID_ARG):
        ctx.debug_submap_grid(0, 2, 1)
    # neither fine call touched the coarse stage's records
    assert np.array_equal(ctx.debug_pair_grid(1, 0, n), coarse_rows)
    _submap_coarse(ctx, 0.0)
    sub_rows = ctx.debug_submap_grid(1, 0, 2)
    assert sub_rows[:, 2].tolist() == [SIZES[0], SIZES[1] + SIZES[2]] and (sub_rows[:, :2] <= 8).all()
    with pytest.raises(bev_amd.BevError, match=INVALID_ARG):
        ctx.debug_pair_grid(1, 0, 1)                                          # ... which a coarse scan-to-map call does
    pair_fine(ctx)
    _submap_fine(ctx, 0.5)
    assert np.array_equal(ctx.debug_submap_grid(1, 0, 2), sub_rows)
    # two launch groups: the hook reads the last one, which has one map
    split = contexts[2]
    split.set_submap_search_grid(8, 8)
    _submap_fine(split, 0.0)
    assert split.debug_submap_grid(0, 0, 1)[0, 2] == SIZES[1] + SIZES[2]
    with pytest.raises(bev_amd.BevError, match=INVALID_ARG):
        split.debug_submap_grid(0, 0, 2)
