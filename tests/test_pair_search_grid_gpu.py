"""GPU: the pair calls' search grids sized to the cloud (bev_set_pair_search_grid, bev_debug_get_pair_grid).
The results do not depend on the grid, so every call is compared byte for byte, as whole bev_icp_result_t records, with the
sequential checkers (tests/fineicp, tests/icp) AND with the same call at D = 0; the hook says which grid was really built, and is
checked against a numpy restatement from the rule and the target's points, so a library that ignored the setter would not pass.
The cases are pair_grid_cases.py's.

  1. fine: bev_icp_point_to_point on the 18 000-point target under both tools' settings, and
     bev_fine_registration_device_resident on frames whose voxel clouds cross 128 x 128 cells, from yaw guesses and from a coarse
     table, packed and d_ordered, at D = 0, 8, 128, 130, 256, 1024;
  2. coarse: bev_icp_point_to_plane on the 5 400-row target and bev_coarse_registration_device_resident, D = 0, 4, 64, 70, 256;
  3. slot structure: one target of several matches, a frame that is query and target, a frame against itself, a query-only frame;
  4. / 5. 1 030 fine matches and 520 coarse ones (1 040 problems) on 300 tiny clouds: more problems than a launch, more targets
     than a build group;
  6. degenerate targets and the mirror ties of both stages;
  7. calls back to back without synchronisation around the setter;
  8. the two setters do not read each other's state;
  9. the hook's refusals.
"""
import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import icp_lib as il
import pair_grid_cases as pc
import reg_cases as rc
import submap_grid_cases as gc
from bev_amd import ICP_RESULT_DTYPE
from submap_reg_gpu_lib import R, _check, _ctx, _dev, _offsets, _results, _same
from test_submap_search_grid_gpu import _coarse_call as _submap_coarse_call
from test_submap_search_grid_gpu import _fine as _submap_fine

pytestmark = pytest.mark.gpu
SENSOR = "HDL_32E"
S = bev_amd.params_for_sensor(SENSOR).slots


@pytest.fixture(scope="module", autouse=True)
def _checkers():
    il.build()
    fl.build()


@pytest.fixture(scope="module")
def ctx():
    c = _ctx(SENSOR, max_points=4096)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults(ctx):
    yield
    ctx.set_pair_search_grid(0, 0)
    ctx.set_submap_search_grid(0, 0)


def _fine_device(ctx, clouds, m, ordered=False, coarse=None, best=None, params=None, d_res=None, sync=True):
    """one bev_fine_registration_device_resident call: packed clouds with offsets, or the d_ordered form of frames of S records"""
    import torch

    d_clouds = _dev(np.concatenate(clouds))
    d_res = d_res if d_res is not None else torch.zeros(max(len(m), 1) * R, dtype=torch.uint8, device=d_clouds.device)
    d_coarse, d_best = (_dev(coarse), _dev(best)) if coarse is not None else (None, None)
    torch.cuda.synchronize()
    ctx.fine_registration_device(len(clouds), d_clouds.data_ptr(), None if ordered else _offsets(clouds), m, d_res.data_ptr(),
                                 d_coarse.data_ptr() if coarse is not None else None,
                                 d_best.data_ptr() if best is not None else None, params=params)
    if not sync:
        return d_res, (d_clouds, d_coarse, d_best)
    ctx.synchronize()
    return _results(d_res)[: len(m)]


def _coarse_device(ctx, frames, stride, m):
    """one bev_coarse_registration_device_resident call: ((n, 2) results, (n,) best)"""
    import torch

    d_pn, d_cnt = _dev(rc.strided(frames, stride)), _dev(np.array([len(f) for f in frames], np.uint32))
    d_res = torch.zeros(len(m) * 2 * R, dtype=torch.uint8, device=d_pn.device)
    d_best = torch.full((len(m),), -7, dtype=torch.int32, device=d_pn.device)
    torch.cuda.synchronize()
    ctx.coarse_registration_device(len(frames), d_pn.data_ptr(), stride, d_cnt.data_ptr(), m, d_res.data_ptr(), d_best.data_ptr())
    ctx.synchronize()
    return d_res.cpu().numpy().view(ICP_RESULT_DTYPE).reshape(-1, 2), d_best.cpu().numpy()


def _check2(name, got, exp):
    (gr, gb), (er, eb) = got, exp
    _check(name, np.asarray(gr).reshape(-1), np.asarray(er).reshape(-1))
    assert np.array_equal(np.asarray(gb), np.asarray(eb)), f"{name}: best differs"


def _hook(ctx, name, coarse, m, targets, D):
    """the hook's row of every match against the restatement for the match's target"""
    rows = ctx.debug_pair_grid(coarse, 0, len(m))
    cap = pc.COARSE_CAP if coarse else pc.FINE_CAP
    for k, row in enumerate(rows):
        tgt = targets[int(m["match_idx"][k])]
        print(f"{name} D {D} match {k}: hook {row.tolist()}, restated {pc.grid_expected(tgt, D if D else cap)}")
        assert pc.hook_matches(row, tgt, D, cap), (name, D, k, row.tolist(), pc.grid_expected(tgt, D if D else cap))
    return rows


# ---- 1. fine -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("settings", ["top", "whole"])
def test_point_to_point_does_not_depend_on_the_grid(ctx, settings):
    P = pc.fine_pair()
    prm = fl.params(**(fl.FINE if settings == "top" else fl.WHOLE))
    exp = P["exp_top" if settings == "top" else "exp_whole"]
    assert exp["state"] != bev_amd.ICP_NO_CORRESPONDENCES
    first = None
    for D in pc.FINE_DIMS:
        ctx.set_pair_search_grid(D, 0)
        got = ctx.icp_point_to_point(P["src"], P["tgt"], P["guess"], prm)
        nx, ny, n, cell = (int(v) for v in ctx.debug_pair_grid(0, 0, 1)[0])
        print(f"{settings} D {D}: grid {nx} x {ny}, {n} searchable, largest cell {cell}")
        first = got if D == 0 else first
        assert _same(got, exp), f"{settings} at D {D}: {got} != {exp}"
        assert _same(got, first), f"{settings} at D {D} differs from D 0"
        assert pc.hook_matches((nx, ny, n, cell), P["tgt"], D, pc.FINE_CAP)
        assert n == 18000
        assert max(nx, ny) == min(D, 135) if D else max(nx, ny) <= pc.FINE_CAP, (D, nx, ny)


@pytest.mark.parametrize("ordered", [False, True], ids=["packed", "d_ordered"])
@pytest.mark.parametrize("settings", ["whole", "top"])
def test_fine_registration_does_not_depend_on_the_grid(ctx, settings, ordered):
    F = pc.fine_frames(S)
    clouds, m = F["ordered" if ordered else "clouds"], F["m"]
    exp = F["exp_whole" if settings == "whole" else "exp_top"]
    assert (exp["state"] != bev_amd.ICP_NO_CORRESPONDENCES).sum() >= 3
    first = None
    for D in pc.FINE_DIMS:
        ctx.set_pair_search_grid(D, 0)
        if settings == "whole":
            got = _fine_device(ctx, clouds, m, ordered, params=bev_amd.icp_whole_defaults())
        else:
            got = _fine_device(ctx, clouds, m, ordered, F["coarse"], F["best"])
        first = got if D == 0 else first
        _check(f"{settings} at D {D} against the checker", got, exp)
        _check(f"{settings} at D {D} against D 0", got, first)
        rows = _hook(ctx, settings, 0, m, F["targets"], D)
        if D == 256:
            assert max(rows[0][:2]) == 135 and max(rows[1][:2]) == gc.grid_dim(17000, 256)
        if D == 0:
            assert rows[:, :2].max() <= pc.FINE_CAP


# ---- 2. coarse -----------------------------------------------------------------------------------------------------------------
def test_point_to_plane_does_not_depend_on_the_grid(ctx):
    P = pc.coarse_pair()
    assert P["exp"]["state"] != bev_amd.ICP_NO_CORRESPONDENCES
    first = None
    for D in pc.COARSE_DIMS:
        ctx.set_pair_search_grid(0, D)
        got = ctx.icp_point_to_plane(P["src"], P["tgt"], P["guess"])
        nx, ny, n, cell = (int(v) for v in ctx.debug_pair_grid(1, 0, 1)[0])
        print(f"coarse D {D}: grid {nx} x {ny}, {n} searchable, largest cell {cell}")
        first = got if D == 0 else first
        assert _same(got, P["exp"]), f"coarse at D {D}: {got} != {P['exp']}"
        assert _same(got, first), f"coarse at D {D} differs from D 0"
        assert pc.hook_matches((nx, ny, n, cell), P["tgt"], D, pc.COARSE_CAP)
        assert n == 5400
        assert max(nx, ny) == min(D, 74) if D else max(nx, ny) <= pc.COARSE_CAP, (D, nx, ny)


def test_coarse_registration_does_not_depend_on_the_grid(ctx):
    F = pc.coarse_frames()
    first = None
    for D in pc.COARSE_DIMS:
        ctx.set_pair_search_grid(0, D)
        got = _coarse_device(ctx, F["frames"], F["stride"], F["m"])
        first = got if D == 0 else first
        _check2(f"coarse at D {D} against the checker", got, F["exp"])
        _check2(f"coarse at D {D} against D 0", got, first)
        rows = _hook(ctx, "coarse", 1, F["m"], F["targets"], D)
        if D == 256:
            assert max(rows[0][:2]) == 74 and max(rows[1][:2]) == gc.grid_dim(5000, 256)
        if D == 0:
            assert rows[:, :2].max() <= pc.COARSE_CAP


# ---- 3. slot structure -----------------------------------------------------------------------------------------------------------
def test_slot_structure():
    C = pc.structure_case()
    m = C["m"]
    c = _ctx(SENSOR, max_points=4096)
    try:
        c.profile_enable(True)
        for D in (0, 256):
            c.set_pair_search_grid(D, D)
            c.profile_reset()
            _check(f"fine structure, D {D}", _fine_device(c, C["clouds"], m, params=bev_amd.icp_whole_defaults()), C["exp_fine"])
            rows = _hook(c, "fine structure", 0, m, dict(enumerate(C["clouds"])), D)
            assert rows[0].tolist() == rows[1].tolist() == rows[2].tolist()          # one grid for one target
            prof = {k["name"]: k for k in c.profile_get()}
            if D:   # the targets' grids and no others: the query-only frame has none
                assert prof["k_pairgrid_desc"]["frames"] == C["n_targets"] and prof["k_subgrid_scan"]["frames"] == C["n_targets"]
                assert "k_fine_grid" not in prof and "k_fine_icp" not in prof and prof["k_fine_icp_wide"]["frames"] == len(m)
            else:
                assert prof["k_fine_grid"]["frames"] == C["n_slots"] and "k_fine_icp_wide" not in prof and "k_subgrid_scan" not in prof
            c.profile_reset()
            _check2(f"coarse structure, D {D}", _coarse_device(c, C["frames"], C["stride"], m), C["exp_coarse"])
            rows = _hook(c, "coarse structure", 1, m, dict(enumerate(C["frames"])), D)
            assert rows[0].tolist() == rows[1].tolist() == rows[2].tolist()
            prof = {k["name"]: k for k in c.profile_get()}
            if D:
                assert prof["k_subgrid_scan"]["frames"] == C["n_targets"] and "k_icp_grid" not in prof and "k_icp" not in prof
                assert prof["k_icp_wide"]["frames"] == 2 * len(m)
            else:
                assert prof["k_icp_grid"]["frames"] == C["n_targets"] and "k_icp_wide" not in prof
    finally:
        c.close()


# ---- 4. and 5. past one launch and one build group -------------------------------------------------------------------------------
def test_more_problems_than_a_launch_and_more_targets_than_a_build_group():
    C = pc.many_case()
    c = _ctx(SENSOR, max_points=4096)
    try:
        first_f = _fine_device(c, C["clouds"], C["mf"], params=bev_amd.icp_whole_defaults())
        first_c = _coarse_device(c, C["frames"], C["stride"], C["mc"])
        _check("1030 fine matches, D 0", first_f, C["exp_fine"])
        _check2("520 coarse matches, D 0", first_c, C["exp_coarse"])
        c.profile_enable(True)
        c.set_pair_search_grid(130, 70)
        got = _fine_device(c, C["clouds"], C["mf"], params=bev_amd.icp_whole_defaults())
        prof = {k["name"]: k for k in c.profile_get()}
        _check("1030 fine matches", got, C["exp_fine"])
        _check("1030 fine matches against D 0", got, first_f)
        assert prof["k_fine_icp_wide"]["launches"] == 2 and prof["k_fine_icp_wide"]["frames"] == 1030
        assert prof["k_subgrid_scan"]["launches"] == 2 and prof["k_subgrid_scan"]["frames"] == C["n_targets"]
        _hook(c, "many fine", 0, C["mf"][:8], dict(enumerate(C["clouds"])), 130)
        last = c.debug_pair_grid(0, 1029, 1)[0]
        assert pc.hook_matches(last, C["clouds"][int(C["mf"]["match_idx"][1029])], 130, pc.FINE_CAP)
        c.profile_reset()
        got = _coarse_device(c, C["frames"], C["stride"], C["mc"])
        prof = {k["name"]: k for k in c.profile_get()}
        _check2("520 coarse matches", got, C["exp_coarse"])
        _check2("520 coarse matches against D 0", got, first_c)
        assert prof["k_icp_wide"]["launches"] == 2 and prof["k_icp_wide"]["frames"] == 1040
        assert prof["k_subgrid_scan"]["launches"] == 2 and prof["k_subgrid_scan"]["frames"] == C["n_targets"]
        _hook(c, "many coarse", 1, C["mc"][:8], dict(enumerate(C["frames"])), 70)
    finally:
        c.close()


# ---- 6. degenerate targets and ties ---------------------------------------------------------------------------------------------
def test_degenerate_targets(ctx):
    whole = fl.params(**fl.WHOLE)
    for name, (fs, ft), (cs, ct) in pc.degenerate_case():
        exp_f, exp_c = fl.run(fs, ft, None, whole), il.run(cs, ct)
        for D in (0, 256):
            ctx.set_pair_search_grid(D, D)
            got = ctx.icp_point_to_point(fs, ft, None, whole)
            fine = ctx.debug_pair_grid(0, 0, 1)[0].tolist()
            assert _same(got, exp_f), f"fine {name} at D {D}: {got} != {exp_f}"
            got = ctx.icp_point_to_plane(cs, ct)
            coarse = ctx.debug_pair_grid(1, 0, 1)[0].tolist()
            assert _same(got, exp_c), f"coarse {name} at D {D}: {got} != {exp_c}"
            print(f"{name} D {D}: fine grid {fine}, coarse grid {coarse}")
            for row, tgt, cap in ((fine, ft, pc.FINE_CAP), (coarse, ct, pc.COARSE_CAP)):
                assert pc.hook_matches(row, tgt, D, cap), (name, D, row, pc.grid_expected(tgt, D if D else cap))
                if name in ("empty", "non_finite"):
                    assert row == [1, 1, 0, 0]
                if name == "one_point":
                    assert row == [1, 1, 1, 1]
                if name == "all_y_equal":
                    assert row[1] == 1 and row[2] == 200 and row[0] == gc.grid_dim(200, D if D else cap)
                if name == "clump":
                    assert row[2] == 4001 and row[3] == 4000 and row[1] == 1
        if name in ("empty", "non_finite", "query_outside"):
            assert exp_f["state"] == bev_amd.ICP_NO_CORRESPONDENCES and exp_c["state"] == bev_amd.ICP_NO_CORRESPONDENCES


def test_ties_go_to_the_lowest_index_whatever_the_order_inside_a_cell(ctx):
    (fsrc, ftgts), (csrc, ctgts) = pc.mirror_ties()
    for name, prm in (("whole", fl.params(**fl.WHOLE)), ("top-part", fl.params(**fl.FINE))):
        exp = [fl.run(fsrc, t, None, prm) for t in ftgts]
        assert not _same(exp[0], exp[1])                                           # the order of the target decides
        for D in (0, 256):
            ctx.set_pair_search_grid(D, D)
            for k in (0, 1):
                got = ctx.icp_point_to_point(fsrc, ftgts[k], None, prm)
                assert _same(got, exp[k]), f"fine mirror tie {name}, order {k}, D {D}: {got} != {exp[k]}"
    cexp = [il.run(csrc, t) for t in ctgts]
    assert not _same(cexp[0], cexp[1])
    for D in (0, 256):
        ctx.set_pair_search_grid(D, D)
        for k in (0, 1):
            got = ctx.icp_point_to_plane(csrc, ctgts[k])
            assert _same(got, cexp[k]), f"coarse mirror tie, order {k}, D {D}: {got} != {cexp[k]}"


# ---- 7. ordering ----------------------------------------------------------------------------------------------------------------
def test_the_setter_needs_no_synchronisation(ctx):
    import torch

    F = pc.fine_frames(S)
    d_clouds = _dev(np.concatenate(F["clouds"]))
    res = [torch.zeros(len(F["m"]) * R, dtype=torch.uint8, device=d_clouds.device) for _ in range(3)]
    ctx.set_pair_search_grid(0, 0)
    torch.cuda.synchronize()
    for d, D in zip(res, (0, 256, 0)):          # nothing waits between these
        ctx.set_pair_search_grid(D, 0)
        ctx.fine_registration_device(len(F["clouds"]), d_clouds.data_ptr(), _offsets(F["clouds"]), F["m"], d.data_ptr(),
                                     params=bev_amd.icp_whole_defaults())
    ctx.synchronize()
    for k, d in enumerate(res):
        _check(f"call {k} of three back to back", _results(d), F["exp_whole"])
    assert max(ctx.debug_pair_grid(0, 0, 1)[0][:2]) <= pc.FINE_CAP                       # the last call ran at D = 0
    C = pc.coarse_frames()
    first = _coarse_device(ctx, C["frames"], C["stride"], C["m"])
    ctx.set_pair_search_grid(0, 256)
    _check2("coarse behind the setter", _coarse_device(ctx, C["frames"], C["stride"], C["m"]), first)
    assert max(ctx.debug_pair_grid(1, 0, 1)[0][:2]) == 74


# ---- 8. the setters are independent --------------------------------------------------------------------------------------------
def test_the_two_setters_do_not_read_each_others_state(ctx):
    P, Q = pc.fine_pair(), pc.coarse_pair()
    ctx.set_submap_search_grid(256, 256)
    assert _same(ctx.icp_point_to_point(P["src"], P["tgt"], P["guess"], fl.params(**fl.FINE)), P["exp_top"])
    assert max(ctx.debug_pair_grid(0, 0, 1)[0][:2]) <= pc.FINE_CAP
    assert _same(ctx.icp_point_to_plane(Q["src"], Q["tgt"], Q["guess"]), Q["exp"])
    assert max(ctx.debug_pair_grid(1, 0, 1)[0][:2]) <= pc.COARSE_CAP
    ctx.set_submap_search_grid(0, 0)
    ctx.set_pair_search_grid(256, 256)
    Sf, Sc = gc.fine_case(), gc.coarse_case()
    _submap_fine(ctx, Sf, "whole", 0.0)
    assert max(ctx.debug_submap_grid(0, 0, 1)[0][:2]) <= gc.FINE_CAP
    _submap_coarse_call(ctx, Sc["frames"], Sc["stride"], Sc["maps"], Sc["m"])
    assert max(ctx.debug_submap_grid(1, 0, 1)[0][:2]) <= gc.COARSE_CAP
    ctx.icp_point_to_point(P["src"], P["tgt"], P["guess"], fl.params(**fl.FINE))
    assert max(ctx.debug_pair_grid(0, 0, 1)[0][:2]) == 135


# ---- 9. the hook's refusals ----------------------------------------------------------------------------------------------------
def test_the_hook_refuses_what_it_cannot_answer(ctx):
    fresh = _ctx(SENSOR, max_points=4096)
    try:
        for coarse in (0, 1):
            with pytest.raises(bev_amd.BevError):
                fresh.debug_pair_grid(coarse, 0, 0)                                 # before any such call
    finally:
        fresh.close()
    for fine, coarse in ((-1, 0), (0, -1), (1025, 0), (0, 1025)):
        with pytest.raises(bev_amd.BevError):
            ctx.set_pair_search_grid(fine, coarse)
    C = pc.structure_case()
    ctx.set_pair_search_grid(256, 256)
    _fine_device(ctx, C["clouds"], C["m"], params=bev_amd.icp_whole_defaults())
    _coarse_device(ctx, C["frames"], C["stride"], C["m"])
    n = len(C["m"])
    for coarse in (0, 1):
        assert len(ctx.debug_pair_grid(coarse, 0, n)) == n
        for first, count in ((0, n + 1), (n, 1), (-1, 1), (0, -1)):
            with pytest.raises(bev_amd.BevError):
                ctx.debug_pair_grid(coarse, first, count)                           # a range past the matches
    with pytest.raises(bev_amd.BevError):
        ctx.debug_pair_grid(2, 0, 1)
    # another call lays the stage's workspace out anew: a voxel grid in the fine stage's, a scan-to-map call in the coarse one's
    ctx.voxel_grid_irct(C["clouds"][0], 0.2)
    with pytest.raises(bev_amd.BevError):
        ctx.debug_pair_grid(0, 0, 1)
    Sc = gc.clump_case()
    _submap_coarse_call(ctx, Sc[0], Sc[1], Sc[2], Sc[3])
    with pytest.raises(bev_amd.BevError):
        ctx.debug_pair_grid(1, 0, 1)
