"""GPU: scan-to-map coarse ICP (bev_submap_coarse_registration_device_resident).  Every result is compared byte for
byte, as whole bev_icp_result_t records and the choice between the guesses, with the checker composition of
submap_coarse_cases.py (the move of every entry's PointNormal rows in numpy float32, concatenation in entry order, the coarse
stage's sequential ICP per guess, its choice):

  a. the seeded list: a thousand matches on ragged frames of 0 .. 512 rows (counts above the stride among them) against 121
     maps of 0 .. 6 entries under planar and full 3-D poses; the matches against one identity entry also equal the pair call
     bev_coarse_registration_device_resident; the same call under a forced group cap (many launch groups, maps alone above the
     cap);
  b. sources of 63, 64, 65 and 2049 rows, targets of 1, 255 and 257 rows and one above 4096 rows (the grid's dimension
     saturates), a map of 257 entries of tiny frames (the scan's second round);
  c. entry bookkeeping: empty frames first and in the middle, a frame twice in a map and in many maps, frames that are only
     query, only entry or unnamed, a map no match names, matches sharing a map, counts above the stride;
  d. values: NaN normals inside a map, non-finite positions, a matrix that overflows to infinity, a matrix that is no rotation;
  e. the mirror tie in both entry orders;
  f. both stages chained without a synchronisation: front end, this call, bev_submap_voxel_registration_device_resident;
  g. calls of different sizes with the pair call between them; a call behind default-stream work;
  h. every refused argument, d_results and d_best untouched; the capacity bound at the limit and one entry above.
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
import submap_reg_cases as sc
from bev_amd import ICP_RESULT_DTYPE
from submap_reg_gpu_lib import F32, INVALID, OK, R, THREADS, TOO_LARGE, _ctx, _dev, _same

pytestmark = pytest.mark.gpu
GROUP_CAP = 150000  # bytes: a few small maps per launch group


@pytest.fixture(scope="module", autouse=True)
def _checkers():
    icp_lib.build()
    fl.build()
    rf.build()


def _check(name, got, exp):
    """got, exp: ((n, 2) results, (n,) best)"""
    (gr, gb), (er, eb) = got, exp
    gr, er = np.asarray(gr).reshape(-1), np.asarray(er).reshape(-1)
    assert len(gr) == len(er), f"{name}: {len(gr)} records, expected {len(er)}"
    bad = [k for k in range(len(er)) if not _same(gr[k], er[k])]
    assert not bad, f"{name}: {len(bad)} of {len(er)} results differ, first match {bad[0] // 2} guess {bad[0] % 2}: {gr[bad[0]]} != {er[bad[0]]}"
    assert np.array_equal(np.asarray(gb), np.asarray(eb)), f"{name}: best differs at {np.flatnonzero(np.asarray(gb) != np.asarray(eb))[:5]}"


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


def _call(ctx, frames, stride, maps, m, prm=None, d=None):
    """one call on strided frames, synchronised: ((n, 2) ICP_RESULT_DTYPE, (n,) int32)"""
    import torch

    d_pn, d_cnt = d if d is not None else _upload(frames, stride)
    d_res, d_best = _outputs(len(m))
    torch.cuda.synchronize()
    ctx.submap_coarse_registration_device(len(frames), d_pn.data_ptr(), stride, d_cnt.data_ptr(), *maps.arrays(), m, d_res.data_ptr(),
                                          d_best.data_ptr(), prm)
    ctx.synchronize()
    return _read(d_res, d_best, len(m))


def _run_and_check(name, frames, stride, maps, m, prm=None):
    exp = cc.expected(frames, maps, m, prm, stride, threads=THREADS)
    ctx = _ctx()
    try:
        got = _call(ctx, frames, stride, maps, m, prm)
    finally:
        ctx.close()
    print(f"{name}: states {exp[0]['state'].tolist()} iterations {exp[0]['iterations'].tolist()} best {exp[1].tolist()}")
    _check(name, got, exp)
    return exp


# ---- a. the seeded list ---------------------------------------------------------------------------------------------------------
def test_the_seeded_list_equals_the_checker_and_identity_maps_the_pair_call():
    import torch

    S = cc.seeded_list()
    m, n_id, stride, frames = S["m"], S["n_id"], S["stride"], S["frames"]
    exp = cc.seeded_expected(THREADS)
    share = cc.condition_share(exp[0])
    print(f"{len(m)} matches: {share:.3f} of them keep correspondences for two iterations or more under both guesses")
    assert share >= 0.9                                     # the condition on the inputs, on the checker's results alone
    assert (_counts(frames) > stride).any()
    ctx = _ctx()
    try:
        d = _upload(frames, stride)
        got = _call(ctx, frames, stride, S["maps"], m, d=d)
        print(f"states {np.bincount(got[0]['state'].ravel(), minlength=6)} best {np.bincount(got[1], minlength=2)}")
        _check("the seeded list", got, exp)
        # the pair call on the matches against one identity entry (the map's index is its frame's)
        d_res, d_best = _outputs(n_id)
        torch.cuda.synchronize()
        ctx.coarse_registration_device(len(frames), d[0].data_ptr(), stride, d[1].data_ptr(), m[:n_id], d_res.data_ptr(), d_best.data_ptr())
        ctx.synchronize()
        _check("the pair call", (got[0][:n_id], got[1][:n_id]), _read(d_res, d_best, n_id))
    finally:
        ctx.close()
    empty = exp[0][m["match_idx"] == S["empty"]]
    assert len(empty) == 2 and (empty["state"] == bev_amd.ICP_NO_CORRESPONDENCES).all()
    assert (empty["fitness"] == np.finfo(np.float64).max).all() and (empty["converged"] == 0).all()


def test_a_forced_group_cap_gives_the_same_results():
    S = cc.seeded_list()
    n_groups, alone = cc.group_count(S["maps"], S["m"], S["stride"], GROUP_CAP)
    assert n_groups >= 20 and alone >= 1                    # many groups, and six-entry maps alone above the cap
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
                got = _call(ctx, S["frames"], S["stride"], S["maps"], S["m"])
                launches[cap] = {k["name"]: k["launches"] for k in ctx.profile_get()}
            finally:
                ctx.close()
            _check(f"cap {cap}", got, cc.seeded_expected(THREADS))
    finally:
        if saved is None:
            os.environ.pop("BEV_SUBMAP_REG_GROUP", None)
        else:
            os.environ["BEV_SUBMAP_REG_GROUP"] = saved
    assert launches[None]["k_submap_pn_target"] == 1 and launches[None]["k_submap_coarse_icp"] == 2, launches  # 1024 + the rest
    assert launches[str(GROUP_CAP)]["k_submap_pn_target"] == n_groups, launches
    assert launches[str(GROUP_CAP)]["k_submap_coarse_icp"] >= n_groups - 1, launches
    assert launches[None]["k_icp_best"] == 1 and "k_icp" not in launches[None] and "k_icp_grid" not in launches[None], launches


# ---- b. sizes ---------------------------------------------------------------------------------------------------------------------
def test_source_and_target_sizes_equal_the_checker():
    big = [cc.frame(2049, 9100 + k) for k in range(3)]
    small = [cc.frame(n, 9200 + n) for n in (1, 100, 155, 157)]
    ONE, C100, C155, C157 = 3, 4, 5, 6
    near = lambda f, k: cc.move(f, sc.planar(1.0 + 0.3 * k, 0.2, -0.1 * k))
    src = [near(big[0][:63], 0), near(big[0][:64], 1), near(big[1][:65], 2), near(big[0], 3), near(small[1], 4)]
    frames = big + small + src
    Q = len(big) + len(small)
    maps = sc.Maps()
    g_big = maps.add([(0, sc.IDENTITY), (1, cc.pose3d(1, -1, 3, 0.5, 0, 0.1)), (2, sc.planar(-4, 0, 0.5))])
    g_255 = maps.add([(C100, sc.IDENTITY), (C155, sc.shift(0.25, 0, 0))])
    g_257 = maps.add([(C100, sc.IDENTITY), (C157, cc.pose3d(0.5, 0.5, 1, 0.25, 0, 0))])
    g_one = maps.add([(ONE, sc.shift(0.1, 0, 0))])
    m = sc.matches([(Q + 0, g_big, 1.0), (Q + 1, g_big, 1.3), (Q + 2, g_big, 1.6), (Q + 3, g_big, 1.9), (Q + 4, g_255, 2.0),
                    (Q + 4, g_257, 2.2), (Q + 4, g_one, 0.0), (Q + 3, g_257, 0.0), (0, g_255, 0.0)])
    n_tgt = {g: len(cc.target(frames, maps.entries(g))) for g in range(len(maps))}
    assert n_tgt[g_big] > 4096 and (n_tgt[g_255], n_tgt[g_257], n_tgt[g_one]) == (255, 257, 1)
    assert [len(frames[Q + k]) for k in range(4)] == [63, 64, 65, 2049]
    exp = _run_and_check("sizes", frames, 2049, maps, m)
    assert (exp[0]["state"][:6] != bev_amd.ICP_NO_CORRESPONDENCES).all()


def test_a_map_of_257_entries_of_tiny_frames_equals_the_checker():
    rng = np.random.default_rng(9300)
    body = cc.frame(600, 9301)
    tiny = [np.ascontiguousarray(body[k: k + n]) for k, n in zip(range(0, 600, 2), rng.integers(0, 4, 300).tolist())]
    frames = tiny + [cc.move(body[:200], sc.planar(1.0, 0.1, 0.1))]
    maps = sc.Maps()
    g = maps.add([(k, sc.shift(0.01 * (k % 7), 0, 0)) for k in range(257)])        # the scan's second round: entry 256
    g2 = maps.add([(k, sc.IDENTITY) for k in range(299, 40, -1)])
    m = sc.matches([(300, g, 1.0), (300, g2, 1.0), (5, g, 0.0)])
    assert len(maps.entries(g)) == 257 and len(cc.target(frames, maps.entries(g), 4)) > 256 and len(tiny[256]) > 0
    exp = _run_and_check("257 entries", frames, 4, maps, m)
    assert (exp[0]["state"][:2] != bev_amd.ICP_NO_CORRESPONDENCES).all()


# ---- c. entry bookkeeping -----------------------------------------------------------------------------------------------------------
def test_entry_bookkeeping_equals_the_checker():
    a, b, c = cc.frame(500, 9401), cc.frame(400, 9402), cc.frame(300, 9403)
    zero = np.zeros((0, 12), F32)
    only_query, only_entry, unnamed = cc.move(a, sc.planar(3.0, 0.2, 0.1)), cc.frame(350, 9404), cc.frame(100, 9405)
    frames = [a, b, c, zero, only_query, only_entry, unnamed, zero.copy()]
    A, B, Cc, ZERO, OQ, OE, UN, ZERO2 = range(8)
    stride = 450                                             # a's count stays above it
    maps = sc.Maps()
    g_none = maps.add([])
    g_gaps = maps.add([(ZERO, sc.IDENTITY), (A, sc.IDENTITY), (ZERO2, sc.planar(1, 0, 0)), (ZERO, cc.pose3d(1, 1, 5, 1, 1, 0)), (B, sc.planar(2, 0.1, 0))])
    g_twice = maps.add([(A, sc.IDENTITY), (A, cc.pose3d(0.3, -0.2, 0.5, 0.05, 0.0, 0.02)), (A, sc.IDENTITY)])
    g_unused = maps.add([(B, sc.IDENTITY), (UN, sc.IDENTITY)])   # named by no match: costs nothing
    g_only_empty = maps.add([(ZERO, sc.IDENTITY), (ZERO2, sc.IDENTITY)])
    g_shared = maps.add([(A, sc.planar(1, 0, 0)), (OE, sc.IDENTITY), (Cc, cc.pose3d(-1, 0.5, -1, 0, 0.1, 0))])
    g_a_again = maps.add([(Cc, sc.IDENTITY), (A, sc.planar(-1, 0.1, 0.1))])
    rows = [(OQ, g_gaps, 3.0), (OQ, g_none, 0.0), (OQ, g_twice, 2.0), (Cc, g_only_empty, 0.0), (OQ, g_shared, 3.0),
            (B, g_shared, 0.0), (Cc, g_shared, 1.0), (OQ, g_shared, -3.0), (A, g_gaps, 0.0), (ZERO, g_twice, 0.0), (OQ, g_a_again, 3.0)]
    m = sc.matches(rows)
    entry_frames = {f for g in set(m["match_idx"].tolist()) for f, _ in maps.entries(g)}
    assert UN not in set(m["query_idx"].tolist()) | entry_frames and g_unused not in m["match_idx"]
    assert OQ not in {f for g in range(len(maps)) for f, _ in maps.entries(g)} and OE not in m["query_idx"]
    assert len(a) > stride
    exp = _run_and_check("bookkeeping", frames, stride, maps, m)
    st = exp[0]["state"]
    assert (st[1] == bev_amd.ICP_NO_CORRESPONDENCES).all() and (st[3] == bev_amd.ICP_NO_CORRESPONDENCES).all()
    assert (st[9] == bev_amd.ICP_NO_CORRESPONDENCES).all()
    assert (st[0] != bev_amd.ICP_NO_CORRESPONDENCES).all() and (st[4] != bev_amd.ICP_NO_CORRESPONDENCES).all()


# ---- d. values --------------------------------------------------------------------------------------------------------------------
def test_non_finite_values_and_matrices_that_are_no_rotations_equal_the_checker():
    a, b = cc.frame(500, 9501), cc.frame(400, 9502)
    nan_normals = a.copy()
    nan_normals[::3, 4:7] = np.nan
    nan_normals[1::9, 5] = np.inf
    bad_points = b.copy()
    bad_points[::7, 0] = np.nan
    bad_points[1::11, 1] = np.inf
    bad_points[2::13, 2] = -np.inf
    bad_points[5::17, 8] = np.nan                            # (a curvature: copied, canonical, never read)
    query = cc.move(a, sc.planar(2.0, 0.2, -0.1))
    query_b = cc.move(b, sc.planar(-2.0, 0.1, 0.1))
    frames = [a, b, nan_normals, bad_points, query, query_b]
    A, B, NN, BP, QA, QB = range(6)
    overflow = np.array([1e38, 0, 0, 0, 0, 1e38, 0, 0, 0, 0, 1, 0], F32)
    scale = np.array([1.3, 0, 0, 0.1, 0, 1.3, 0, 0, 0, 0, 1.3, 0], F32)
    shear = np.array([1, 0.4, 0, 0, 0, 1, 0, 0.2, 0.1, 0, 1, 0], F32)
    nan_mat = np.array([1, 0, 0, np.nan, 0, 1, 0, 0, 0, 0, 1, 0], F32)
    maps = sc.Maps()
    g_nn = maps.add([(NN, sc.IDENTITY), (B, sc.planar(1, 0.1, 0))])
    g_bp = maps.add([(BP, sc.planar(1, 0.1, -0.1)), (A, sc.IDENTITY), (BP, sc.IDENTITY)])
    g_inf = maps.add([(A, overflow), (B, sc.IDENTITY)])
    g_all_inf = maps.add([(A, nan_mat), (B, nan_mat)])       # no searchable point
    g_scale = maps.add([(A, scale)])
    g_shear = maps.add([(A, shear), (B, sc.IDENTITY)])
    m = sc.matches([(QA, g_nn, 2.0), (QB, g_bp, -2.0), (QB, g_inf, -2.0), (QA, g_all_inf, 0.0), (QA, g_scale, 2.0), (QA, g_shear, 2.0),
                    (NN, g_nn, 0.0), (BP, g_bp, 0.0)])
    t_bp = cc.target(frames, maps.entries(g_bp))
    assert not np.isfinite(t_bp[: len(b), :3]).all() and np.isfinite(t_bp[len(b): len(b) + len(a), :3]).all()
    assert np.isinf(cc.target(frames, maps.entries(g_inf))[: len(a), :2]).any()
    assert np.isnan(cc.target(frames, maps.entries(g_nn))[: len(a), 4:7]).any()
    exp = _run_and_check("values", frames, 512, maps, m)
    st = exp[0]["state"]
    assert (st[3] == bev_amd.ICP_NO_CORRESPONDENCES).all() and (st[[0, 1, 2, 5], 0] != bev_amd.ICP_NO_CORRESPONDENCES).all()


# ---- e. the tie -------------------------------------------------------------------------------------------------------------------
def test_the_mirror_tie_follows_the_entry_order():
    frames, maps, m = cc.mirror_tie()
    exp = _run_and_check("mirror tie", frames, 400, maps, m)
    assert not _same(exp[0][0, 0], exp[0][1, 0])


# ---- f. both stages chained -----------------------------------------------------------------------------------------------------------
def test_front_end_coarse_and_fine_stage_chained_without_a_synchronisation():
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
    # the checker: the front end's chain per frame, the coarse composition, the fine composition from the coarse table
    pn = [rf.chain(c) for c in clouds]
    coarse = cc.expected(pn, maps, m, None, stride, threads=THREADS)
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
        ctx.submap_coarse_registration_device(F, d_pn.data_ptr(), stride, d_cnt.data_ptr(), *maps.arrays(), m, d_res.data_ptr(),
                                              d_best.data_ptr())
        ctx.submap_voxel_registration_device(F, d_clouds.data_ptr(), offs, *maps.arrays(), m, d_fine.data_ptr(), 0.0,
                                             d_res.data_ptr(), d_best.data_ptr())
        ctx.synchronize()
        counts = d_cnt.cpu().numpy()
        assert counts.tolist() == [len(p) for p in pn]
        _check("coarse", _read(d_res, d_best, len(m)), coarse)
        got = d_fine.cpu().numpy().view(ICP_RESULT_DTYPE)
        bad = [k for k in range(len(m)) if not _same(got[k], fine[k])]
        assert not bad, f"fine: {bad}: {got[bad[0]]} != {fine[bad[0]]}"
    finally:
        ctx.close()
    print(f"coarse states {coarse[0]['state'].tolist()} best {coarse[1].tolist()}; fine states {fine['state'].tolist()}")
    assert (coarse[0]["state"][:4] != bev_amd.ICP_NO_CORRESPONDENCES).all() and (fine["state"][:4] != bev_amd.ICP_NO_CORRESPONDENCES).all()


# ---- g. ordering --------------------------------------------------------------------------------------------------------------------
def _medium():
    a, b = cc.frame(480, 9701), cc.frame(350, 9702)
    frames = [a, b, cc.move(a, sc.planar(4.0, 0.3, 0.1)), cc.move(b, sc.planar(-3.0, -0.2, 0.2)), cc.frame(65, 9703)]
    maps = sc.Maps()
    maps.add([(0, sc.IDENTITY), (1, cc.pose3d(1, 1, 1, 0.2, 0, 0))])
    maps.add([(1, sc.IDENTITY), (0, sc.planar(-1, -0.2, 0)), (4, sc.IDENTITY)])
    return frames, 480, maps, sc.matches([(2, 0, 4.0), (3, 1, -3.0), (4, 0, 0.0)])


def test_calls_of_different_sizes_with_the_pair_call_between_equal_the_checker():
    import torch

    S = cc.seeded_list()
    exp_list = cc.seeded_expected(THREADS)
    frames, stride, maps, m = _medium()
    exp_medium = cc.expected(frames, maps, m, None, stride, threads=THREADS)
    n_id = S["n_id"]
    ctx = _ctx()
    try:
        d_list, d_medium = _upload(S["frames"], S["stride"]), _upload(frames, stride)
        outs = [_outputs(len(mm)) for mm in (m, S["m"], m, S["m"])]
        pair = _outputs(n_id)
        torch.cuda.synchronize()
        medium = lambda o: ctx.submap_coarse_registration_device(len(frames), d_medium[0].data_ptr(), stride, d_medium[1].data_ptr(),
                                                                 *maps.arrays(), m, o[0].data_ptr(), o[1].data_ptr())
        big = lambda o: ctx.submap_coarse_registration_device(len(S["frames"]), d_list[0].data_ptr(), S["stride"], d_list[1].data_ptr(),
                                                              *S["maps"].arrays(), S["m"], o[0].data_ptr(), o[1].data_ptr())
        medium(outs[0])   # a small call first: the next one grows the workspace and the table of a context that is in use
        big(outs[1])
        medium(outs[2])
        ctx.coarse_registration_device(len(S["frames"]), d_list[0].data_ptr(), S["stride"], d_list[1].data_ptr(), S["m"][:n_id],
                                       pair[0].data_ptr(), pair[1].data_ptr())   # the pair call shares the buffer and the table
        big(outs[3])
        ctx.synchronize()
        _check("0: medium", _read(*outs[0], len(m)), exp_medium)
        _check("1: the list", _read(*outs[1], len(S["m"])), exp_list)
        _check("2: medium again", _read(*outs[2], len(m)), exp_medium)
        _check("3: the pair call between", _read(*pair, n_id), (exp_list[0][:n_id], exp_list[1][:n_id]))
        _check("4: the list again", _read(*outs[3], len(S["m"])), exp_list)
    finally:
        ctx.close()


def test_the_call_waits_for_work_queued_on_the_default_stream():
    import torch

    S = cc.seeded_list()
    host = torch.from_numpy(rc.strided(S["frames"], S["stride"]).reshape(-1).view(np.uint8).copy()).pin_memory()
    h_cnt = torch.from_numpy(_counts(S["frames"]).view(np.uint8).copy()).pin_memory()
    dev = torch.device("cuda:0")
    ctx = _ctx()
    try:
        d_pn, d_cnt = (torch.zeros(h.numel(), dtype=torch.uint8, device=dev) for h in (host, h_cnt))
        d_res, d_best = _outputs(len(S["m"]))
        torch.cuda.synchronize()
        d_pn.copy_(host, non_blocking=True)
        d_cnt.copy_(h_cnt, non_blocking=True)
        d_res.fill_(0xFF)
        d_best.fill_(0xFF)
        ctx.submap_coarse_registration_device(len(S["frames"]), d_pn.data_ptr(), S["stride"], d_cnt.data_ptr(), *S["maps"].arrays(),
                                              S["m"], d_res.data_ptr(), d_best.data_ptr())
        ctx.synchronize()
        _check("behind an upload and a fill", _read(d_res, d_best, len(S["m"])), cc.seeded_expected(THREADS))
    finally:
        ctx.close()


# ---- h. refused arguments -----------------------------------------------------------------------------------------------------------
def test_every_refused_argument_leaves_the_outputs_untouched_and_the_bound_is_exact():
    import torch

    lib = bev_amd.load_lib()
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    stride = 4096
    n_at = cc.COARSE_MAX_TARGET // stride                    # entries of a map of exactly 2^22 rows
    frames = [cc.frame(40, 9801), cc.move(cc.frame(40, 9801), sc.planar(1.0, 0.1, 0.1))]
    maps = sc.Maps()
    maps.add([(0, sc.shift(0.001 * (k % 50), 0.0, 0.0)) for k in range(n_at)])
    maps.add([(1, sc.IDENTITY)])
    moffs, eframe, epose = maps.arrays()
    m = sc.matches([(1, 0, 1.0), (0, 1, -1.0)])
    prm = bev_amd.icp_params()
    bad_prm = bev_amd.icp_params(max_iterations=0)
    bad_d = bev_amd.icp_params(max_correspondence_distance=float("nan"))
    ctx = _ctx()
    try:
        d_pn, d_cnt = _upload(frames, stride)
        d_res, d_best = _outputs(len(m), 0xA5)
        torch.cuda.synchronize()
        h, pn, cnt = ctx._h, C.c_void_p(d_pn.data_ptr()), C.c_void_p(d_cnt.data_ptr())
        res, best = C.c_void_p(d_res.data_ptr()), C.c_void_p(d_best.data_ptr())

        def call(n_frames=2, pn_=pn, stride_=stride, cnt_=cnt, n_maps=2, moffs_=moffs, eframe_=eframe, epose_=epose, n_matches=2, m_=m,
                 prm_=prm, res_=res, best_=best):
            return lib.bev_submap_coarse_registration_device_resident(
                h, n_frames, pn_, stride_, cnt_, n_maps, u64(moffs_) if moffs_ is not None else None,
                eframe_.ctypes.data if eframe_ is not None else None, epose_.ctypes.data if epose_ is not None else None, n_matches,
                m_.ctypes.data if m_ is not None else None, C.byref(prm_) if prm_ is not None else None, res_, best_)

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
        refused = {
            "n_frames < 0": (call(n_frames=-1), INVALID), "n_maps < 0": (call(n_maps=-1), INVALID),
            "n_matches < 0": (call(n_matches=-1), INVALID), "iterations 0": (call(prm_=bad_prm), INVALID),
            "D nan": (call(prm_=bad_d), INVALID), "stride 0": (call(stride_=0), INVALID),
            "NULL frames": (call(pn_=None), INVALID), "NULL counts": (call(cnt_=None), INVALID),
            "NULL matches": (call(m_=None), INVALID), "NULL results": (call(res_=None), INVALID), "NULL best": (call(best_=None), INVALID),
            "NULL map offsets": (call(moffs_=None), INVALID), "NULL entry frames": (call(eframe_=None), INVALID),
            "NULL entry poses": (call(epose_=None), INVALID),
            "decreasing map offsets": (call(moffs_=np.array([0, 5, 3], np.uint64)), INVALID),
            "entry frame 2": (call(eframe_=other(eframe, 3, 2)), INVALID), "entry frame -1": (call(eframe_=other(eframe, n_at, -1)), INVALID),
            "query 2": (call(m_=match(0, "query_idx", 2)), INVALID), "query -1": (call(m_=match(1, "query_idx", -1)), INVALID),
            "map 2": (call(m_=match(1, "match_idx", 2)), INVALID), "map -1": (call(m_=match(0, "match_idx", -1)), INVALID),
            "a frame as match_idx of fewer maps": (call(n_maps=1), INVALID),
            "too many entries (arrays not read)": (call(moffs_=too_many, eframe_=None, epose_=None), TOO_LARGE),
            "a map one entry above the capacity bound": (call(moffs_=one_more.arrays()[0], eframe_=one_more.arrays()[1],
                                                              epose_=one_more.arrays()[2]), TOO_LARGE),
            "the same map at a stride one row longer": (call(stride_=stride + 1), TOO_LARGE),
        }
        ctx.synchronize()
        wrong = {k: v for k, v in refused.items() if v[0] != v[1]}
        assert not wrong, wrong
        assert (d_res.cpu().numpy() == 0xA5).all() and (d_best.cpu().numpy() == 0xA5).all(), "a refused call wrote its outputs"
        assert call(n_matches=0, m_=None, res_=None, best_=None, pn_=None, cnt_=None, stride_=0) == OK
        assert call(n_frames=0, n_maps=0, n_matches=0, pn_=None, cnt_=None, moffs_=None, eframe_=None, epose_=None, m_=None, res_=None,
                    best_=None) == OK
        ctx.synchronize()
        assert (d_res.cpu().numpy() == 0xA5).all() and (d_best.cpu().numpy() == 0xA5).all()
        # the map of exactly BEV_SUBMAP_COARSE_MAX_TARGET rows of capacity is accepted (its frames hold 40 rows each)
        assert call() == OK
        ctx.synchronize()
        exp = cc.expected(frames, maps, m, None, stride, threads=2)
        _check("at the bound", _read(d_res, d_best, len(m)), exp)
        assert (exp[0]["state"] != bev_amd.ICP_NO_CORRESPONDENCES).all()
    finally:
        ctx.close()
