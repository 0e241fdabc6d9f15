"""GPU: scan-to-map registration (bev_submap_registration_device_resident, bev_submap_registration_batch).
Every result is compared byte for byte, as a whole bev_icp_result_t, with the checker composition of submap_reg_cases.py
(the fine stage's sequential voxel grid per frame, the oracle's transform per entry, concatenation in entry order, the fine
stage's sequential ICP):

  a. more than 1024 matches on small frames — maps of one identity entry (which also equal the pair call
     bev_fine_registration_device_resident), maps of several posed entries, a map of five 4096-record frames, a map without
     entries — under the whole tool's settings with yaw guesses and the top-part tool's with an uploaded coarse table; the
     same call under a forced group cap (several launch groups, one map alone above the cap);
  b. targets larger than any frame (more than 16384 points: the grid's dimension saturates), of 255, 257 and 1 point;
  c. entry bookkeeping: empty voxel clouds first and in the middle, non-finite points that hold indices, a frame twice in a
     map, a frame in many maps, frames that are only query, only entry or unnamed, matches sharing a map;
  d. the mirror tie in both entry orders;
  e. d_ordered input (h_offsets NULL) of marked HDL_64E frames at half-window 1;
  f. the batch form; calls of different sizes without a synchronisation; a call behind default-stream work;
  g. every refused argument, d_results untouched.
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
from bev_amd import MATCH_DTYPE, POINT_DTYPE, synth
from submap_reg_gpu_lib import F32, INVALID, OK, R, THREADS, TOO_LARGE, _check, _ctx, _dev, _fine_call, _offsets, _results, _same

pytestmark = pytest.mark.gpu
GROUP_CAP = 400000  # bytes: a few small maps per launch group


@pytest.fixture(scope="module", autouse=True)
def _checker():
    fl.build()


def _call(ctx, clouds, maps, m, prm, d_clouds=None, coarse=None, best=None, fill=0):
    """one device-resident call on packed clouds, synchronised: (n,) ICP_RESULT_DTYPE"""
    return _fine_call(ctx, clouds, maps, m, prm, None, d_clouds, coarse, best, fill)


def _lattice(n, seed, spacing=0.5):
    """n points with one point per voxel at leaf 0.2 (a lattice of `spacing` >= 0.25 m): the voxel cloud has n points"""
    rng = np.random.default_rng([int(seed), 0x1A7])
    side = int(np.ceil(n ** 0.5)) + 3
    cells = rng.choice(side * side, n, replace=False)
    c = np.zeros(n, POINT_DTYPE)
    c["x"] = ((cells % side) * spacing - side * spacing / 2 + 0.0625).astype(F32)
    c["y"] = ((cells // side) * spacing - side * spacing / 2 + 0.0625).astype(F32)
    c["z"] = (rng.integers(0, 4, n) * 0.5 + 0.0625).astype(F32)
    c["label"] = 1
    return c


# ---- a. more than 1024 matches on small frames -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small():
    """48 frames of at most 512 records (24 scenes and a moved copy of each) and one of 4096; maps 0 .. 47: frame f under the
    identity; 48 .. 71: one to three posed entries; 72: five entries of the 4096-record frame; 73: no entries.  More than
    1024 matches, the first N_ID of them against the identity maps."""
    rng = np.random.default_rng(20261)
    sizes = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512] + rng.integers(100, 513, 12).tolist()
    H = len(sizes)
    base = [rc.scene(n, 3000 + k) for k, n in enumerate(sizes)]
    yaw = rng.uniform(-10, 10, H).astype(F32)
    tr = rng.uniform(-0.5, 0.5, (H, 2)).astype(F32)
    clouds = base + [rc.moved(base[i], yaw[i], tr[i, 0], tr[i, 1]) for i in range(H)] + [rc.scene(4096, 3999)]
    BIG = 2 * H
    maps = sc.Maps()
    for f in range(2 * H):
        maps.add([(f, sc.IDENTITY)])
    for i in range(H):
        entries = [(H + i, sc.IDENTITY), (H + (i + 1) % H, sc.planar(rng.uniform(-3, 3), *rng.uniform(-1, 1, 2))),
                   ((i + 5) % H, sc.planar(rng.uniform(-3, 3), *rng.uniform(-1, 1, 2)))]
        maps.add(entries[: i % 3 + 1])
    big = maps.add([(BIG, sc.planar(2.0 * k, 0.3 * k, -0.2 * k)) for k in range(5)])
    empty = maps.add([])
    rows, truth = [], []
    n_id = 600
    for _ in range(n_id):
        q, f = int(rng.integers(0, 2 * H)), int(rng.integers(0, 2 * H))
        rows.append((q, f, rng.uniform(-12, 12)))
    for i in range(H):  # every multi-entry map by its own base frame: the first entry is its moved copy
        rows.append((i, 2 * H + i, float(yaw[i]) + rng.uniform(-2, 2)))
    for _ in range(1100 - n_id - H):
        rows.append((int(rng.integers(0, 2 * H)), int(rng.integers(2 * H, 3 * H)), rng.uniform(-12, 12)))
    rows += [(9, big, 1.0), (H + 11, big, -2.0), (BIG, big, 0.5), (7, empty, 0.0), (0, empty, 3.0)]
    order = list(range(n_id)) + (n_id + rng.permutation(len(rows) - n_id)).tolist()
    m = sc.matches([rows[k] for k in order])
    assert len(m) > rc.PROBLEMS_PER_LAUNCH
    coarse, best, guesses = rc.synthetic_coarse(m, [None] * len(m))
    whole = sc.expected(clouds, maps, m, fl.params(**fl.WHOLE), threads=THREADS)
    top = sc.expected(clouds, maps, m, fl.params(**fl.FINE), guesses, threads=THREADS)
    return dict(clouds=clouds, maps=maps, m=m, n_id=n_id, coarse=coarse, best=best, whole=whole, top=top, big=big, empty=empty,
                BIG=BIG)


def _small_call(ctx, S, settings, d_clouds=None):
    if settings == "whole":
        return _call(ctx, S["clouds"], S["maps"], S["m"], bev_amd.icp_whole_defaults(), d_clouds)
    return _call(ctx, S["clouds"], S["maps"], S["m"], None, d_clouds, S["coarse"], S["best"])


@pytest.mark.parametrize("settings", ["whole", "top"])
def test_identity_maps_equal_the_pair_call_and_every_map_the_checker(settings):
    import torch

    S = _small()
    m, n_id = S["m"], S["n_id"]
    exp = S[settings]
    ctx = _ctx()
    try:
        d_clouds = _dev(rc.packed(S["clouds"]))
        got = _small_call(ctx, S, settings, d_clouds)
        print(f"{settings}: {len(m)} matches, states {np.bincount(got['state'], minlength=6)}")
        _check(settings, got, exp)
        # the pair call on the matches against one identity entry (the map's index is its frame's)
        d_pair = torch.zeros(n_id * R, dtype=torch.uint8, device=d_clouds.device)
        kw = dict(params=bev_amd.icp_whole_defaults())
        if settings == "top":
            d_coarse, d_best = _dev(S["coarse"]), _dev(S["best"])
            kw = dict(d_coarse=d_coarse.data_ptr(), d_best=d_best.data_ptr())
        torch.cuda.synchronize()
        ctx.fine_registration_device(len(S["clouds"]), d_clouds.data_ptr(), _offsets(S["clouds"]), m[:n_id], d_pair.data_ptr(), **kw)
        ctx.synchronize()
        _check(f"{settings}: pair call", got[:n_id], _results(d_pair))
    finally:
        ctx.close()
    states = np.bincount(exp["state"], minlength=6)
    assert states[bev_amd.ICP_NO_CORRESPONDENCES] > 0 and (states[1:5] > 0).sum() >= 2
    big = exp[m["match_idx"] == S["big"]]
    assert len(big) == 3 and (big["state"] != bev_amd.ICP_NO_CORRESPONDENCES).all()
    empty = exp[m["match_idx"] == S["empty"]]
    assert len(empty) == 2 and (empty["state"] == bev_amd.ICP_NO_CORRESPONDENCES).all()
    assert (empty["fitness"] == np.finfo(np.float64).max).all() and (empty["converged"] == 0).all()


def _expected_groups(S, cap):
    """the plan's greedy rule restated: groups of consecutive used maps within the cap, a map above it alone"""
    maps, used = S["maps"], sorted({int(g) for g in S["m"]["match_idx"]})
    bytes_of = lambda g: 32 * sum(len(S["clouds"][f]) for f, _ in maps.entries(g)) + 4 * (sc.GRID_CELLS + 1) + 32
    groups, cur, alone = 0, 0, 0
    for g in used:
        b = bytes_of(g)
        if cur and cur + b > cap:
            groups, cur = groups + 1, 0
        alone += b > cap
        cur += b
    return groups + (1 if cur else 0), alone


def test_a_forced_group_cap_gives_the_same_results():
    S = _small()
    n_groups, alone = _expected_groups(S, GROUP_CAP)
    assert n_groups >= 4 and alone == 1  # at least three groups and the five-entry map alone above the cap
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
                got = _small_call(ctx, S, "whole")
                launches[cap] = {k["name"]: k["launches"] for k in ctx.profile_get()}
            finally:
                ctx.close()
            _check(f"cap {cap}", got, S["whole"])
    finally:
        if saved is None:
            os.environ.pop("BEV_SUBMAP_REG_GROUP", None)
        else:
            os.environ["BEV_SUBMAP_REG_GROUP"] = saved
    assert launches[None]["k_submap_target"] == 1 and launches[None]["k_submap_icp"] == 2, launches  # 1024 + the rest
    assert launches[str(GROUP_CAP)]["k_submap_target"] == n_groups, launches
    assert launches[str(GROUP_CAP)]["k_submap_icp"] >= n_groups - 1, launches
    assert "k_fine_grid" not in launches[None] and "k_fine_icp" not in launches[None], launches


# ---- b. targets larger than any frame, and tiny ones ------------------------------------------------------------------------
def test_targets_larger_than_any_frame_and_tiny_targets_equal_the_checker():
    big = [rc.scene(4096, 4100 + k) for k in range(3)]
    lat = [_lattice(100, 1), _lattice(155, 2), _lattice(157, 3), _lattice(1, 4), _lattice(300, 5)]
    queries = [rc.moved(big[0][:300], 2.0, 0.2, -0.1), rc.moved(lat[4], 1.0, 0.05, 0.05)]
    clouds = big + lat + queries
    L, Q = len(big), len(big) + len(lat)
    maps = sc.Maps()
    g_big = maps.add([(0, sc.IDENTITY), (1, sc.planar(3, 0.5, 0)), (2, sc.planar(-4, 0, 0.5)), (0, sc.planar(7, -0.7, 0.2)),
                      (1, sc.planar(-9, 0.1, -0.9))])
    g_big2 = maps.add([(2, sc.planar(1, 0, 0)), (2, sc.IDENTITY), (1, sc.IDENTITY), (0, sc.planar(-2, 0.3, 0.3)), (0, sc.IDENTITY)])
    g_255 = maps.add([(L + 0, sc.IDENTITY), (L + 1, sc.shift(0.25, 0, 0))])
    g_257 = maps.add([(L + 0, sc.IDENTITY), (L + 2, sc.shift(0.25, 0, 0))])
    g_one = maps.add([(L + 3, sc.shift(0.1, 0, 0))])
    m = sc.matches([(Q, g_big, 2.5), (Q, g_big2, 1.5), (Q + 1, g_255, 0.0), (Q + 1, g_257, 1.0), (Q + 1, g_one, 0.0),
                    (L + 0, g_255, 0.0), (L + 4, g_257, -1.0), (Q + 1, g_big, 0.0)])
    vox = {f: fl.voxel_irct(clouds[f]) for f in range(len(clouds))}
    n_tgt = {g: len(sc.target(vox, maps.entries(g))) for g in range(len(maps))}
    assert n_tgt[g_big] > 16384 and n_tgt[g_big2] > 16384              # above every frame's count and the grid's 128 x 128 points
    assert (n_tgt[g_255], n_tgt[g_257], n_tgt[g_one]) == (255, 257, 1)
    for name, prm in (("whole", fl.params(**fl.WHOLE)), ("top-part", fl.params(**fl.FINE))):
        exp = sc.expected(clouds, maps, m, prm, threads=THREADS)
        ctx = _ctx()
        try:
            got = _call(ctx, clouds, maps, m, prm)
        finally:
            ctx.close()
        print(f"{name}: states {exp['state'].tolist()} iterations {exp['iterations'].tolist()}")
        _check(name, got, exp)
        assert (exp["state"] != bev_amd.ICP_NO_CORRESPONDENCES).all()   # (every source point near a map of one point matches it)


# ---- c. entry bookkeeping ---------------------------------------------------------------------------------------------------
def test_entry_bookkeeping_equals_the_checker():
    a, b, c = rc.scene(900, 5001), rc.scene(700, 5002), rc.scene(300, 5003)
    all_nan = rc._special("all_nan", 2026)
    zero = rc.scene(0, 5004)
    holes = rc._special("overflow", 2026)          # the voxel grid returns its input: the records keep their places
    holes["x"][5::7] = np.nan
    holes["z"][6::11] = np.inf
    only_query, unnamed = rc.moved(a, 3.0, 0.2, 0.1), rc.scene(400, 5005)
    clouds = [a, b, c, all_nan, zero, holes, only_query, unnamed, rc.moved(holes, -2.0, 0.1, 0.0)]
    A, B, Cc, NAN, ZERO, HOLES, OQ, _, HQ = range(9)
    maps = sc.Maps()
    g_none = maps.add([])
    g_gaps = maps.add([(NAN, sc.IDENTITY), (A, sc.IDENTITY), (ZERO, sc.planar(1, 0, 0)), (NAN, sc.planar(5, 1, 1)), (B, sc.planar(2, 0.1, 0))])
    g_holes = maps.add([(HOLES, sc.planar(1, 0.1, -0.1)), (Cc, sc.IDENTITY), (HOLES, sc.IDENTITY)])
    g_twice = maps.add([(A, sc.IDENTITY), (A, sc.planar(0.5, 0.05, 0.0)), (A, sc.IDENTITY)])
    g_unused = maps.add([(B, sc.IDENTITY), (7, sc.IDENTITY)])   # named by no match: costs nothing
    g_only_nan = maps.add([(NAN, sc.IDENTITY), (ZERO, sc.IDENTITY)])
    g_inf = maps.add([(A, np.array([1e38, 0, 0, 0, 0, 1e38, 0, 0, 0, 0, 1, 0], F32)), (B, sc.IDENTITY)])  # entry 0 overflows to inf
    g_shared = maps.add([(A, sc.planar(1, 0, 0)), (B, sc.IDENTITY), (Cc, sc.planar(-1, 0, 0.1))])
    rows = [(OQ, g_gaps, 3.0), (OQ, g_none, 0.0), (HQ, g_holes, -2.0), (OQ, g_twice, 2.0), (Cc, g_only_nan, 0.0),
            (B, g_inf, 0.5), (OQ, g_shared, 3.0), (B, g_shared, 0.0), (Cc, g_shared, 1.0), (OQ, g_shared, -3.0),
            (A, g_gaps, 0.0), (NAN, g_shared, 0.0), (ZERO, g_twice, 0.0), (HOLES, g_holes, 0.0)]
    m = sc.matches(rows)
    named = set(m["query_idx"].tolist()) | {f for g in set(m["match_idx"].tolist()) for f, _ in maps.entries(g)}
    assert 7 not in named and g_unused not in m["match_idx"] and OQ not in {f for g in range(len(maps)) for f, _ in maps.entries(g)}
    vox = {f: fl.voxel_irct(clouds[f]) for f in (A, B, Cc, NAN, ZERO, HOLES)}
    assert len(vox[NAN]) == 0 and len(vox[ZERO]) == 0 and len(vox[HOLES]) == len(holes)
    t_holes = sc.target(vox, maps.entries(g_holes))
    assert not np.isfinite(t_holes["x"][:len(holes)]).all() and np.isfinite(t_holes["x"][len(holes):len(holes) + len(vox[Cc])]).all()
    assert not np.isfinite(sc.target(vox, maps.entries(g_inf))["x"][: len(vox[A])]).all()
    for name, prm in (("whole", fl.params(**fl.WHOLE)), ("top-part", fl.params(**fl.FINE))):
        exp = sc.expected(clouds, maps, m, prm, threads=THREADS)
        ctx = _ctx()
        try:
            got = _call(ctx, clouds, maps, m, prm)
        finally:
            ctx.close()
        print(f"{name}: states {exp['state'].tolist()}")
        _check(name, got, exp)
        assert exp["state"][1] == exp["state"][4] == bev_amd.ICP_NO_CORRESPONDENCES
        assert exp["state"][0] != bev_amd.ICP_NO_CORRESPONDENCES and exp["state"][2] != bev_amd.ICP_NO_CORRESPONDENCES


# ---- d. the tie ---------------------------------------------------------------------------------------------------------------
def test_the_mirror_tie_follows_the_entry_order():
    clouds, maps, m = sc.mirror_tie()
    for name, prm in (("whole", fl.params(**fl.WHOLE)), ("top-part", fl.params(**fl.FINE))):
        exp = sc.expected(clouds, maps, m, prm, threads=2)
        ctx = _ctx()
        try:
            got = _call(ctx, clouds, maps, m, prm)
        finally:
            ctx.close()
        _check(name, got, exp)
        assert not _same(got[0], got[1]) and got[0]["T"][3] > 0.25 and got[1]["T"][3] < -0.25


# ---- e. d_ordered input -------------------------------------------------------------------------------------------------------
def test_marked_frames_in_the_d_ordered_layout_equal_the_checker():
    import torch

    p = bev_amd.params_for_sensor("HDL_64E")
    F, S = 4, p.slots
    frames = [synth.sweep(p, 900 + i, keep=0.25, n_dup=500) for i in range(F)]
    offs = _offsets(frames)
    dev = torch.device("cuda:0")
    rel = lambda i, j: sc.IDENTITY if i == j else sc.planar(float(j - i), 0.5 * (j - i), 0.1 * (j - i))
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
        ctx.submap_registration_device(F, d_ord.data_ptr(), None, *maps.arrays(), m, d_res.data_ptr(),
                                       params=bev_amd.icp_whole_defaults())
        ctx.synchronize()
        ordered = list(d_ord.cpu().numpy().view(POINT_DTYPE).reshape(F, S))
        got = _results(d_res)
    finally:
        ctx.close()
    exp = sc.expected(ordered, maps, m, fl.params(**fl.WHOLE), threads=THREADS)
    _check("d_ordered", got, exp)
    assert (exp["state"] != bev_amd.ICP_NO_CORRESPONDENCES).all()


# ---- f. the batch form, reuse and ordering --------------------------------------------------------------------------------------
def _medium():
    a, b = rc.scene(1500, 6001), rc.scene(1100, 6002)
    clouds = [a, b, rc.moved(a, 4.0, 0.3, 0.1), rc.moved(b, -3.0, -0.2, 0.2), rc.scene(65, 6003)]
    maps = sc.Maps()
    maps.add([(0, sc.IDENTITY), (1, sc.planar(1, 0.2, 0))])
    maps.add([(1, sc.IDENTITY), (0, sc.planar(-1, -0.2, 0)), (4, sc.IDENTITY)])
    m = sc.matches([(2, 0, 4.0), (3, 1, -3.0), (4, 0, 0.0)])
    return clouds, maps, m


def test_the_batch_form_equals_the_device_form():
    S = _small()
    clouds, maps, m = _medium()
    ctx = _ctx()
    try:
        for name, (cl, mp, mm, prm, exp) in {
            "medium": (clouds, maps, m, None, sc.expected(clouds, maps, m, fl.params(**fl.FINE), threads=THREADS)),
            "small": (S["clouds"], S["maps"], S["m"], bev_amd.icp_whole_defaults(), S["whole"]),
        }.items():
            dev = _call(ctx, cl, mp, mm, prm)
            host = ctx.submap_registration_batch(cl, *mp.arrays(), mm, params=prm)
            _check(f"{name}: device form", dev, exp)
            _check(f"{name}: batch form", host, dev)
        assert len(ctx.submap_registration_batch(clouds, *maps.arrays(), m[:0])) == 0
    finally:
        ctx.close()


def test_calls_of_different_sizes_without_a_sync_equal_the_checker():
    import torch

    S = _small()
    clouds, maps, m = _medium()
    exp_medium = sc.expected(clouds, maps, m, fl.params(**fl.FINE), threads=THREADS)
    ctx = _ctx()
    try:
        dev = torch.device("cuda:0")
        d_small, d_medium = _dev(rc.packed(S["clouds"])), _dev(rc.packed(clouds))
        d_r = [torch.zeros(len(mm) * R, dtype=torch.uint8, device=dev) for mm in (m, S["m"], m, S["m"])]
        d_pair = torch.zeros(S["n_id"] * R, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        medium = lambda d: ctx.submap_registration_device(len(clouds), d_medium.data_ptr(), _offsets(clouds), *maps.arrays(), m, d.data_ptr())
        small = lambda d: ctx.submap_registration_device(len(S["clouds"]), d_small.data_ptr(), _offsets(S["clouds"]), *S["maps"].arrays(),
                                                         S["m"], d.data_ptr(), params=bev_amd.icp_whole_defaults())
        medium(d_r[0])   # a small call first: the next one grows the workspace and the table of a context that is in use
        small(d_r[1])
        medium(d_r[2])
        ctx.fine_registration_device(len(S["clouds"]), d_small.data_ptr(), _offsets(S["clouds"]), S["m"][: S["n_id"]], d_pair.data_ptr(),
                                     params=bev_amd.icp_whole_defaults())   # the pair call shares the buffer
        small(d_r[3])
        ctx.synchronize()
        _check("0: medium", _results(d_r[0]), exp_medium)
        _check("1: small", _results(d_r[1]), S["whole"])
        _check("2: medium again", _results(d_r[2]), exp_medium)
        _check("3: the pair call between", _results(d_pair), S["whole"][: S["n_id"]])
        _check("4: small again", _results(d_r[3]), S["whole"])
    finally:
        ctx.close()


def test_the_call_waits_for_work_queued_on_the_default_stream():
    import torch

    S = _small()
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
        ctx.submap_registration_device(len(S["clouds"]), d_clouds.data_ptr(), _offsets(S["clouds"]), *S["maps"].arrays(), S["m"],
                                       d_res.data_ptr(), d_coarse.data_ptr(), d_best.data_ptr())
        ctx.synchronize()
        _check("behind an upload and a fill", _results(d_res), S["top"])
    finally:
        ctx.close()


# ---- g. refused arguments -------------------------------------------------------------------------------------------------------
def test_every_refused_argument_leaves_the_results_untouched():
    import torch

    lib = bev_amd.load_lib()
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    big = rc.scene(65536, 7001)                     # really allocated: 64 entries of it are a map of exactly 2^22 records
    small = rc.scene(200, 7002)
    clouds = [big, small]
    offs = _offsets(clouds)
    n_at = sc.REG_MAX_TARGET // len(big)
    assert n_at * len(big) == sc.REG_MAX_TARGET
    maps = sc.Maps()
    maps.add([(0, sc.planar(0.5 * k, 0.01 * k, 0.0)) for k in range(n_at)])
    maps.add([(1, sc.IDENTITY)])
    moffs, eframe, epose = maps.arrays()
    m = sc.matches([(1, 0, 0.0), (1, 1, 1.0)])
    prm = bev_amd.icp_whole_defaults()
    bad_prm = bev_amd.icp_params(max_iterations=0)
    ctx = _ctx()
    try:
        d_clouds = _dev(rc.packed(clouds))
        d_res = torch.full((len(m) * R,), 0xA5, dtype=torch.uint8, device=d_clouds.device)
        d_tab = torch.zeros(4 * R, dtype=torch.uint8, device=d_clouds.device)
        torch.cuda.synchronize()
        h, cl, res, tab = ctx._h, C.c_void_p(d_clouds.data_ptr()), C.c_void_p(d_res.data_ptr()), C.c_void_p(d_tab.data_ptr())

        def call(n_frames=2, clouds_=cl, offs_=offs, leaf=0.2, n_maps=2, moffs_=moffs, eframe_=eframe, epose_=epose, n_matches=2,
                 m_=m, coarse=None, best=None, prm_=prm, res_=res):
            return lib.bev_submap_registration_device_resident(
                h, n_frames, clouds_, u64(offs_) if offs_ is not None else None, leaf, n_maps,
                u64(moffs_) if moffs_ is not None else None, eframe_.ctypes.data if eframe_ is not None else None,
                epose_.ctypes.data if epose_ is not None else None, n_matches, m_.ctypes.data if m_ is not None else None,
                coarse, best, C.byref(prm_) if prm_ is not None else None, res_)

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
            "n_matches < 0": (call(n_matches=-1), INVALID), "leaf 0": (call(leaf=0.0), INVALID), "leaf nan": (call(leaf=float("nan")), INVALID),
            "params": (call(prm_=bad_prm), INVALID), "coarse without best": (call(coarse=tab), INVALID),
            "best without coarse": (call(best=tab), INVALID), "NULL clouds": (call(clouds_=None), INVALID),
            "NULL matches": (call(m_=None), INVALID), "NULL results": (call(res_=None), INVALID),
            "NULL map offsets": (call(moffs_=None), INVALID), "NULL entry frames": (call(eframe_=None), INVALID),
            "NULL entry poses": (call(epose_=None), INVALID),
            "decreasing frame offsets": (call(offs_=np.array([0, 70000, 65536], np.uint64)), INVALID),
            "decreasing map offsets": (call(moffs_=np.array([0, 5, 3], np.uint64)), INVALID),
            "entry frame 2": (call(eframe_=other(eframe, 3, 2)), INVALID), "entry frame -1": (call(eframe_=other(eframe, n_at, -1)), INVALID),
            "query 2": (call(m_=match(0, "query_idx", 2)), INVALID), "query -1": (call(m_=match(1, "query_idx", -1)), INVALID),
            "map 2": (call(m_=match(1, "match_idx", 2)), INVALID), "map -1": (call(m_=match(0, "match_idx", -1)), INVALID),
            "a frame as match_idx of fewer maps": (call(n_maps=1, m_=m), INVALID),
            "too many entries (arrays not read)": (call(moffs_=too_many), TOO_LARGE),
            "a map one frame above the target bound": (call(moffs_=one_more.arrays()[0], eframe_=one_more.arrays()[1],
                                                            epose_=one_more.arrays()[2]), TOO_LARGE),
        }
        ctx.synchronize()
        wrong = {k: v for k, v in refused.items() if v[0] != v[1]}
        assert not wrong, wrong
        assert (d_res.cpu().numpy() == 0xA5).all(), "a refused call wrote d_results"
        assert call(n_matches=0, m_=None, res_=None, clouds_=None) == OK
        assert call(n_frames=0, n_maps=0, n_matches=0, clouds_=None, offs_=None, moffs_=None, eframe_=None, epose_=None, m_=None, res_=None) == OK
        ctx.synchronize()
        assert (d_res.cpu().numpy() == 0xA5).all()
        # the map of exactly BEV_SUBMAP_REG_MAX_TARGET records is accepted (a leaf of 50 m keeps its voxel clouds tiny)
        assert call(leaf=50.0) == OK
        ctx.synchronize()
        exp = sc.expected(clouds, maps, m, fl.params(**fl.WHOLE), leaf=50.0, threads=2)
        _check("at the bound", _results(d_res), exp)
    finally:
        ctx.close()
