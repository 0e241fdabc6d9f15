"""GPU: the BEV rasters over the parameter space bev_create admits (tests/raster_cases.py): every admitted image size and
band layout, intervals and height resolutions that are divided by (the kPow2 = false instantiations of k_stage, k_walk and
k_ground_resolve), layer counts, ranges and ground offsets the reference does not have, and the other consumers of
RasterParams (the per-cloud rasters, the posed rasters), plus the float BEV at intervals that are not powers of two.
Every comparison is of bytes against the generalised oracle (oracle_multi_bev_ex / oracle_single_bev_ex after the
oracle's ordering and ground marking).  Each case first asserts, on the oracle's side, that its input exercises what
the case is about: points on both sides of every image edge, coordinates that a multiplication by a rounded reciprocal
would bin or layer differently, non-empty layer planes, the route a frame took, the raster's fallback taken."""
import functools

import numpy as np
import pytest
import torch

import bev_amd
import oracle_lib as orc
import raster_cases as rc
from bev_amd import POINT_DTYPE, synth
from packed_cases import _dev, _pack

pytestmark = pytest.mark.gpu
GENERAL, STREAM, REDO, STRUCTURED, COLMAJOR, COLMAJOR_GEN = 0, 1, 2, 3, 4, 5
GUARD, PATTERN = 1 << 12, 0xA5


def _want(p, frames):
    return [orc.process_frame_params(p, f) for f in frames]


def _assert_frames(got, want, what):
    ordered, multi, single, gm = got
    for i, (o_ord, o_gm, o_multi, o_single) in enumerate(want):
        assert ordered[i].tobytes() == o_ord.tobytes(), f"{what}: frame {i}: ordered cloud / labels differ"
        if gm is not None:
            assert np.array_equal(gm[i], o_gm), f"{what}: frame {i}: ground_mat differs"
        assert np.array_equal(multi[i], o_multi), f"{what}: frame {i}: multi BEV differs at {np.argwhere(multi[i] != o_multi)[:4]}"
        assert np.array_equal(single[i], o_single), f"{what}: frame {i}: single BEV differs at {np.argwhere(single[i] != o_single)[:4]}"


def _run_batch(p, frames, want, max_batch=4):
    """process_batch with and without the ground matrix (two kGm instantiations of the walk) in one context"""
    ctx = bev_amd.BevContext(p, device=0, max_batch=max_batch, max_points=max(8, max(len(f) for f in frames)))
    try:
        for want_gm in (True, False):
            _assert_frames(ctx.process_batch(frames, want_ground_mat=want_gm), want, f"want_ground_mat={want_gm}")
        return [int(v) for v in ctx.code_overflow(0, min(len(frames), max(1, max_batch // 2 - 1)))] if max_batch >= 4 else []
    finally:
        ctx.close()


def _edge_conditions(p, want):
    """points fall on both sides of every image edge, and in the first and last bin, on x and on y"""
    s = rc.survivors([w[0] for w in want])
    M = p.mat_size
    for c in ("x", "y"):
        b = rc.bins_div(s[c], p.max_range, p.interval)
        other = rc.bins_div(s["y" if c == "x" else "x"], p.max_range, p.interval)
        inside = (other >= 0) & (other < M)
        assert (b < 0).any() and (b >= M).any(), c
        assert ((b == 0) & inside).any() and ((b == M - 1) & inside).any(), c


def _divide_conditions(p, want):
    """among the points that reach the rasters: at least 8 coordinates that fl(1 / interval) would bin differently, at least
    4 heights that fl(1 / height_res) would layer differently (where the divisor is not a power of two)"""
    s = rc.survivors([w[0] for w in want])
    M = p.mat_size
    bx, by = rc.bins_div(s["x"], p.max_range, p.interval), rc.bins_div(s["y"], p.max_range, p.interval)
    s = s[(bx >= 0) & (bx < M) & (by >= 0) & (by < M)]   # (a point outside the image on either axis tests nothing)
    nb, nl = rc.discriminating(p, s["x"], s["y"], s["z"])
    if not rc.is_pow2(p.interval):
        assert nb >= 8, nb
    if not rc.is_pow2(p.height_res):
        assert nl >= 4, nl
    return nb, nl


def _layer_conditions(p, want):
    """every layer plane holds a cell, the single image holds a clamped 255, and heights reach two layers below the first
    plane and two above the last"""
    multi = np.maximum.reduce([w[2] for w in want])
    single = np.maximum.reduce([w[3] for w in want])
    assert multi.shape[0] == p.n_layers and all(multi[l].any() for l in range(p.n_layers)), [bool(multi[l].any()) for l in range(p.n_layers)]
    assert (single == 255).any()
    s = rc.survivors([w[0] for w in want])
    lay = rc.layers_div(s["z"], p.height_res, p.lidar_to_ground)
    assert (lay <= -2).any() and (lay == -1).any() and (lay == p.n_layers).any() and (lay >= p.n_layers + 2).any()


# ---- (a) every admitted size ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fields", rc.SIZE_CASES, ids=[n for n, _ in rc.SIZE_CASES])
def test_every_admitted_image_size(name, fields):
    """9 frames (one more than a launch group of 8) of the small geometry per call, max_batch 4"""
    p = rc.small_params(**fields)
    frames, _ = rc.small_frames(p)
    assert len(frames) == 9
    want = _want(p, frames)
    _edge_conditions(p, want)
    if not rc.is_pow2(p.interval):
        _divide_conditions(p, want)
    _run_batch(p, frames, want)


STRIP_COLS, CODE_LIST_CAP = 236, 4096   # bev_internal.h kStripCols, kCodeListCap


def _distinct_codes_per_list(p, pts):
    """A lower bound of what the walk appends to each (strip, band) code list of a frame: the number of DISTINCT codes among
    the strip's slots that are not candidates (the walk skips a code only when it has listed the same code before)."""
    import hostcheck_lib as hc
    ordered, gm_a = hc.phase_a_ground_mat(p, pts)
    M, lay = p.mat_size, hc.band_layout(p.mat_size)
    with np.errstate(all="ignore"):
        bx, by = rc.bins_div(ordered["x"], p.max_range, p.interval), rc.bins_div(ordered["y"], p.max_range, p.interval)
        h = np.clip(np.trunc((ordered["z"] + np.float32(p.lidar_to_ground)).astype(np.float64) * 4.0), 0, 255)
        layer = rc.layers_div(ordered["z"], p.height_res, p.lidar_to_ground)
    layer = np.where((layer >= 0) & (layer < p.n_layers), layer, 31)
    ok = (ordered["label"] != 0) & (gm_a.reshape(-1) != 1) & (bx >= 0) & (bx < M) & (by >= 0) & (by < M) & np.isfinite(ordered["z"])
    x = bx[ok].astype(np.int64)
    n0, n1 = lay["z0"] // lay["coarse"], (lay["z1"] - lay["z0"]) // lay["fine"]
    band = np.where(x < lay["z0"], x // lay["coarse"],
                    np.where(x < lay["z1"], n0 + (x - lay["z0"]) // lay["fine"], n0 + n1 + (x - lay["z1"]) // lay["coarse"]))
    strip = (np.arange(p.slots) % p.horizon_scan // STRIP_COLS)[ok]
    code = x | (by[ok].astype(np.int64) << 9) | (h[ok].astype(np.int64) << 18) | (layer[ok].astype(np.int64) << 26)
    keys = np.unique((strip.astype(np.int64) * 64 + band) << 32 | code)
    _, counts = np.unique(keys >> 32, return_counts=True)
    return int(counts.max()) if len(counts) else 0


@pytest.mark.parametrize("name,fields", [c for c in rc.SIZE_CASES if c[0] in ("M16", "M32", "M48", "M16_coarse")],
                         ids=["M16", "M32", "M48", "M16_coarse"])
def test_small_images_take_the_rasters_fallback(name, fields):
    """A (strip, band) code list holds min(kCodeListCap = 4096, N * 236) codes: on the small geometry (N = 16: 3,776) no list
    can overflow, whatever the image size, so the smallest sizes run HDL_64E frames as well (15,104 slots per strip).  The
    walk lists a code once per strip as long as it remembers it, and a band of a small image holds few distinct codes:
    scaled HDL_64E sweeps stay far under the capacity at these sizes too (at most 320 distinct codes in a list, and no
    overflow when run: both printed below).  The frame that does overflow is a pile: every return above the image's first coarse band with
    heights over the whole range of the clamped height, i.e. more than 4,096 distinct codes in one list — counted on the
    oracle's side before the GPU runs.  That band is then rastered from the ordered cloud, without BEV_CODE_CAP."""
    p = rc.with_fields(bev_amd.params_for_sensor("HDL_64E"), **fields)
    coarse = rc.mat_size_layout(p)["coarse"]
    pile = synth.structured(p, 84, 1.0).copy()
    rng = np.random.default_rng(1)
    pile["x"] = (rng.uniform(-0.9, coarse - 1.1, len(pile)) * p.interval - p.max_range).astype(np.float32)   # image rows 0 .. coarse - 1
    pile["y"] = (rng.uniform(-1.1, 1.1, len(pile)) * p.max_range).astype(np.float32)
    pile["z"] = rng.uniform(-3, 63, len(pile)).astype(np.float32)
    frames = [rc.scale_xy(p, synth.sweep(p, 90).copy()), rc.scale_xy(p, synth.structured(p, 91, 0.9).copy()), pile]
    placed = rc.place_boundary(p, frames, [0, 1], rc.boundary_points(p))
    assert placed > 0
    fill = [_distinct_codes_per_list(p, f) for f in frames]
    print(name, "distinct codes in the fullest (strip, band) list per frame:", fill)
    assert fill[2] > CODE_LIST_CAP, fill
    want = _want(p, frames)
    ovf = _run_batch(p, frames, want, max_batch=8)
    print(name, "bands with an overflowed list per frame:", ovf)
    assert len(ovf) == 3 and ovf[2] > 0, ovf


# ---- (b) divide variants ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fields", rc.DIVIDE_CASES, ids=[n for n, _ in rc.DIVIDE_CASES])
def test_intervals_and_resolutions_that_are_divided_by(name, fields):
    p = rc.small_params(**fields)
    assert not (rc.is_pow2(p.interval) and rc.is_pow2(p.height_res))
    frames, _ = rc.small_frames(p)
    want = _want(p, frames)
    print(name, "discriminating (bin coordinates, layer heights) among the surviving points:", _divide_conditions(p, want))
    _edge_conditions(p, want)
    _run_batch(p, frames, want)


# ---- (c) every route under the divide variant ---------------------------------------------------------------------------
def _shuffled(p, fid):
    f = synth.sweep(p, fid, keep=0.9, n_dup=500)
    return f[np.random.default_rng(fid).permutation(len(f))]


ROUTES = [("sweep", "HDL_64E", lambda p, i: synth.sweep(p, 500 + i, n_dup=2000), STREAM),
          ("structured", "HDL_32E", lambda p, i: synth.structured(p, 510 + i, (0.98, 1.0, 0.6)[i]), STRUCTURED),
          ("firing_order", "OS1_64", lambda p, i: synth.firing_order(p, 520 + i), COLMAJOR),
          ("firing_real", "OS1_64", lambda p, i: synth.firing_real(p, 530 + i), COLMAJOR_GEN),
          ("shuffled", "HDL_32E", _shuffled, GENERAL)]


@pytest.mark.parametrize("layout,sensor,make,mode", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route_under_the_divide_variant(layout, sensor, make, mode):
    """interval 0.7 and the sensor's height resolution x 1.2 through bev_process_device_resident, with and without the
    ground matrix: k_walk / k_stage of every source with kPow2 = false; and the identity walk of bev_mark_ground"""
    p = rc.with_fields(bev_amd.params_for_sensor(sensor), interval=0.7, height_res=rc.ROUTE_RES[sensor])
    frames = [make(p, i).copy() for i in range(3)]
    assert rc.place_boundary(p, frames, [0, 1, 2], rc.boundary_points(p)) > 500
    want = _want(p, frames)
    _divide_conditions(p, want)
    S, M, L, n = p.slots, p.mat_size, p.n_layers, len(frames)
    offs, flat = _pack(frames)
    dev = torch.device("cuda:0")
    ctx = bev_amd.BevContext(p, device=0, max_batch=16, max_points=max(len(f) for f in frames))
    try:
        d_in = _dev(flat)
        for with_gm in (True, False):
            outs = [torch.full((n * k + GUARD,), PATTERN, dtype=torch.uint8, device=dev) for k in (S * 32, L * M * M, M * M, S)]
            torch.cuda.synchronize()
            ctx.process_device(n, d_in.data_ptr(), offs, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                               outs[3].data_ptr() if with_gm else None)
            ctx.synchronize()
            info = ctx.frame_info(0, n)
            assert [int(m) for m in info[:, 1]] == [mode] * n, (layout, info)
            host = [o.cpu().numpy() for o in outs]
            for o, k in zip(host, (S * 32, L * M * M, M * M, S)):
                assert (o[n * k:] == PATTERN).all(), "something was written behind an output"
            got = (host[0][:n * S * 32].view(POINT_DTYPE).reshape(n, S), host[1][:n * L * M * M].reshape(n, L, M, M),
                   host[2][:n * M * M].reshape(n, M, M),
                   host[3][:n * S].view(np.int8).reshape(n, p.n_scan, p.horizon_scan) if with_gm else None)
            if not with_gm:
                assert (host[3] == PATTERN).all()
            _assert_frames(got, want, f"{layout} with_gm={with_gm}")
        sp = orc.sensor_from_params(p)
        plain = orc.order_cloud(sp, frames[0])
        cloud, gm = ctx.mark_ground(plain)
        o_cloud, o_gm, _ = orc.mark_ground(sp, plain)
        assert cloud.tobytes() == o_cloud.tobytes() and np.array_equal(gm, o_gm)
    finally:
        ctx.close()


# ---- (d) layers, range and offset -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fields", rc.LAYER_CASES, ids=[n for n, _ in rc.LAYER_CASES])
def test_layer_counts_ranges_and_ground_offsets(name, fields):
    """store_planes' split of the layer masks at 16 (n_layers 1, 16, 17, 30), the offset in the layer and in the clamped
    height, ranges under 75 m (the ground grid's cell edges leave the image: candidate keys escape or clamp)"""
    p = rc.small_params(**fields)
    frames, _ = rc.small_frames(p)
    want = _want(p, frames)
    _layer_conditions(p, want)
    _edge_conditions(p, want)
    _run_batch(p, frames, want)


# ---- (e) the other consumers of RasterParams --------------------------------------------------------------------------
POSES = [(1.5, -2.25, 0.125, 30), (-3, 4, 1, -45.5)]


@pytest.mark.parametrize("name,fields", rc.OTHER_CASES, ids=[n for n, _ in rc.OTHER_CASES])
def test_per_cloud_and_posed_rasters(name, fields):
    """bev_multi_bev / bev_single_bev on an arbitrary cloud (k_cloud_codes + the dense raster) and
    bev_posed_bev_device_resident without a pose and under two poses (k_posed_*), against the oracle's transform_cloud and
    the generalised rasters"""
    p = rc.small_params(**fields)
    sp = orc.sensor_from_params(p)
    b = rc.boundary_points(p)
    b["label"] = -2
    adv = synth.adversarial(p, 12000, 7, nonfinite=True)
    sweep = rc.scale_xy(p, synth.sweep(p, 600, keep=1.0, n_dup=0).copy())
    clouds = [np.concatenate([b, adv]), sweep, adv[:0], np.concatenate([adv[:257], b[::3]])]
    args = (p.interval, p.max_range, p.n_layers, p.lidar_to_ground)

    def want(cloud, m=None):
        moved = cloud if m is None else orc.transform_cloud(cloud, m)
        return orc.multi_bev(sp, moved, *args), orc.single_bev(moved, p.interval, p.max_range, p.lidar_to_ground)

    if not (rc.is_pow2(p.interval) and rc.is_pow2(p.height_res)):
        nb, nl = rc.discriminating(p, b["x"], b["y"], b["z"])
        assert nb >= 8 and nl >= 4, (nb, nl)
    assert want(clouds[0])[0].any()
    M, L = p.mat_size, p.n_layers
    ctx = bev_amd.BevContext(p, device=0, max_batch=4, max_points=max(len(c) for c in clouds))
    try:
        for c in clouds:
            wm, ws = want(c)
            assert np.array_equal(ctx.multi_bev(c), wm) and np.array_equal(ctx.single_bev(c), ws), len(c)
        offs, flat = _pack(clouds)
        d_in = _dev(flat)
        mats = np.stack([orc.yaw_translate_matrix(*[float(v) for v in pose]) for pose in POSES])
        for poses in (None, np.broadcast_to(mats, (len(clouds), 2, 12)).copy()):
            K = 1 if poses is None else 2
            n = len(clouds) * K
            d_multi = torch.full((n * L * M * M + GUARD,), PATTERN, dtype=torch.uint8, device=d_in.device)
            d_single = torch.full((n * M * M + GUARD,), PATTERN, dtype=torch.uint8, device=d_in.device)
            torch.cuda.synchronize()
            ctx.posed_bev_device(len(clouds), d_in.data_ptr(), offs, d_multi.data_ptr(), d_single.data_ptr(), poses=poses)
            ctx.synchronize()
            gm_, gs_ = d_multi.cpu().numpy(), d_single.cpu().numpy()
            assert (gm_[n * L * M * M:] == PATTERN).all() and (gs_[n * M * M:] == PATTERN).all()
            gm_, gs_ = gm_[:n * L * M * M].reshape(n, L, M, M), gs_[:n * M * M].reshape(n, M, M)
            for f, c in enumerate(clouds):
                for k in range(K):
                    wm, ws = want(c, None if poses is None else poses[f, k])
                    assert np.array_equal(gm_[f * K + k], wm) and np.array_equal(gs_[f * K + k], ws), (f, k)
    finally:
        ctx.close()


# ---- (f) the float BEV at intervals that are not powers of two ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _float_sources():
    p = bev_amd.params_for_sensor("HDL_64E")
    sp = orc.sensor_from_params(p)
    marked = orc.mark_ground(sp, orc.order_cloud(sp, synth.sweep(p, 21)))[0]
    adv = synth.adversarial(p, 60000, 3, nonfinite=True)
    assert (marked["label"] == 0).any() and (adv["label"] == 0).any()
    return p, marked, adv


def _float_family(interval, M):
    """the float BEV's bins (saveAsMat: range 100, M = 200 / interval + 1): every edge and its neighbours, and coordinates
    within 64 ulps of an edge that fl(1 / interval) bins differently"""
    q = bev_amd.BevParams()
    q.interval, q.max_range, q.n_layers, q.height_res, q.lidar_to_ground = interval, 100, 1, 1.0, 2.0
    k = np.arange(M + 1, dtype=np.float32)
    edges = (k * np.float32(interval)).astype(np.float32) - np.float32(100)
    w = rc._ulp_window(edges)
    a, b = rc.bins_div(w, 100, interval), rc.bins_mul(w, 100, interval)
    hit = w[(a != b) & (np.minimum(a, b) >= 0) & (np.maximum(a, b) < M)]
    fam = np.concatenate([rc._with_neighbours(edges), hit[np.linspace(0, len(hit) - 1, min(256, len(hit))).astype(int)]])
    rng = np.random.default_rng(int(M))
    pts = np.zeros(len(fam), POINT_DTYPE)
    pts["x"], pts["y"] = fam, rng.permutation(fam)
    pts["z"] = rng.uniform(-1.9, 30, len(fam)).astype(np.float32)
    pts["label"] = -2
    return pts


@pytest.mark.parametrize("interval,M", [(0.8, 251), (0.3, 667), (0.2, 1001), (7.0, 29)])
def test_float_bev_at_intervals_that_are_not_powers_of_two(interval, M):
    p, marked, adv = _float_sources()
    fam = _float_family(interval, M)
    rng = np.random.default_rng(11)
    frames = [adv[:0], adv[:1], fam, marked[5000:5000 + 40000], adv[1000:1000 + int(rng.integers(3000, 40001))],
              np.concatenate([fam[::2], marked[70000:90000]]), adv[:257]]
    assert max(len(f) for f in frames) <= 40000
    bx, by = rc.bins_div(fam["x"], 100, interval), rc.bins_div(fam["y"], 100, interval)
    ins = (bx >= 0) & (bx < M) & (by >= 0) & (by < M)
    nb = int((((rc.bins_mul(fam["x"], 100, interval) != bx) | (rc.bins_mul(fam["y"], 100, interval) != by)) & ins).sum())
    assert nb >= 8, nb
    mats = np.stack([orc.yaw_translate_matrix(*[float(v) for v in pose]) for pose in POSES])
    poses = np.broadcast_to(mats, (len(frames), 2, 12)).copy()

    def want(cloud, skip, m=None):
        return orc.float_bev(cloud if m is None else orc.transform_cloud(cloud, m), interval, skip)

    ctx = bev_amd.BevContext(p, device=0, max_batch=4, max_points=p.slots)
    try:
        assert int(ctx.lib.bev_float_bev_size(interval)) == M == want(frames[0], True).shape[0]
        assert want(fam, True).any()
        for skip in (True, False):
            for f in (fam, frames[3]):
                assert ctx.float_bev(f, interval, skip).tobytes() == want(f, skip).tobytes(), (skip, len(f))
        offs, flat = _pack(frames)
        d_in = _dev(flat)
        for ps in (None, poses):
            K = 1 if ps is None else 2
            n = len(frames) * K
            d_out = torch.full((n * M * M * 4 + GUARD,), PATTERN, dtype=torch.uint8, device=d_in.device)
            torch.cuda.synchronize()
            ctx.float_bev_device(len(frames), d_in.data_ptr(), offs, d_out.data_ptr(), interval, True, poses=ps)
            ctx.synchronize()
            host = d_out.cpu().numpy()
            assert (host[n * M * M * 4:] == PATTERN).all(), "something was written behind d_out"
            got = host[:n * M * M * 4].view(np.float32).reshape(len(frames), K, M, M)
            for f, cloud in enumerate(frames):
                for k in range(K):
                    assert got[f, k].tobytes() == want(cloud, True, None if ps is None else ps[f, k]).tobytes(), (f, k)
        got = ctx.float_bev_batch(frames, interval, False, poses=poses[:, :1])
        for f, cloud in enumerate(frames):
            assert got[f, 0].tobytes() == want(cloud, False, poses[f, 0]).tobytes(), f
        got = ctx.float_bev_batch(frames, interval, True)
        for f, cloud in enumerate(frames):
            assert got[f, 0].tobytes() == want(cloud, True).tobytes(), f
    finally:
        ctx.close()
