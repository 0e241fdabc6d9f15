"""CPU: the raster configurations bev_create admits beyond the reference's (tests/raster_cases.py).
  - which image sizes validate_params admits, and how fill_geometry cuts each into bands (csrc/bev_exact.h
    raster_band_layout);
  - the generalised checker: oracle_multi_bev_ex / oracle_single_bev_ex equal the fixed entry points at the reference's
    literals and equal the Python restatement at every listed configuration;
  - the closed forms the kernels evaluate (tests/hostcheck) against that checker at every listed configuration."""
import ctypes as C

import numpy as np
import pytest

import bev_amd
import hostcheck_lib as hc
import oracle_lib as orc
import py_restatement as py
import raster_cases as rc
from bev_amd import POINT_DTYPE, synth

CASE_IDS = [n for n, _ in rc.ALL_CASES]


# ---- admitted sizes --------------------------------------------------------------------------------------------------
def _bytes(max_range, interval=1.0, n_layers=24):
    p = rc.small_params(max_range=max_range, interval=interval, n_layers=n_layers)
    lib = bev_amd.load_lib()
    return int(lib.bev_multi_bytes(C.byref(p))), int(lib.bev_single_bytes(C.byref(p)))


def test_admitted_image_sizes():
    """M = 16 .. 512 in steps of 16 (max_range = 8 k, interval 1): nine sizes have no band height whose LDS planes fit and
    are refused, every other one is sized n_layers * M * M; so are M = 8 and M = 528"""
    refused = []
    for k in range(1, 33):
        M = 16 * k
        multi, single = _bytes(8 * k)
        if multi == 0:
            refused.append(M)
            assert single == 0
        else:
            assert (multi, single) == (24 * M * M, M * M), M
            assert _bytes(8 * k, n_layers=30)[0] == 30 * M * M and _bytes(8 * k, n_layers=1)[0] == M * M
    assert tuple(refused) == rc.REFUSED_SIZES
    assert _bytes(4) == (0, 0) and _bytes(264) == (0, 0)           # M = 8, M = 528
    assert _bytes(100) == (0, 0)                                    # M = 200: not a multiple of 16
    for name, f in rc.ALL_CASES:                                    # every listed configuration is one bev_create admits
        p = rc.small_params(**f)
        assert bev_amd.load_lib().bev_multi_bytes(C.byref(p)) == p.n_layers * p.mat_size ** 2 and p.mat_size % 16 == 0, name
    h = C.c_void_p()
    p = rc.small_params(max_range=152)                              # M = 304
    assert bev_amd.load_lib().bev_create(C.byref(h), 0, C.byref(p), 1, 1000) == -5


def _layout_restated(M):
    """raster_bands_for + raster_band_layout restated: (u, bands, coarse, fine, z0, z1, LDS bytes)"""
    tail = 280 + 4 + 2
    u = next((b for b in (8, 16, 32, 64) if M % b == 0 and (2 * (M // b) * M + tail) * 4 <= 40960), 0)
    if not u:
        return None
    coarse = M // u
    fine = coarse // 2 if coarse % 2 == 0 else coarse
    z0 = (3 * u // 8) * coarse
    z1 = M - z0
    if 2 * (z0 // coarse) + (z1 - z0) // fine > 64:
        fine = coarse
    return dict(u=u, bands=2 * (z0 // coarse) + (z1 - z0) // fine, coarse=coarse, fine=fine, z0=z0, z1=z1,
                lds_bytes=(2 * coarse * M + tail) * 4, violations=0)


def test_band_layout_of_every_admitted_size():
    """hostcheck's copy of raster_bands_for admits what the library admits; for each of the 23 sizes the layout
    raster_band_layout produces has at most kMaxBands bands, zone borders on band borders, bands that tile [0, M) exactly,
    raster_band_of_nodiv == raster_band_of == the covering band, planes under the LDS cap (hc_band_layout counts
    violations) — and is the layout a restatement in Python gives"""
    shapes = set()
    for M in range(16, 513, 16):
        got = hc.band_layout(M)
        if M in rc.REFUSED_SIZES:
            assert got["u"] == 0 and _layout_restated(M) is None, M
            continue
        assert got == _layout_restated(M), (M, got)
        assert got["violations"] == 0 and got["bands"] <= 64, (M, got)
        shapes.add((got["u"], got["coarse"] == got["fine"], got["bands"]))
    lay = {M: hc.band_layout(M) for M in rc.ADMITTED_SIZES}
    assert (lay[16]["coarse"], lay[16]["fine"]) == (2, 1) and lay[48]["fine"] == 3
    for M in (208, 240, 272):
        assert lay[M]["coarse"] % 2 == 1 and lay[M]["fine"] == lay[M]["coarse"] and lay[M]["bands"] == 16, lay[M]
    assert lay[192]["lds_bytes"] == lay[384]["lds_bytes"] == 38008 and lay[272]["lds_bytes"] == 38136
    assert all(lay[M]["u"] == 32 for M in range(288, 385, 16) if M in lay)
    assert (lay[512]["u"], lay[512]["bands"], lay[512]["fine"]) == (64, 64, 8)
    assert hc.lib().hc_small_div_check() == 0
    print("band shapes (u, uniform, bands):", sorted(shapes))


# ---- the generalised checker -----------------------------------------------------------------------------------------
def _kat_clouds():
    """the points of tests/test_oracle_kat.py's hand-derived raster answers (bin edges, both clamps, layer 23 / 24, label 0)
    as one cloud, and the frames the oracle-vs-closed-form tests run"""
    p32, p64 = bev_amd.params_for_sensor("HDL_32E"), bev_amd.params_for_sensor("OS1_64")
    kat = np.zeros(12, POINT_DTYPE)
    kat["x"] = [0, -112.5, -113.0, 110.4, 111.0, 0, 0, 0, 0, 0, 0, 0]
    kat["y"] = [0, -112.5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    kat["z"] = [0, 1.0, 1.0, 1.0, 1.0, 1.0, 100.0, -5.0, -1.73, 10.6, 10.9, 3.0]
    kat["label"] = [-2, -2, -2, -2, -2, 0, -2, -2, -2, -2, -2, -2]
    kat["intensity"] = 0.5
    return [(p32, kat), (p32, synth.sweep(p32, 3)), (p32, synth.adversarial(p32, 60000, 1, True)), (p64, synth.firing_order(p64, 2)),
            (p32, np.empty(0, POINT_DTYPE))]


def test_ex_forms_at_the_reference_literals_equal_the_fixed_entry_points():
    for p, pts in _kat_clouds():
        sp = orc.sensor_from_params(p)
        cloud = orc.mark_ground(sp, orc.order_cloud(sp, pts))[0] if len(pts) != 12 else pts   # (the KAT points have no slots)
        for interval in (1.0, 0.5, 2.0):
            assert orc.multi_bev(sp, cloud, interval, 112, 24, 2.0).tobytes() == orc.multi_bev_fixed(sp, cloud, interval).tobytes()
            assert orc.single_bev(cloud, interval, 112, 2.0).tobytes() == orc.single_bev_fixed(cloud, interval).tobytes()
        o_ord, o_gm, o_multi, o_single = orc.process_frame(sp, pts)
        e_ord, e_gm, e_multi, e_single = orc.process_frame_params(p, pts)
        assert o_ord.tobytes() == e_ord.tobytes() and np.array_equal(o_gm, e_gm)
        assert o_multi.tobytes() == e_multi.tobytes() and o_single.tobytes() == e_single.tobytes()


def _small_cloud(p, seed):
    """a few thousand labelled points: the boundary set, an adversarial cloud (non-finite coordinates, labels 0 among
    them) and a scaled sweep"""
    a = synth.adversarial(p, 1500, seed, nonfinite=True).copy()
    s = rc.scale_xy(p, synth.sweep(p, 300 + seed, keep=0.15, n_dup=0).copy())
    b = rc.boundary_points(p, seed)
    b["label"] = -2
    return np.concatenate([b, a, s])


@pytest.mark.parametrize("name,fields", rc.ALL_CASES, ids=CASE_IDS)
def test_ex_forms_equal_the_python_restatement(name, fields):
    p = rc.small_params(**fields)
    cloud = _small_cloud(p, 1)
    assert 1000 < len(cloud) < 8000
    sp = orc.sensor_from_params(p)
    args = (p.interval, p.max_range, p.n_layers, p.lidar_to_ground)
    got_m = orc.multi_bev(sp, cloud, *args)
    got_s = orc.single_bev(cloud, p.interval, p.max_range, p.lidar_to_ground)
    assert got_m.shape == (p.n_layers, p.mat_size, p.mat_size) and got_m.any() and got_s.any()
    assert np.array_equal(got_m, py.multi_bev(cloud, p.height_res, *args))
    assert np.array_equal(got_s, py.single_bev(cloud, p.interval, p.max_range, p.lidar_to_ground))


# ---- the closed forms at these configurations ------------------------------------------------------------------------
@pytest.mark.parametrize("name,fields", rc.ALL_CASES, ids=CASE_IDS)
def test_closed_forms_equal_the_checker(name, fields):
    """hc.process_frame (order, phase A closed form, candidate keys, per-cell sums, codes, rasters from codes) on one frame
    of the small geometry with the boundary set placed, and hc_bev_code per point, against the generalised oracle"""
    p = rc.small_params(**fields)
    frames, bpts = rc.small_frames(p, n_frames=1, seed=2)
    pts = frames[0]
    o_ord, o_gm, o_multi, o_single = orc.process_frame_params(p, pts)
    h_ord, h_gm, _, h_multi, h_single = hc.process_frame(p, pts)
    assert h_ord.tobytes() == o_ord.tobytes() and np.array_equal(h_gm, o_gm)
    assert np.array_equal(h_multi, o_multi) and np.array_equal(h_single, o_single)
    assert (o_gm == 1).sum() > 50 and o_multi.any()
    # bev_code per point against the oracle's rasters of that one point
    sp = orc.sensor_from_params(p)
    M, L = p.mat_size, p.n_layers
    sample = np.concatenate([bpts[::7], rc.survivors([o_ord])[::97]])
    for q in sample:
        code = hc.bev_code(p, q["x"], q["y"], q["z"], -2)
        one = np.array([q], POINT_DTYPE)
        one["label"] = -2
        m = orc.multi_bev(sp, one, p.interval, p.max_range, L, p.lidar_to_ground)
        s = orc.single_bev(one, p.interval, p.max_range, p.lidar_to_ground)
        bins = rc.bins_div(np.array([q["x"], q["y"]], np.float32), p.max_range, p.interval)
        bx, by = int(bins[0]), int(bins[1])
        if not (0 <= bx < M and 0 <= by < M):
            assert code == 0xFFFFFFFF and not m.any() and not s.any(), q
            continue
        assert (code & 511, (code >> 9) & 511) == (bx, by), q
        assert int(s[bx, by]) == (code >> 18) & 255 and np.count_nonzero(s) <= 1, q
        layer = (code >> 26) & 31
        want = np.zeros_like(m)
        if layer != 31:
            want[layer, bx, by] = 255
        assert np.array_equal(m, want), (q, layer)


def test_divide_cases_hold_discriminating_points():
    """what makes the divide cases tests of the DIVISION: the boundary set holds coordinates that a multiplication by
    fl(1 / interval) bins differently and heights that fl(1 / height_res) layers differently.  The bare family (every
    edge and its two float neighbours, on x and on y) holds 10 to 84 such coordinates per listed interval except 0.75 at
    range 72, where it holds none (raster_cases.searched_coords says why), and 4 to 6 such heights per listed resolution; the
    set as placed adds coordinates found within 64 ulps of the edges.  0.625 and 1.25 give none in the bare family."""
    for name, f in rc.DIVIDE_CASES + rc.ROUTE_CASES + rc.OTHER_CASES[:1]:
        p = rc.small_params(**f)
        c, z = rc.boundary_coords(p), rc.boundary_heights(p)
        none = np.empty(0, np.float32)
        bare_b, bare_l = rc.discriminating(p, c, c, none)[0], rc.discriminating(p, none, none, z)[1]
        b = rc.boundary_points(p)
        nb, nl = rc.discriminating(p, b["x"], b["y"], b["z"])
        print(f"{name}: bare family {bare_b} bin coordinates, {bare_l} layer heights; placed set {nb}, {nl}")
        if rc.is_pow2(p.interval):
            assert bare_b == nb == 0
        else:
            assert nb >= 16, (name, bare_b, nb)
        if rc.is_pow2(p.height_res):
            assert bare_l == nl == 0
        else:
            assert bare_l >= 4 and nl >= 6, (name, bare_l, nl)
    for interval in (0.625, 1.25):
        p = rc.small_params(interval=interval, max_range=80)
        c = rc.boundary_coords(p)
        assert rc.discriminating(p, c, c, np.empty(0, np.float32))[0] == 0
