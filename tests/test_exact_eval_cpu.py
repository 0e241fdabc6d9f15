"""CPU: the shared host/device arithmetic (csrc/bev_exact.h, bev_libm.h, bev_libm_f64.h) one function at a time, through the
dispatch the device hook bev_debug_exact_eval runs (csrc/bev_exact_eval.h, built for the host in tests/exacteval), on the
inputs of tests/exact_eval_cases.py:
(1) against plain references — this machine's libm, the ICP checker's independent sin / cos, the reference's literal double
    expressions in numpy float64, the oracle's libm projection;
(2) sharpness: the sets can tell a build that contracts to FMA, and an evaluation under flush-to-zero, from the product's.
tests/test_exact_eval_gpu.py then asks the device for the same bits."""
import math

import numpy as np
import pytest

import bev_amd
import exact_eval_cases as cs
import exacteval_lib as ee
import icp_lib as il
import oracle_lib as orc

F32, F64, U32, I32 = np.float32, np.float64, np.uint32, np.int32
INT_MIN = -(1 << 31)

# ---- sharpness: which mutation moves which function (the counts are in DESIGN.md §6v) ----
FMA_SENSITIVE = ("fd_atanf", "fd_atan2f", "kitti_azimuth", "kitti_col_xy", "project_mulran", "project_oxford", "fd_sin", "fd_cos",
                 "angle_is_ground", "angle_is_ground_nodiv", "transform_xyz")
FTZ_SENSITIVE = ("fd_atan2f", "kitti_azimuth", "kitti_col_xy", "kitti_crossing", "project_mulran", "project_oxford",
                 "floor_half_to_int", "bin_of_shifted", "angle_is_ground", "angle_is_ground_nodiv", "transform_xyz", "degrees_of",
                 "wrap_azimuth")
# neither mutation can move these: no product feeds a sum (nothing to fuse), and a subnormal operand or result ends in
# the same integer, comparison or bit pattern whether it is flushed or not
EXEMPT = {
    "kitti_col": "one sum and one double quotient of a float: no product to fuse, and no double here is subnormal",
    "cvtt_f32": "comparisons and one conversion; a subnormal truncates to 0 like the zero it is flushed to",
    "cvtt_f64": "comparisons and one conversion; a subnormal truncates to 0 like the zero it is flushed to",
    "ground_cell": "x + 75.0f absorbs a subnormal x exactly as it absorbs 0; the rest is floor_half_to_int of a normal number",
    "round_half_up_bin": "floor / ceil and comparisons; only |v| <= 2^-55 is special, and -2^-55 is a normal float",
    "height_times4": "a scaling by 4 that truncates to 0 for every subnormal",
    "bin_in_range": "as round_half_up_bin: its patch for [-2^-55, 0) tests the unflushed input against normal constants",
    "bev_bin": "p + R is R for a subnormal p; the quotient feeds round_half_up_bin",
    "count_advance": "exact additions on a binade's grid, on counts of 0.01 and more",
    "exact_reciprocal": "integer operations on the bit pattern",
    "to_u16": "cvtt_f32 and a truncation",
    "bev_code": "the sums p + R and z + l2g absorb subnormals; every product is a scaling by a power of two or feeds no sum",
}


@pytest.fixture(scope="module", autouse=True)
def _checkers():
    ee.build()
    il.build()


def _same(a, b):
    """bit-equal, except that NaN matches NaN: (mask of differing elements, NaN pairs)"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    ia = a.view({4: U32, 8: np.uint64}[a.itemsize])
    d = ia != b.view(ia.dtype)
    nan = np.zeros(a.shape, bool)
    if a.dtype.kind == "f":
        nan = np.isnan(a) & np.isnan(b)
        d &= ~nan
    return d, int(nan.sum())


def _assert_same(name, set_name, got, want, inputs):
    d, _ = _same(got, want)
    if d.any():
        k = int(np.flatnonzero(d.reshape(len(d), -1).any(1))[0])
        raise AssertionError(f"{name} / {set_name}: {int(d.sum())} differ; first at {k}: inputs "
                             f"{[a[k].tobytes().hex() for a in inputs]} got {got[k]!r} want {want[k]!r}")


def _each(name):
    for set_name, arrs, prm in cs.sets(name):
        yield set_name, arrs, prm, ee.eval(name, *arrs, params=prm)


# ---- plain references, numpy float64 / float32 (IEEE operations, no contraction) ----
def _cvtt(v64):
    """cvttsd2si / cvttss2si of values held in float64"""
    ok = (v64 > -2147483649.0) & (v64 < 2147483648.0)
    with np.errstate(invalid="ignore"):
        return np.where(ok, np.trunc(np.where(ok, v64, 0.0)), INT_MIN).astype(np.int64).astype(I32)


def _round_away(d):
    """C's round(): half away from zero, without adding 0.5 (which rounds for the double below 0.5)"""
    a = np.abs(d)
    f = np.floor(a)
    with np.errstate(invalid="ignore"):
        return np.copysign(np.where(a - f >= 0.5, f + 1.0, f), d)


def _bin_map(b):
    return np.where((b < 0) | (b >= 4096), -1, b)


def _ref_round_half_up(v):
    with np.errstate(invalid="ignore"):  # (a signalling NaN among the bit patterns)
        return _cvtt(_round_away(v.astype(F64) + 0.5))


def _ref_degrees(rad):
    return (rad.astype(F64) / np.pi * 180.0).astype(F32)


def _ref_wrap(az):
    with np.errstate(invalid="ignore"):
        return np.where(az > F32(360), az - F32(360), np.where(az < F32(0), az + F32(360), az)).astype(F32)


def _ref_kitti_col(az):
    with np.errstate(invalid="ignore"):
        a = np.where(az >= F32(360), az - F32(360), np.where(az < F32(0), az + F32(360), az)).astype(F32)
        c = _cvtt(_round_away(a.astype(F64) / (360.0 / 2083))).astype(np.int64)
    c = np.where(c >= 2083, c - 2083, np.where(c < 0, c + 2083, c))
    return np.where((c >= 0) & (c < 2083), c, -1).astype(I32)


def _ref_bev_bin(p, R, interval):
    with np.errstate(all="ignore"):
        return _ref_round_half_up(((p + R).astype(F32) / interval).astype(F32))


REFS = {
    "fd_atanf": lambda x: ee.libm_atanf(x),
    "fd_atan2f": lambda y, x: ee.libm_atan2f(y, x),
    "kitti_azimuth": lambda x, y: _ref_degrees(ee.libm_atan2f(y, x)),
    "kitti_col": _ref_kitti_col,
    "kitti_col_xy": lambda x, y: _ref_kitti_col(_ref_degrees(ee.libm_atan2f(y, x))),
    "kitti_crossing": lambda a, b: ((a <= 0) & (b > 0)).astype(I32),
    "cvtt_f32": lambda v: _cvtt(v.astype(F64)),
    "cvtt_f64": _cvtt,
    "floor_half_to_int": lambda n: _cvtt(np.floor(n.astype(F64) / 2.0)),                       # hostcheck.cpp, form 1
    "height_times4": lambda t: _cvtt(t.astype(F64) * 4.0),                                     # form 3
    "degrees_of": _ref_degrees,
    "wrap_azimuth": _ref_wrap,
    "to_u16": lambda v: (_cvtt(v.astype(F64)).astype(np.int64) & 0xFFFF).astype(I32),
    "bev_bin": _ref_bev_bin,
}


@pytest.mark.parametrize("name", sorted(REFS))
def test_host_header_equals_plain_reference(name):
    """fd_atanf / fd_atan2f against this machine's libm bit for bit (what tests/test_projection_cpu.py presupposes); the
    exact forms against the reference's literal double expressions (hostcheck.cpp, hc_exhaustive_exact_forms) in float64"""
    with np.errstate(all="ignore"):
        for set_name, arrs, _, got in _each(name):
            want = REFS[name](*arrs)
            if name == "bev_bin":
                got, want = _bin_map(got), _bin_map(want)
            _assert_same(name, set_name, got, np.asarray(want, got.dtype), arrs)


def test_round_half_up_and_the_range_forms():
    """forms 2, 5 and 6: round_half_up_bin against cvttsd2si(round((double)v + 0.5)) with everything outside [0, 4096) as one
    value; bin_in_range against that bin being in [0, M); bin_of_shifted against bin_in_range on shifted coordinates"""
    for set_name, arrs, _, got in _each("round_half_up_bin"):
        _assert_same("round_half_up_bin", set_name, _bin_map(got), _bin_map(_ref_round_half_up(arrs[0])), arrs)
    for set_name, (v, M), _, got in _each("bin_in_range"):
        full = _ref_round_half_up(v).astype(np.int64)
        want_in = (full >= 0) & (full < M.astype(np.int64))
        assert np.array_equal(got >> 31 == 1, want_in), set_name
        assert np.array_equal((got & 0x7FFFFFFF)[want_in], full[want_in]), set_name
    v, M = cs.shifted_bins()
    assert np.array_equal(ee.eval("bin_of_shifted", v, M), ee.eval("bin_in_range", v, M))
    full = _ref_round_half_up(v).astype(np.int64)
    assert ((full >= 0) & (full < M)).sum() > len(v) // 2  # the set is inside the images


def test_ground_cell_equals_get_belonging_grid():
    """BatchMultiBevGen.h:73-99 literally: (float)((double)x + 75.0), floor(n / 2.0), clamps"""
    for set_name, (x, y), _, got in _each("ground_cell"):
        with np.errstate(all="ignore"):
            r = _cvtt(np.floor((x.astype(F64) + 75.0).astype(F32).astype(F64) / 2.0))
            c = _cvtt(np.floor((y.astype(F64) + 50.0).astype(F32).astype(F64) / 2.0))
        want = np.clip(r, 0, 74) * 50 + np.clip(c, 0, 49)
        _assert_same("ground_cell", set_name, got, want.astype(I32), (x, y))


def test_count_advance_equals_step_by_step():
    k, n = cs.count_cases()
    (set_name, arrs, _, got), = list(_each("count_advance"))
    _assert_same("count_advance", set_name, got, cs.count_sequence()[k + n], arrs)
    assert len(k) > 100_000 and (k == 0).sum() >= 1 << 16


def test_exact_reciprocal():
    for set_name, (v,), _, got in _each("exact_reciprocal"):
        with np.errstate(all="ignore"):
            pow2 = (np.frexp(v)[0] == 0.5) & (v >= F32(2.0 ** -126)) & (v <= F32(2.0 ** 125))
            want = np.where(pow2, F32(1) / v, F32(0)).astype(F32)
        _assert_same("exact_reciprocal", set_name, got, want, (v,))
        assert not (got[pow2] * v[pow2] != 1).any()


def test_angle_predicates():
    T = np.array([0x3E348F0F], U32).view(F32)[0]
    for name in ("angle_is_ground", "angle_is_ground_nodiv"):
        for set_name, (dx, dy, dz), _, got in _each(name):
            with np.errstate(all="ignore"):
                s = np.sqrt(dx * dx + dy * dy)
                a = np.abs(dz)
                want = ((a == 0) & (s == 0)) | (a / s <= T)
            _assert_same(name, set_name, got, want.astype(I32), (dx, dy, dz))
    dx, dy, dz = cs.angle_threshold_triples()
    lib = orc.lib()
    ref = np.fromiter((lib.oracle_angle_is_ground(float(a), float(b), float(c)) for a, b, c in zip(dx[:50000], dy[:50000], dz[:50000])),
                      I32, 50000)
    assert np.array_equal(ee.eval("angle_is_ground", dx[:50000], dy[:50000], dz[:50000]), ref)  # the libm expression itself


def test_projections_equal_the_oracle():
    """project_mulran / project_oxford against the oracle's literal restatement over this machine's libm"""
    for set_name, (k, x, y), _, got in _each("project_mulran"):
        want = orc.project(0, np.stack([x, y, np.zeros_like(x), np.ones_like(x)], 1))
        assert np.array_equal(k % 64, want["row"]), set_name
        _assert_same("project_mulran", set_name, got, want["row"].astype(U32) | want["col"].astype(U32) << 16, (k, x, y))
    for set_name, (x, y, z), _, got in _each("project_oxford"):
        want = orc.project(1, np.stack([-x, y, -z, np.ones_like(x)], 0))  # (the selector flips x and z first)
        _assert_same("project_oxford", set_name, got, want["row"].astype(U32) | want["col"].astype(U32) << 16, (x, y, z))
        if set_name == "row_edges":
            assert set(np.unique(got & 0xFFFF)) == set(range(32))


def _ulps64(a, b):
    ia, ib = a.view(np.int64), b.view(np.int64)
    return np.abs(np.where(ia < 0, -(ia & 0x7FFFFFFFFFFFFFFF), ia) - np.where(ib < 0, -(ib & 0x7FFFFFFFFFFFFFFF), ib))


def test_sin_cos_equal_the_icp_checker_and_stay_within_one_ulp_of_libm():
    """fd_sin / fd_cos of the product's header: bit-equal to tests/icp's independent restatement of the same published
    algorithm, and within the bound tests/test_icp_cpu.py asserts for that restatement against math.sin / math.cos (1 ulp)"""
    l = il.lib()
    for name, mine, libm in (("fd_sin", l.icp_sin, math.sin), ("fd_cos", l.icp_cos, math.cos)):
        for set_name, (x,), _, got in _each(name):
            xs = x.tolist()
            other = np.array([mine(v) for v in xs], F64)
            _assert_same(name, set_name, got, other, (x,))
            beyond = (((x.view(np.int64) >> 32) & 0x7FFFFFFF) > 0x413921FB)  # past 2^20 pi/2, infinities and NaNs
            assert np.array_equal(np.isnan(got), beyond), (name, set_name)
            ref = np.array([libm(v) for v in x[~beyond].tolist()], F64)
            worst = int(_ulps64(got[~beyond], ref).max())
            print(f"{name} / {set_name}: {int((~beyond).sum())} arguments, worst {worst} ulp from libm")
            assert worst <= 1, (name, set_name)
    assert math.copysign(1.0, float(ee.eval("fd_sin", np.array([-0.0]))[0])) < 0


def test_transform_xyz():
    for set_name, (x, y, z), m, got in _each("transform_xyz"):
        with np.errstate(all="ignore"):
            want = np.stack([m[4 * r] * x + (m[4 * r + 1] * y + (m[4 * r + 2] * z + m[4 * r + 3])) for r in range(3)], 1).astype(F32)
            _assert_same("transform_xyz", set_name, got, want, (x, y, z))
            M = m.astype(F64).reshape(3, 4)
            ref = np.stack([x, y, z, np.ones_like(x)], 1).astype(F64) @ M.T
            scale = np.abs(np.stack([x, y, z, np.ones_like(x)], 1).astype(F64)) @ np.abs(M).T
            # (terms of 1e-30 and more: no subnormal rounding; sums below 1e38: no overflow on the way)
            terms = np.abs(np.stack([x, y, z, np.ones_like(x)], 1).astype(F64))[:, None, :] * np.abs(M)[None, :, :]
            ok = np.isfinite(got) & (scale > 0) & (scale < 1e38) & ((terms == 0) | (terms > 1e-30)).all(2)
            spread = np.abs(got.astype(F64) - ref)[ok] / scale[ok]
        print(f"transform_xyz / {set_name}: float32 association against the float64 product over {int(ok.sum())} finite results, "
              f"relative to sum |m||p|: max {spread.max():.3e}")
        # the deepest term goes through its product's rounding and three sums': (1 + 2^-24)^4 - 1
        assert spread.max() <= (1 + 2.0 ** -24) ** 4 - 1


def test_bev_code_equals_the_literal_rasters():
    """BatchMultiBevGen.cpp:279-285, :343-349 in numpy: float bins through round((double)v + 0.5), layer through roundf, height
    through (int)((double)(z + l2g) * 4.0)"""
    for set_name, (px, py, pz), prm, got in _each("bev_code"):
        R, interval, res, l2g, layers = (F32(v) for v in prm)
        with np.errstate(all="ignore"):
            M = int(F32(int(R) * 2) / interval)
            bx = _ref_bev_bin(px, R, interval).astype(np.int64)
            by = _ref_bev_bin(py, R, interval).astype(np.int64)
            inside = (bx >= 0) & (bx < M) & (by >= 0) & (by < M)
            layer = _cvtt(_round_away(((pz / res).astype(F32) + l2g).astype(F32).astype(F64))).astype(np.int64)
            h = np.clip(_cvtt((pz + l2g).astype(F32).astype(F64) * 4.0), 0, 255).astype(np.int64)
        layer = np.where((layer >= 0) & (layer < int(layers)), layer, 31)
        want = np.where(inside, bx | by << 9 | h << 18 | layer << 26, 0xFFFFFFFF).astype(U32)
        _assert_same("bev_code", set_name, got, want, (px, py, pz))
        assert inside.sum() > 1 << 16


def test_dispatch_table_matches_the_package():
    assert bev_amd.EXACT_EVAL_NAMES[7] == "fd_sin" and len(bev_amd.EXACT_EVAL_NAMES) == ee.lib().ee_count()
    for i, name in enumerate(bev_amd.EXACT_EVAL_NAMES):
        kinds, out_kind, n_params = bev_amd.EXACT_EVAL[name]
        assert ee.signature(i) == (kinds, {"d": 2, "f3": 3}.get(out_kind, 1), n_params), name
        for set_name, arrs, _ in cs.sets(name):
            assert 0 < len(arrs[0]) <= cs.MAX_SET, (name, set_name)
    assert ee.signature(-1) is None and ee.signature(len(bev_amd.EXACT_EVAL_NAMES)) is None
    assert sorted(set(FMA_SENSITIVE) | set(FTZ_SENSITIVE) | set(EXEMPT)) == sorted(bev_amd.EXACT_EVAL_NAMES)
    assert not (set(FMA_SENSITIVE) | set(FTZ_SENSITIVE)) & set(EXEMPT)


def _moved(name, mode):
    total = 0
    for set_name, arrs, prm, plain in _each(name):
        d, _ = _same(plain, ee.eval(name, *arrs, params=prm, mode=mode))
        total += int(d.reshape(len(d), -1).any(1).sum())
    return total


def test_sharpness_flush_to_zero():
    """the sets contain elements on which flushing subnormals changes the result, for every function where it can"""
    counts = {name: _moved(name, "ftz") for name in bev_amd.EXACT_EVAL_NAMES}
    print("elements moved by FTZ|DAZ:", counts)
    for name in FTZ_SENSITIVE:
        assert counts[name] > 0, name
    for name in bev_amd.EXACT_EVAL_NAMES:
        if name not in FTZ_SENSITIVE:
            assert counts[name] == 0, (name, "list it in FTZ_SENSITIVE")


def test_sharpness_contraction():
    """the sets contain elements on which a build contracted to FMA differs, for every function with a product feeding a sum"""
    if not ee.cpu_has_fma():
        pytest.skip("this CPU has no FMA: the contracted build cannot run")
    counts = {name: _moved(name, "fma") for name in bev_amd.EXACT_EVAL_NAMES}
    print("elements moved by -ffp-contract=fast -mfma:", counts)
    for name in FMA_SENSITIVE:
        assert counts[name] > 0, name
    for name in EXEMPT:
        assert counts[name] == 0, name
