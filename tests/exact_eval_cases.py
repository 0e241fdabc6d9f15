"""Inputs of the per-function host/device comparison (bev_debug_exact_eval against tests/exacteval): seeded,
deterministic, every set at most 2^21 elements.  sets(name) lists the (set name, input arrays, params) of one function of
bev_amd.EXACT_EVAL; the arrays of a set are in the function's own argument order."""
from __future__ import annotations

import functools

import numpy as np

F32, F64, U32 = np.float32, np.float64, np.uint32
SEED = 0x5EED
MAX_SET = 1 << 21
FLT_TRUE_MIN = np.array([1], U32).view(F32)[0]
# hostcheck.cpp, hc_exhaustive_exact_forms: (MAX_RANGE, interval)
RANGE_INTERVAL = ((112.0, 1.0), (8.0, 1.0), (50.0, 0.25), (80.0, 0.5), (100.0, 0.4), (2048.0, 8.0), (3.0, 0.375))
BIN_M = (2, 16, 112, 224, 448, 512, 4096)
COLUMNS = (1024, 1056, 2083)
# fd_atanf's thresholds and fd_atan2f's x == 1.0f (bev_libm.h)
ATANF_THRESHOLD_BITS = (0x4C000000, 0x3EE00000, 0x31000000, 0x3F980000, 0x3F300000, 0x401C0000)
# (MAX_RANGE, interval, HEIGHT_RES, lidar_to_ground, n_layers) of bev_code: the three sensors' and one of no power of two
BEV_CODE_CONFIGS = ((112, 1.0, 0.5, 2.0, 24), (112, 1.0, 0.25, 2.0, 24), (112, 1.0, 1.0, 2.0, 24), (100, 0.4, 0.3, 1.7, 20))


def _rng(tag: int):
    return np.random.default_rng([SEED, tag])


def _bits32(b):
    return np.ascontiguousarray(np.asarray(b, np.int64) & 0xFFFFFFFF, np.int64).astype(U32).view(F32)


def around32(values, k: int):
    """every float within k ulps of each value (the zeros are one point of the ordered line; NaN patterns past infinity stay)"""
    b = np.ascontiguousarray(values, F32).view(U32).astype(np.int64)
    o = np.where(b & 0x80000000, -(b & 0x7FFFFFFF), b)[:, None] + np.arange(-k, k + 1)[None, :]
    o = np.clip(o, -0x7FFFFFFF, 0x7FFFFFFF).reshape(-1)
    return _bits32(np.where(o < 0, 0x80000000 | -o, o))


def around64(values, k: int):
    b = np.ascontiguousarray(values, F64).view(np.int64)
    o = np.where(b < 0, -(b & 0x7FFFFFFFFFFFFFFF), b)[:, None] + np.arange(-k, k + 1)[None, :]
    o = o.reshape(-1)
    return np.where(o < 0, np.int64(-0x8000000000000000) | -o, o).astype(np.int64).view(F64)


@functools.lru_cache(None)
def every_exponent_f32():
    """both signs, every exponent field; mantissas 0, 1, the middle, all ones and 60 seeded ones: 32768 floats"""
    rng = _rng(1)
    mant = np.concatenate([np.broadcast_to(np.array([0, 1, 0x400000, 0x7FFFFF]), (512, 4)), rng.integers(0, 1 << 23, (512, 60))], 1)
    se = np.arange(512)[:, None]  # sign and exponent field
    return _bits32(((se >> 8) << 31 | (se & 255) << 23 | mant).reshape(-1))


@functools.lru_cache(None)
def every_exponent_f64():
    rng = _rng(2)
    mant = np.concatenate([np.broadcast_to(np.array([0, 1, 1 << 51, (1 << 52) - 1]), (4096, 4)), rng.integers(0, 1 << 52, (4096, 60))], 1)
    se = np.arange(4096, dtype=np.uint64)[:, None]
    bits = ((se >> np.uint64(11)) << np.uint64(63)) | ((se & np.uint64(2047)) << np.uint64(52)) | mant.astype(np.uint64)
    return bits.reshape(-1).view(F64)


@functools.lru_cache(None)
def thin_f32(n_exp: int = 30):
    """about 6 * n_exp values of the every-exponent vector: zeros, subnormals, infinities and NaNs among them"""
    exps = {30: (0, 1, 2, 30, 60, 66, 67, 90, 100, 110, 117, 120, 124, 125, 126, 127, 128, 129, 130, 134, 137, 150, 160,
                 187, 188, 200, 230, 253, 254, 255),
            7: (0, 1, 100, 126, 127, 140, 255)}[n_exp]
    rng = _rng(3)
    out = []
    for s in (0, 1):
        for e in exps:
            for m in (0, 0x7FFFFF, int(rng.integers(1, 1 << 23))):
                out.append(s << 31 | e << 23 | m)
    return _bits32(out)


def _cross(a, b):
    return np.repeat(a, len(b)), np.tile(b, len(a))


@functools.lru_cache(None)
def seeded_pairs(n: int = 1 << 20):
    """(y, x) in the three families of hc_libm_vs_host: any bit patterns; a 2^-10 grid over +-512; scaled against each other"""
    rng = _rng(4)
    m = n // 3
    y0, x0 = _bits32(rng.integers(0, 1 << 32, m)), _bits32(rng.integers(0, 1 << 32, m))
    y1 = ((rng.integers(0, 1 << 20, m) - 524288) / 1024.0).astype(F32)
    x1 = ((rng.integers(0, 1 << 20, m) - 524288) / 1024.0).astype(F32)
    sc = np.ldexp(F32(1), rng.integers(-40, 40, n - 2 * m)).astype(F32)
    y2 = (sc * (rng.integers(0, 1 << 16, n - 2 * m) - 32768).astype(F32) / F32(777)).astype(F32)
    x2 = ((rng.integers(0, 1 << 16, n - 2 * m) - 32768).astype(F32) / F32(333) / sc).astype(F32)
    return np.concatenate([y0, y1, y2]), np.concatenate([x0, x1, x2])


@functools.lru_cache(None)
def pairs():
    """(y, x): the cross product of the thinned every-exponent vector, then the seeded pairs"""
    cy, cx = _cross(thin_f32(), thin_f32())
    sy, sx = seeded_pairs()
    return np.concatenate([cy, sy]), np.concatenate([cx, sx])


@functools.lru_cache(None)
def radii():
    return np.concatenate([np.array([2.0 ** -6, 1, 8, 64], F64), _rng(5).uniform(3, 90, 3).astype(F32).astype(F64)])


@functools.lru_cache(None)
def column_edges(k: int = 2):
    """(y, x) on every column edge (c + 0.5) / C * 2 pi of C = 1024, 1056, 2083 and on the seams (0 / 360 and +-180), at
    seven radii, y moved by -k .. +k ulps (an ulp of y is not an ulp of the azimuth: at k = 2 under half of the edges are
    straddled, at k = 8 nearly all)"""
    ang = np.concatenate([(np.arange(C) + 0.5) / C * 2 * np.pi for C in COLUMNS] + [np.array([0.0, np.pi, 2 * np.pi])])
    a, r = _cross(ang, radii())
    x = (r * np.cos(a)).astype(F32)
    y = (r * np.sin(a)).astype(F32)
    y[a == 0.0] = 0.0
    return around32(y, k), np.repeat(x, 2 * k + 1)


def column_edges_wide():
    return column_edges(8)


@functools.lru_cache(None)
def oxford_row_edges():
    """(x, y, z) on the elevations 10.67 - (r + 0.5) * 1.3335 degrees, r = -1 .. 32, the same radii, 16 azimuths, z moved
    by -2 .. +2 ulps"""
    el = np.deg2rad(10.67 - (np.arange(-1, 33) + 0.5) * 1.3335)
    az = np.concatenate([np.deg2rad([0, 90, 180, 270]), _rng(6).uniform(0, 2 * np.pi, 12)])
    e, r = _cross(el, radii())
    e, a = _cross(e, az)
    r = np.repeat(r, len(az))
    x = (r * np.cos(e) * np.cos(a)).astype(F32)
    y = (r * np.cos(e) * np.sin(a)).astype(F32)
    z = (r * np.sin(e)).astype(F32)
    return np.repeat(x, 5), np.repeat(y, 5), around32(z, 2)


@functools.lru_cache(None)
def subnormal_pairs():
    """(y, x): y subnormal, +-0 or at the ends of the normal range against x of both signs over every sixth exponent and the
    subnormals: quotients that are subnormal, that underflow and that overflow; y down to +-FLT_TRUE_MIN"""
    rng = _rng(7)
    ymag = np.concatenate([[0, 1, 2, 3, 0x7FFFFF, 0x800000, 0x800001, 0x1000000, 0x7F7FFFFF, 0x7E800000, 0x71800000],
                           rng.integers(1, 1 << 23, 40), rng.integers(0x800000, 0x2000000, 12)])
    xmag = np.concatenate([(np.arange(1, 255, 6) << 23), (np.arange(1, 255, 6) << 23) | rng.integers(0, 1 << 23, 43),
                           [1, 0x7FFFFF, 0x400000], rng.integers(1, 1 << 23, 8)])
    y = _bits32(np.concatenate([ymag, ymag | 0x80000000]))
    x = _bits32(np.concatenate([xmag, xmag | 0x80000000]))
    return _cross(y, x)


@functools.lru_cache(None)
def atan2_branches():
    """(y, x): exponent differences of 58 .. 62 either way with mantissas that straddle (iy - ix) >> 23 == +-60, all sign
    pairs; x within 256 ulps of 1.0f against the thinned vector and fd_atanf's thresholds"""
    rng = _rng(8)
    mant = np.concatenate([[0, 1, 0x7FFFFF, 0x400000], rng.integers(0, 1 << 23, 4)])
    ys, xs = [], []
    for ey in (1, 64, 127, 190, 254):
        for d in (-62, -61, -60, -59, -58, 58, 59, 60, 61, 62):
            ex = ey - d
            if not 1 <= ex <= 254:
                continue
            my, mx = _cross(mant, mant)
            for sy in (0, 1):
                for sx in (0, 1):
                    ys.append(sy << 31 | ey << 23 | my)
                    xs.append(sx << 31 | ex << 23 | mx)
    one = around32(np.array([1.0, -1.0], F32), 256)
    yv = np.concatenate([thin_f32(), around32(_bits32(ATANF_THRESHOLD_BITS), 4), -around32(_bits32(ATANF_THRESHOLD_BITS), 4)])
    oy, ox = _cross(yv, one)
    return np.concatenate([_bits32(np.concatenate(ys)), oy]), np.concatenate([_bits32(np.concatenate(xs)), ox])


@functools.lru_cache(None)
def unary_branches():
    """every float within 256 ulps of a branch constant of a one-argument function, both signs: fd_atanf's six thresholds,
    cvtt's 2^31, floor_half_to_int's -FLT_TRUE_MIN (around zero), the rasters' and the projections' literals"""
    v = np.concatenate([_bits32(ATANF_THRESHOLD_BITS + (0x3F800000, 0x4F000000, 0x3E348F0F, 0x00800000, 0x7F800000)),
                        np.array([0.0, 2147483000.0, 360.0, 180.0, 90.0, 0.3, 0.5, 2.0, 65536.0, 65535.0, 1024.0, 1056.0, 2083.0,
                                  4096.0, 4095.0, 2.0 ** -55, 2.0 ** 22, 2.0 ** 23, 2.0 ** 24, 2.0 ** 32, np.pi / 2, np.pi, np.pi / 4,
                                  2.0 ** 125, 2.0 ** 126, 2.0 ** -126, 75.0, 50.0, 150.0, 100.0, 10.67, 63.75, 0.25], F32)])
    return around32(np.concatenate([v, -v]), 256)


@functools.lru_cache(None)
def unary_grid():
    """k / 4 for k = -16 .. 16400 (every bin, half-bin and height step up to M = 4096), each -2 .. +2 ulps"""
    return around32((np.arange(-16, 16401) / 4.0).astype(F32), 2)


@functools.lru_cache(None)
def unary_angles():
    """the column edges as angles, in radians and in degrees, both signs, each -2 .. +2 ulps"""
    frac = np.concatenate([(np.arange(C) + 0.5) / C for C in COLUMNS] + [np.array([0.0, 0.5, 1.0])])
    v = np.concatenate([frac * 2 * np.pi, frac * 360.0]).astype(F32)
    return around32(np.concatenate([v, -v]), 2)


def _unary32():
    return [("every_exponent", (every_exponent_f32(),), None), ("branch_constants", (unary_branches(),), None),
            ("quarter_grid", (unary_grid(),), None), ("column_angles", (unary_angles(),), None)]


@functools.lru_cache(None)
def f64_branches():
    """every double within 256 ulps of: the high-word thresholds of fd_sin / fd_cos and fd_rem_pio2, the multiples of pi/4 up to 64,
    2^20 pi/2, cvtt's +-2^31 and -2^31 - 1"""
    hi = np.array([0x3E400000, 0x3FD33333, 0x3FE90000, 0x3FE921FB, 0x3FE921FC, 0x3FF921FB, 0x3FF921FC, 0x4002D97C, 0x413921FB,
                   0x413921FC], np.int64)
    v = np.concatenate([(hi << 32).view(F64), np.arange(1, 83) * (np.pi / 4), [2.0 ** 20 * (np.pi / 2), 2.0 ** 31, 2147483649.0,
                        0.0, 2.0 ** -27, 0.3, 0.28125, 0.78125, 1.0, 2.0 ** 52, 2.0 ** 63]])
    return around64(np.concatenate([v, -v]), 256)


@functools.lru_cache(None)
def f64_sweep():
    """seeded arguments over fd_rem_pio2's ranges: +-4 pi uniform, 2^-30 .. past 2^20 pi/2 log-uniform, and n pi/2 within a few
    ulps for n up to 2^20 (the cancellation rounds)"""
    rng = _rng(9)
    a = rng.uniform(-4 * np.pi, 4 * np.pi, 1 << 17)
    b = np.exp2(rng.uniform(-30, 20.8, 1 << 17)) * rng.choice([-1.0, 1.0], 1 << 17)
    n = np.concatenate([np.arange(1, 4097), rng.integers(1, 1 << 20, 8192)]).astype(F64)
    c = around64(n * (np.pi / 2), 2)
    return np.concatenate([a, b, c, -c])


def _unary64():
    return [("every_exponent", (every_exponent_f64(),), None), ("branch_constants", (f64_branches(),), None),
            ("sweep", (f64_sweep(),), None)]


@functools.lru_cache(None)
def triples():
    """(a, b, c): the cube of a 42-value thinning of the every-exponent vector, then 2^18 seeded triples (any bit patterns;
    sweep-like coordinates; coordinates scaled against each other)"""
    t = thin_f32(7)
    a, b = _cross(t, t)
    a, c = _cross(a, t)
    b = np.repeat(b, len(t))
    rng = _rng(10)
    m = 1 << 16
    r0 = [_bits32(rng.integers(0, 1 << 32, m)) for _ in range(3)]
    r1 = [rng.uniform(-120, 120, 2 * m).astype(F32), rng.uniform(-120, 120, 2 * m).astype(F32), rng.uniform(-8, 30, 2 * m).astype(F32)]
    sc = np.ldexp(F32(1), rng.integers(-40, 40, m)).astype(F32)
    r2 = [(sc * rng.normal(0, 1, m)).astype(F32), (rng.normal(0, 1, m) / sc).astype(F32), rng.normal(0, 1, m).astype(F32)]
    return tuple(np.concatenate([u, v, w, x]) for u, v, w, x in zip((a, b, c), r0, r1, r2))


@functools.lru_cache(None)
def angle_threshold_triples(n: int = 1 << 18):
    """(dx, dy, dz) with |dz| / hypot(dx, dy) within 8 ulps of the tangent threshold"""
    rng = _rng(11)
    s = np.ldexp(1.0 + rng.random(n), rng.integers(-20, 20, n)).astype(F32)
    t = (np.float64(0.17632698070846498) * s.astype(F64)).astype(F32)
    dz = (t.view(U32).astype(np.int64) + rng.integers(-8, 9, n)).astype(U32).view(F32)
    dz = np.where(rng.random(n) < 0.5, -dz, dz).astype(F32)
    ang = rng.random(n) * 2 * np.pi
    return (s.astype(F64) * np.cos(ang)).astype(F32), (s.astype(F64) * np.sin(ang)).astype(F32), dz


def _bin_edges(R: float, interval: float):
    """coordinates p with (p + R) / interval on every bin edge of the image, two bins beyond it included, -2 .. +2 ulps"""
    M = int(F32(R * 2) / F32(interval))
    return around32((np.arange(-2, M + 3) * np.float64(F32(interval)) - R).astype(F32), 2)


@functools.lru_cache(None)
def bev_bin_edges():
    p = [_bin_edges(R, i) for R, i in RANGE_INTERVAL]
    return (np.concatenate(p), np.concatenate([np.full(len(q), R, F32) for q, (R, _) in zip(p, RANGE_INTERVAL)]),
            np.concatenate([np.full(len(q), i, F32) for q, (_, i) in zip(p, RANGE_INTERVAL)]))


@functools.lru_cache(None)
def bev_bin_exponents():
    e = every_exponent_f32()
    return (np.tile(e, len(RANGE_INTERVAL)), np.repeat(np.array([r for r, _ in RANGE_INTERVAL], F32), len(e)),
            np.repeat(np.array([i for _, i in RANGE_INTERVAL], F32), len(e)))


@functools.lru_cache(None)
def shifted_bins():
    """(v, M): v = (p + R) scaled by the interval as bev_bin_rp computes it, p on the bin edges — bin_of_shifted's domain"""
    p, R, i = bev_bin_edges()
    pow2 = np.frexp(i)[0] == 0.5
    with np.errstate(all="ignore"):
        v = np.where(pow2, (p + R) * (F32(1) / i), (p + R) / i).astype(F32)
    return v, ((R * F32(2)) / i).astype(np.int64).astype(U32)


@functools.lru_cache(None)
def value_times_m():
    v = np.concatenate([every_exponent_f32(), unary_branches(), unary_grid()])
    return np.tile(v, len(BIN_M)), np.repeat(np.array(BIN_M, U32), len(v))


@functools.lru_cache(None)
def cell_edges():
    """(x, y) on the edges of the 2 m ground cells, one cell beyond the grid included, -2 .. +2 ulps"""
    x = around32((2.0 * np.arange(-1, 77) - 75.0).astype(F32), 2)
    y = around32((2.0 * np.arange(-1, 52) - 50.0).astype(F32), 2)
    return _cross(x, y)


COUNT_STEPS = 1 << 24


@functools.lru_cache(None)
def count_sequence():
    """the reference's count after k ground points, k < 2^24: cnt = 0.01f, then cnt = cnt + 1 in float, step by step
    (numpy's cumulative sum of float32 adds in order)"""
    a = np.ones(COUNT_STEPS, F32)
    a[0] = F32(0.01)
    return np.cumsum(a, dtype=F32)


@functools.lru_cache(None)
def count_cases():
    """(k, n): start after k steps, advance n — the binade crossings hc_count_advance_check walks: from 0.01f every n up to
    2^16 and n within 3 of every power of two; starts within 4 steps of every power of two with runs of 1 .. 9; seeded
    starts with runs up to 700"""
    rng = _rng(12)
    pw = (1 << np.arange(1, 24))
    near = (pw[:, None] + np.arange(-3, 4)[None, :]).reshape(-1)
    k0 = [np.zeros(1 << 16, np.int64), np.zeros(len(near), np.int64)]
    n0 = [np.arange(1, (1 << 16) + 1), near]
    ks, ns = _cross((pw[:, None] + np.arange(-4, 5)[None, :]).reshape(-1), np.arange(1, 10))
    kr = rng.integers(0, COUNT_STEPS - 800, 1 << 16)
    nr = rng.integers(1, 701, 1 << 16)
    k = np.concatenate(k0 + [ks, kr])
    n = np.concatenate(n0 + [ns, nr])
    ok = (k >= 0) & (n >= 1) & (k + n < COUNT_STEPS)
    return k[ok], n[ok]


@functools.lru_cache(None)
def zero_crossing_azimuths():
    """(az_prev, az) around az == 0: the cross product of +-0, +-FLT_TRUE_MIN, subnormals, small normals, 180, 360 and NaN"""
    mag = np.array([0, 1, 2, 0x7FFFFF, 0x800000, 0x800001, 0x34000000, 0x3F800000, 0x43340000, 0x43B40000, 0x7F800000, 0x7FC00000])
    v = _bits32(np.concatenate([mag, mag | 0x80000000]))
    return _cross(v, v)


TRANSFORMS = (
    (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0),
    (0.8660254, -0.5, 0, 1.5, 0.5, 0.8660254, 0, -2.25, 0, 0, 1, 0.125),
    (-0.71270514, 0.6971142, 0.07845911, -31.7, -0.7013291, -0.7092596, -0.0688132, 12.3, 0.00767712, -0.10406928, 0.9945403, 0.4),
    (3.0e10, -1.0e-12, 7.0, 1.0e20, 1.0e-30, 2.5, -3.0e-38, -1.0e-38, 0.333, 1.0e38, -0.1, 5.0e-45),
)


@functools.lru_cache(None)
def bev_code_points(cfg: int):
    """(px, py, pz): x and y on the bin edges of the configuration's image, z on its layer edges ((k + 0.5 - l2g) * res) and
    height steps (k / 4 - l2g), 2^17 seeded combinations; then the triples"""
    R, interval, res, l2g, layers = BEV_CODE_CONFIGS[cfg]
    rng = _rng(20 + cfg)
    e = _bin_edges(R, interval)
    z = around32(np.concatenate([(np.arange(-2, layers + 2) + 0.5 - np.float64(F32(l2g))) * np.float64(F32(res)),
                                 np.arange(-2, 259) / 4.0 - np.float64(F32(l2g))]).astype(F32), 2)
    m = 1 << 17
    t = triples()
    return (np.concatenate([rng.choice(e, m), t[0]]), np.concatenate([rng.choice(e, m), t[1]]), np.concatenate([rng.choice(z, m), t[2]]))


def _yx_sets(swap: bool, with_k: bool = False):
    out = []
    for name, f in (("pairs", pairs), ("column_edges", column_edges), ("column_edges_wide", column_edges_wide),
                    ("subnormal_quotients", subnormal_pairs),
                    ("branch_constants", atan2_branches)):
        y, x = f()
        arrs = (x, y) if swap else (y, x)
        if with_k:
            arrs = (np.arange(len(x), dtype=U32),) + arrs
        out.append((name, arrs, None))
    return out


def sets(name: str):
    """[(set name, input arrays in the function's argument order, params or None)] of one function of bev_amd.EXACT_EVAL"""
    if name in ("fd_atanf", "kitti_col", "cvtt_f32", "floor_half_to_int", "round_half_up_bin", "height_times4", "exact_reciprocal",
                "degrees_of", "wrap_azimuth", "to_u16"):
        return _unary32()
    if name in ("fd_sin", "fd_cos", "cvtt_f64"):
        return _unary64()
    if name == "fd_atan2f":
        return _yx_sets(False)
    if name in ("kitti_azimuth", "kitti_col_xy"):
        return _yx_sets(True)
    if name == "project_mulran":
        return _yx_sets(True, True)
    if name == "kitti_crossing":
        return [("pairs", pairs(), None), ("zero_crossings", zero_crossing_azimuths(), None)]
    if name == "ground_cell":
        return [("pairs", pairs()[::-1], None), ("cell_edges", cell_edges(), None)]
    if name == "project_oxford":
        y, x = column_edges()
        z = (np.hypot(x.astype(F64), y.astype(F64)) * np.tan(np.deg2rad(_rng(13).uniform(-31, 11, len(x))))).astype(F32)
        return [("row_edges", oxford_row_edges(), None), ("column_edges", (x, y, z), None), ("triples", triples(), None)]
    if name in ("angle_is_ground", "angle_is_ground_nodiv"):
        return [("triples", triples(), None), ("threshold", angle_threshold_triples(), None)]
    if name == "bev_bin":
        return [("bin_edges", bev_bin_edges(), None), ("every_exponent", bev_bin_exponents(), None)]
    if name in ("bin_in_range", "bin_of_shifted"):
        return [("values_times_m", value_times_m(), None), ("shifted", shifted_bins(), None)]
    if name == "count_advance":
        k, n = count_cases()
        return [("binade_crossings", (count_sequence()[k], n.astype(U32)), None)]
    if name == "transform_xyz":
        return [(f"matrix{j}", triples(), np.array(m, F32)) for j, m in enumerate(TRANSFORMS)]
    if name == "bev_code":
        return [(f"config{j}", bev_code_points(j), np.array(c, F32)) for j, c in enumerate(BEV_CODE_CONFIGS)]
    raise KeyError(name)


# ---- frames of raw returns made from the edge sets, for the projection kernels that inline these functions ----
def mulran_edge_frame():
    """(n, 4) XYZI: every column-edge return, then the subnormal quotients"""
    y = np.concatenate([column_edges()[0], subnormal_pairs()[0]])
    x = np.concatenate([column_edges()[1], subnormal_pairs()[1]])
    return np.ascontiguousarray(np.stack([x, y, np.full_like(x, 0.5), np.ones_like(x)], 1))


def oxford_edge_frame():
    """(4, n) planes as the selector reads them (it flips x and z): the row-edge returns, then the column-edge ones"""
    (_, rows, _), (_, cols, _) = sets("project_oxford")[:2]
    x, y, z = (np.concatenate([a, b]) for a, b in zip(rows, cols))
    return np.ascontiguousarray(np.stack([-x, y, -z, np.ones_like(x)], 0))


def kitti_edge_frame():
    """(n, 4) XYZI in file order: 63 rings, each one turn over the 2083 column edges at one radius and one move of y
    (-8 .. +8 ulps), so that every ring starts with an azimuth zero crossing after more than 0.6 * 2083 returns"""
    ang = (np.arange(2083) + 0.5) / 2083 * 2 * np.pi
    xs, ys = [], []
    for r in radii():
        x = (r * np.cos(ang)).astype(F32)
        y = around32((r * np.sin(ang)).astype(F32), 8).reshape(2083, 17)
        for move in (-8, -4, -2, -1, 0, 1, 2, 4, 8):
            xs.append(x)
            ys.append(y[:, move + 8])
    x, y = np.concatenate(xs), np.concatenate(ys)
    return np.ascontiguousarray(np.stack([x, y, np.full_like(x, -1.0), np.ones_like(x)], 1))
