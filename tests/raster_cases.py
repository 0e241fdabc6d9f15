"""The raster configurations bev_create admits beyond the reference's own (interval 1, range 112, 24 layers, offset 2):
the list of cases shared by the CPU tests of the checker / the closed forms and by tests/test_raster_params_gpu.py, the
small sensor geometry they run on, and the boundary coordinates that tell a division from a multiplication by a
rounded reciprocal.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import bev_amd
from bev_amd import POINT_DTYPE, synth

F32 = np.float32

# image sizes validate_params admits (M % 16 == 0, 16..512, and a band height whose two LDS planes fit) and refuses
REFUSED_SIZES = (304, 336, 368, 400, 416, 432, 464, 480, 496)
ADMITTED_SIZES = tuple(m for m in range(16, 513, 16) if m not in REFUSED_SIZES)
assert len(ADMITTED_SIZES) == 23

# (name, dict of bev_params_t fields); fields not named keep small_params()'s values
SIZE_CASES = [(f"M{m}", dict(max_range=m // 2, interval=1.0)) for m in ADMITTED_SIZES] + [
    ("M512_quarter", dict(max_range=64, interval=0.25)),     # a 2 m ground cell spans 8 bins: candidate keys escape
    ("M512_half", dict(max_range=128, interval=0.5)),
    ("M16_coarse", dict(max_range=112, interval=14.0)),
]
DIVIDE_CASES = [
    ("i0.7_r0.25", dict(interval=0.7, height_res=0.25)),
    ("i1.75_r0.5", dict(interval=1.75, height_res=0.5)),
    ("i0.875_r0.3", dict(interval=0.875, height_res=0.3)),
    ("i1.0_r0.3", dict(interval=1.0, height_res=0.3)),
    ("i0.4375_r0.4", dict(interval=0.4375, height_res=0.4)),
    ("i0.375_r0.1", dict(interval=0.375, max_range=96, height_res=0.1)),
    ("i0.75_r0.15", dict(interval=0.75, max_range=72, height_res=0.15)),
    ("i3.5_r1.0", dict(interval=3.5, height_res=1.0)),
]
# n_layers x lidar_to_ground in full, max_range rotated through them (a Latin square: every pair of values of any two
# of the three parameters occurs).  Range 100 needs an interval that makes 200 / interval a multiple of 16:
# 0.78125 = 25 / 32 gives M = 256 (interval 1 gives 200, which validate_params refuses); 40 and 64 keep interval 1.
_RANGES = [(40, 1.0), (64, 1.0), (100, 0.78125)]
LAYER_CASES = []
for _i, _L in enumerate((1, 16, 17, 30)):
    for _j, _ltg in enumerate((0.0, 1.5, -1.0)):
        _r, _iv = _RANGES[(_i + _j) % 3]
        LAYER_CASES.append((f"L{_L}_g{_ltg}_R{_r}", dict(n_layers=_L, lidar_to_ground=_ltg, max_range=_r, interval=_iv)))
# the reference sensors' height resolutions x 1.2 at interval 0.7 (the route cases), and the two configurations of the
# other consumers of RasterParams
ROUTE_RES = {"HDL_32E": float(F32(0.5) * F32(1.2)), "HDL_64E": float(F32(0.25) * F32(1.2)), "OS1_64": float(F32(1.0) * F32(1.2))}
ROUTE_CASES = [(f"route_{s}", dict(interval=0.7, height_res=r)) for s, r in ROUTE_RES.items()]
OTHER_CASES = [("other_divide", dict(interval=0.7, height_res=0.3, n_layers=30)), ("other_M272", dict(max_range=136, interval=1.0))]
ALL_CASES = SIZE_CASES + DIVIDE_CASES + LAYER_CASES + ROUTE_CASES + OTHER_CASES


def small_params(**fields) -> bev_amd.BevParams:
    """n_scan 16, horizon_scan 500, ground_upper_scan 10: three column strips, the last of 28 columns; S = 8,000; phase A
    tests rows 15 .. 6 and marks row 5 at most, so rows 0 .. 4 keep their labels"""
    p = bev_amd.params_for_sensor("HDL_32E")
    p.n_scan, p.horizon_scan, p.ground_upper_scan = 16, 500, 10
    return with_fields(p, **fields)


def with_fields(p: bev_amd.BevParams, **fields) -> bev_amd.BevParams:
    q = bev_amd.BevParams()
    for name, _ in bev_amd.BevParams._fields_:
        setattr(q, name, getattr(p, name))
    for k, v in fields.items():
        setattr(q, k, v)
    return q


def mat_size_layout(p) -> dict:
    """the band layout of p's image (tests/hostcheck: csrc/bev_exact.h raster_band_layout)"""
    import hostcheck_lib as hc
    return hc.band_layout(p.mat_size)


def is_pow2(v: float) -> bool:
    m, _ = np.frexp(F32(v))
    return bool(m == 0.5)


# ---- the reference's bin / layer expressions on arrays (finite inputs), and their "approximate" variants ----------
def _round_half_away(d):
    return np.where(d >= 0, np.floor(d + 0.5), -np.floor(-d + 0.5))


def bins_div(c, max_range, interval):
    """BatchMultiBevGen.cpp:279: (p + MAX_RANGE) / interval in float, + 0.5 and round() in double"""
    with np.errstate(all="ignore"):
        sh = ((c.astype(F32) + F32(max_range)) / F32(interval)).astype(F32)
        return _round_half_away(sh.astype(np.float64) + 0.5)


def bins_mul(c, max_range, interval):
    """the same with the division replaced by a multiplication by fl(1 / interval)"""
    with np.errstate(all="ignore"):
        sh = ((c.astype(F32) + F32(max_range)) * (F32(1) / F32(interval))).astype(F32)
        return _round_half_away(sh.astype(np.float64) + 0.5)


def layers_div(z, height_res, ltg):
    """:281: roundf(z / HEIGHT_RES + lidar_to_ground), all float"""
    with np.errstate(all="ignore"):
        return _round_half_away(((z.astype(F32) / F32(height_res)).astype(F32) + F32(ltg)).astype(F32).astype(np.float64))


def layers_mul(z, height_res, ltg):
    with np.errstate(all="ignore"):
        return _round_half_away(((z.astype(F32) * (F32(1) / F32(height_res))).astype(F32) + F32(ltg)).astype(F32).astype(np.float64))


def _with_neighbours(v):
    v = v.astype(F32)
    return np.concatenate([v, np.nextafter(v, F32(np.inf)), np.nextafter(v, F32(-np.inf))]).astype(F32)


def boundary_coords(p) -> np.ndarray:
    """for every image bin k = 0 .. M: fl(k * interval) - max_range and its two float neighbours (x and y alike)"""
    k = np.arange(p.mat_size + 1, dtype=F32)
    return _with_neighbours((k * F32(p.interval)).astype(F32) - F32(p.max_range))


def boundary_heights(p) -> np.ndarray:
    """for every layer edge k = -2 .. n_layers + 2: fl((k + 0.5 - lidar_to_ground) * height_res) and its neighbours; and
    both clamps of the single height, (int)((z + lidar_to_ground) * 4.0) at 0 and at 255, with their neighbours"""
    k = np.arange(-2, p.n_layers + 3, dtype=F32)
    edges = ((k + F32(0.5) - F32(p.lidar_to_ground)) * F32(p.height_res)).astype(F32)
    clamps = np.array([0.0, 0.25, 63.5, 63.75, 64.0, 80.0, -3.0], F32) - F32(p.lidar_to_ground)
    return np.concatenate([_with_neighbours(edges), _with_neighbours(clamps)]).astype(F32)


def _ulp_window(c, w=64):
    """the floats within w ulps of every element of c (c != 0)"""
    u = c[c != 0].astype(F32).view(np.int32).astype(np.int64)
    return (u[:, None] + np.arange(-w, w + 1)[None, :]).astype(np.int32).view(F32).reshape(-1)


def searched_coords(p, cap=96) -> np.ndarray:
    """Coordinates within 64 ulps of an image bin's edge that a multiplication by fl(1 / interval) bins differently than
    the division, at most `cap` of them, spread over the edges.  The edges and their immediate neighbours do not always
    hold one: at interval 0.75, range 72, k * 0.75 and the shift by 72 are exact and one ulp to either side does not
    flip the rounded product, while a few ulps further out it does."""
    if is_pow2(p.interval):
        return np.empty(0, F32)
    k = np.arange(p.mat_size + 1, dtype=F32)
    w = _ulp_window((k * F32(p.interval)).astype(F32) - F32(p.max_range))
    a, b = bins_div(w, p.max_range, p.interval), bins_mul(w, p.max_range, p.interval)
    hit = w[(a != b) & (np.minimum(a, b) >= 0) & (np.maximum(a, b) < p.mat_size)]
    return hit[np.linspace(0, len(hit) - 1, min(cap, len(hit))).astype(int)] if len(hit) else hit


def searched_heights(p, cap=48) -> np.ndarray:
    """the same for the layer edges and fl(1 / height_res)"""
    if is_pow2(p.height_res):
        return np.empty(0, F32)
    k = np.arange(0, p.n_layers + 1, dtype=F32)
    w = _ulp_window(((k + F32(0.5) - F32(p.lidar_to_ground)) * F32(p.height_res)).astype(F32))
    a, b = layers_div(w, p.height_res, p.lidar_to_ground), layers_mul(w, p.height_res, p.lidar_to_ground)
    hit = w[(a != b) & (np.minimum(a, b) >= 0) & (np.maximum(a, b) < p.n_layers)]
    return hit[np.linspace(0, len(hit) - 1, min(cap, len(hit))).astype(int)] if len(hit) else hit


def discriminating(p, x, y, z):
    """(coordinates that bin differently under a multiplication by fl(1 / interval) than under the division, heights that
    layer differently under fl(1 / height_res)), counted over in-image bins / layers of either variant"""
    M, L = p.mat_size, p.n_layers
    nb = 0
    for c in (x, y):
        a, b = bins_div(c, p.max_range, p.interval), bins_mul(c, p.max_range, p.interval)
        nb += int(((a != b) & (((a >= 0) & (a < M)) | ((b >= 0) & (b < M)))).sum())
    a, b = layers_div(z, p.height_res, p.lidar_to_ground), layers_mul(z, p.height_res, p.lidar_to_ground)
    nl = int(((a != b) & (((a >= 0) & (a < L)) | ((b >= 0) & (b < L)))).sum())
    return nb, nl


def boundary_points(p, seed=0) -> np.ndarray:
    """the boundary set as points: every x of the family (and of searched_coords) with a y of it (shuffled) and the heights
    (and searched_heights) in turn"""
    rng = np.random.default_rng(seed)
    bx = np.concatenate([boundary_coords(p), searched_coords(p)])
    bz = np.concatenate([boundary_heights(p), searched_heights(p)])
    n = max(len(bx), len(bz))
    pts = np.zeros(n, POINT_DTYPE)
    pts["x"] = bx[np.arange(n) % len(bx)]
    pts["y"] = rng.permutation(bx)[np.arange(n) % len(bx)]
    pts["z"] = bz[np.arange(n) % len(bz)]
    # the edge bins leave the image on one axis and take the other axis' coordinate with them: those points get a
    # mid-image coordinate on the other axis in turn, so that every boundary coordinate lands in an image once
    mid = F32(0.37) * F32(p.interval)
    out_x = (bins_div(pts["x"], p.max_range, p.interval) < 0) | (bins_div(pts["x"], p.max_range, p.interval) >= p.mat_size)
    extra = pts[out_x].copy()
    extra["x"], extra["y"] = mid, pts["y"][out_x]
    return np.concatenate([pts, extra])


def place_boundary(p, frames, which, bpts) -> int:
    """Overwrites xyz (and sets label -2, a valid intensity) of points of frames[i], i in `which`, with the boundary set:
    only points that win their slot (the last in input order with that (row, col)) in rows phase A never tests
    (row < N - G - 1) are taken, so every placed point survives getOrderedCloud and markGroundPoints.  Returns how many
    points were placed (all of bpts, or the test's frames are too small)."""
    N, H, G = p.n_scan, p.horizon_scan, p.ground_upper_scan
    done = 0
    for i in which:
        f = frames[i]
        ok = (f["row"] < N) & (f["col"] < H) & (f["label"] != 0)   # (not the all-zero records of a structured cloud)
        key = f["row"].astype(np.int64) * H + f["col"]
        last = np.full(N * H, -1, np.int64)
        allp = np.flatnonzero((f["row"] < N) & (f["col"] < H))
        last[key[allp]] = allp                     # (ascending index: the last assignment wins)
        win = last[last >= 0]
        win = win[ok[win]]
        win = win[f["row"][win] < N - G - 1]
        take = win[:len(bpts) - done]
        for c in ("x", "y", "z"):
            f[c][take] = bpts[c][done:done + len(take)]
        f["label"][take] = -2
        f["intensity"][take] = 1.0
        done += len(take)
        if done == len(bpts):
            break
    return done


def scale_xy(p, f, share_outside=0.2):
    """scales x, y so that `share_outside` of the finite points lie beyond the image's edges (on every side: the sweeps
    are centred on the sensor)"""
    r = np.maximum(np.abs(f["x"]), np.abs(f["y"]))
    r = r[np.isfinite(r) & (r > 0) & (r < 1e6)]
    if len(r) == 0:
        return f
    s = F32(p.max_range / np.quantile(r, 1.0 - share_outside))
    with np.errstate(all="ignore"):
        f["x"] = (f["x"] * s).astype(F32)
        f["y"] = (f["y"] * s).astype(F32)
    return f


def small_frames(p, n_frames=9, seed=0):
    """The frames of one call on the small geometry: sweeps (sorted, with appended duplicates: the in-place route and its
    tail), adversarial clouds with non-finite coordinates, an empty and a one-point frame; x / y scaled across the image
    edges; the boundary set placed in the sweeps.  Returns (frames, boundary points placed)."""
    S = p.slots
    frames = [synth.sweep(p, 200 + seed, keep=0.98, n_dup=300).copy(),
              synth.adversarial(p, S, 40 + seed, nonfinite=True).copy(),
              np.empty(0, POINT_DTYPE),
              synth.sweep(p, 201 + seed, keep=0.9, n_dup=0)[77:78].copy(),
              synth.sweep(p, 202 + seed, keep=1.0, n_dup=0).copy(),
              synth.sweep(p, 203 + seed, keep=0.7, n_dup=40).copy(),
              synth.adversarial(p, S // 2, 41 + seed, nonfinite=False).copy(),
              synth.sweep(p, 204 + seed, keep=0.95, n_dup=1000).copy(),
              synth.sweep(p, 205 + seed, keep=1.0, n_dup=0).copy()][:n_frames]
    for f in frames:
        if len(f) > 1:
            scale_xy(p, f)
    bpts = boundary_points(p, seed)
    placed = place_boundary(p, frames, [i for i in (0, 4, 5, 7, 8) if i < len(frames)], bpts)
    assert placed == len(bpts), (placed, len(bpts))
    return frames, bpts


def survivors(ordered):
    """the points of ordered clouds that reach the rasters' tests with finite coordinates"""
    o = np.concatenate([np.asarray(c).reshape(-1) for c in ordered])
    o = o[(o["label"] != 0) & np.isfinite(o["x"]) & np.isfinite(o["y"]) & np.isfinite(o["z"])]
    return o
