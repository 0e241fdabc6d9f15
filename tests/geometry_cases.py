"""The sensor geometries (n_scan, horizon_scan, ground_upper_scan) bev_create admits: the corners of the admitted range,
their refused neighbours and the pair of cases on either side of every eligibility threshold of the in-place routes —
the list shared by tests/test_sensor_geometry_cpu.py (the checker, the closed forms, this table's own arithmetic) and
tests/test_sensor_geometry_gpu.py; the frames they run and what a frame must contain to count.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import bev_amd
from bev_amd import POINT_DTYPE, synth

# ---- the limits, restated from csrc/bev_internal.h (test_sensor_geometry_cpu.py holds the table below against
# bev_multi_bytes, so a constant that moves fails there first) --------------------------------------------------------
STRIP_COLS = 236            # kStripCols
MAX_SLOTS = 1024 * 1024     # kMaxTiles * kTile
MAX_SEGS = 1024             # kMaxSegs >= (G + 1) * strips
MAX_STRIPS = 280            # kMaxStrips
RESOLVE_PARTS = 4           # kResolveParts: emitters = strips + kResolveParts
STREAM_MAX_ROWS = 64        # kStreamMaxRows
TAIL_BUCKETS = 2048         # kTailBuckets >= N * strips
CM_MAX_ROWS = 128           # kCmMaxRows
CM_MAX_STRIPS = 16          # kCmMaxStrips
MAX_SAMPLES = 4096          # kMaxSamples == kCmMaxSamples
STREAM_MIN_PREFIX = 2048    # kStreamMinPrefix
TAIL_MAX = 16384            # kTailMax
TAIL_CAP = 64               # kTailCap
STRIDE, STRIDE_DENSE, STRIDE_PRIME = 63, 127, 61   # kProbeStride, kProbeStrideDense, the stride of S-record frames when 3 | N or 7 | N
GENERAL, STREAM, REDO, STRUCTURED, COLMAJOR, COLMAJOR_GEN = 0, 1, 2, 3, 4, 5
NOT_ELIGIBLE, SHORT_PREFIX, LONG_TAIL, LIST_OVERFLOW = 1, 2, 3, 4   # `consumed` of a frame that went general (k_probe)
BEV_ERR_INVALID_ARG, BEV_ERR_UNSUPPORTED = -1, -5   # include/bev_mi355x.h


def strips(h: int) -> int:
    return (h + STRIP_COLS - 1) // STRIP_COLS


def segs(h: int, g: int) -> int:
    return (g + 1) * strips(h)


def status(n: int, h: int, g: int) -> int:
    """validate_params' answer for the geometry, by this table's arithmetic: 0, BEV_ERR_INVALID_ARG, BEV_ERR_UNSUPPORTED"""
    if n < 3 or n > 65535 or h < 5 or h > 65535 or g < 1 or g > n - 2:
        return BEV_ERR_INVALID_ARG
    if n * h > MAX_SLOTS or segs(h, g) > MAX_SEGS:
        return BEV_ERR_UNSUPPORTED
    return 0


# (name, (N, H, G), what it pins)
ADMITTED = [
    ("square_max", (1024, 1024, 203), "S == 2^20, tiles == kMaxTiles; 5 strips, the last of 80 columns; 1020 segments"),
    ("tall_max", (65535, 16, 1023), "largest row index 65534; one strip; exactly 1024 segments; S = 1,048,560"),
    ("wide_max", (16, 65535, 2), "largest column index 65534; 278 strips (282 emitters), the last of 163 columns; 834 segments"),
    ("wide_3rows", (3, 65535, 1), "smallest N with the most strips"),
    ("segs_one_strip", (1026, 236, 1023), "H == kStripCols; 1024 segments; G == N - 3"),
    ("segs_four_strips", (257, 944, 255), "H == 4 * kStripCols; 1024 segments; first row count above 255"),
    ("tiny", (3, 5, 1), "smallest admitted sensor"),
]
ADMITTED_BY_NAME = {name: nhg for name, nhg, _ in ADMITTED}
# what the table says about itself: (S, strips, segments)
ADMITTED_ARITHMETIC = {
    "square_max": (1 << 20, 5, 1020), "tall_max": (1048560, 1, 1024), "wide_max": (1048560, 278, 834),
    "wide_3rows": (196605, 278, 556), "segs_one_strip": (242136, 1, 1024), "segs_four_strips": (242608, 4, 1024),
    "tiny": (15, 1, 2),
}
LARGE = ("square_max", "tall_max", "wide_max")           # S ~ 2^20: the per-function entry points run here
REFUSED_UNSUPPORTED = [(1025, 1024, 10), (65535, 17, 10), (1024, 1024, 204), (65535, 16, 1024), (16, 65535, 3),
                       (1026, 237, 1023), (257, 945, 255)]
REFUSED_INVALID = [(65536, 16, 10), (2, 1024, 1), (16, 65536, 2), (16, 4, 2), (64, 1024, 0), (64, 1024, 63)]
REFUSED = [(nhg, BEV_ERR_UNSUPPORTED) for nhg in REFUSED_UNSUPPORTED] + [(nhg, BEV_ERR_INVALID_ARG) for nhg in REFUSED_INVALID]


def params(n: int, h: int, g: int) -> bev_amd.BevParams:
    """the reference's raster (interval 1, range 112, 24 layers: what oracle_lib.process_frame computes) on an (N, H, G) sensor"""
    p = bev_amd.params_for_sensor("HDL_32E")
    p.n_scan, p.horizon_scan, p.ground_upper_scan = n, h, g
    return p


def case_params(name: str) -> bev_amd.BevParams:
    return params(*ADMITTED_BY_NAME[name])


def probe_samples(n_pts: int, n: int, h: int) -> int:
    """how many samples k_probe takes of a frame of n_pts points (bev_front.h)"""
    S = n * h
    stride = STRIDE_DENSE if (n_pts != S and n_pts >= S - S // 10) else (STRIDE_PRIME if (n_pts == S and (n % 3 == 0 or n % 7 == 0)) else STRIDE)
    return (n_pts - 1) // stride + 1 if n_pts else 0


def stream_eligible(n: int, h: int) -> bool:
    """sorted sweeps of the geometry can be read in place (mode 1): the stream walk's per-row estimates and k_probe's
    tail counters fit"""
    return n <= STREAM_MAX_ROWS and n * strips(h) <= TAIL_BUCKETS


def cm_gen_eligible(n: int, h: int) -> bool:
    """real firing-order sweeps of the geometry have their route (mode 5)"""
    return n <= CM_MAX_ROWS and strips(h) <= CM_MAX_STRIPS and probe_samples(n * h, n, h) <= MAX_SAMPLES


def context_bytes(p, max_batch: int, max_points: int, want_gm: bool = True) -> int:
    """device bytes of a context after a process_batch call, from bev_create's and ensure_staging's allocations (the
    per-lane workspace of the 8 lanes, the single-cloud code buffer, the staging)"""
    import hostcheck_lib as hc
    n, h, g, S, nb = p.n_scan, p.horizon_scan, p.ground_upper_scan, p.slots, max_batch
    st, sg, bands = strips(h), segs(h, g), hc.band_layout(p.mat_size)["bands"]
    worst = max(n * STRIP_COLS, ((sg + RESOLVE_PARTS - 1) // RESOLVE_PARTS + 1) * 256)
    stride = (((min(worst, 4096) + 63) // 64) | 1) * 64
    lane = nb * 32 + nb * n * st * 4 + nb * S * 4 + (nb * sg + 1) * 256 * 8 + nb * sg * 4
    lane += nb * (st + RESOLVE_PARTS) * bands * (stride + 1) * 4 + nb * 3750 * 4
    if stream_eligible(n, h):
        lane += nb * n * st * (TAIL_CAP + 1) * 4
    if n <= CM_MAX_ROWS and st <= CM_MAX_STRIPS:
        lane += nb * ((4 + CM_MAX_ROWS) + (CM_MAX_ROWS // 2) * CM_MAX_STRIPS * 2 + 3 * CM_MAX_ROWS) * 4
    if want_gm:
        lane += nb * S
    M, L = p.mat_size, p.n_layers
    staging = max(max_points, S) * nb * 32 + nb * S * 32 + nb * (L + 1) * M * M + nb * S
    return 8 * lane + max(max_points, S, 1 << 20) * 4 + staging


# ---- frames -----------------------------------------------------------------------------------------------------------
def plant_ground(p, f):
    """Overwrites a handful of records of f (coordinates and intensity only, never row / col: a frame keeps its layout) so
    that the frame has, whatever the sensor: two columns of flat ground in rows N - 1 and N - 2 (ground_mat 1, label 0), one
    column of a flat platform 0.7 m higher in the neighbouring 2 m ground cell (candidates of phase A that phase C puts
    back), one column with an invalid lower return (ground_mat -1).  The records are the last of their slot nearest to the
    middle column; all-zero records (a structured cloud's dropped returns, a real sweep's no-return records) are skipped."""
    N, H = p.n_scan, p.horizon_scan
    real = (f["row"] < N) & (f["col"] < H) & ((f["x"] != 0) | (f["y"] != 0) | (f["z"] != 0))
    idx = np.flatnonzero(real & (f["row"] >= N - 2))
    slot = f["row"][idx].astype(np.int64) * H + f["col"][idx]
    have = set(slot.tolist())
    cols = [c % H for c in range(H // 2, H // 2 + H)]
    found = [c for c in cols if (N - 1) * H + c in have and (N - 2) * H + c in have][:4]
    if len(found) < 3:
        return f
    roles = [(-1.7, 3.0, False), (-1.0, 5.0, False), (-1.7, 3.4, True), (-1.7, 3.2, False)]   # (z, x of the upper row, lower return invalid)
    for c, (z, x, invalid) in zip(found, roles):
        for r, dx in ((N - 2, 0.0), (N - 1, 0.5)):
            i = idx[slot == r * H + c]                   # (every record that claims the slot: whichever wins it)
            f["x"][i], f["y"][i], f["z"][i] = np.float32(x + dx), np.float32(0.5), np.float32(z)
            f["intensity"][i] = -1.0 if (invalid and r == N - 1) else 0.5
            f["label"][i] = np.where(f["label"][i] == 0, -2, f["label"][i])
    return f


def boundaries(h: int, about: int = 20):
    """the first, the last and about `about` of the strip boundaries between them (first columns of strips 1 ..)"""
    b = np.arange(1, strips(h)) * STRIP_COLS
    if len(b) > about + 2:
        b = np.unique(np.concatenate([b[:1], b[-1:], b[np.linspace(1, len(b) - 2, about).astype(int)]]))
    return b


def place_invalid(p, f, seed=0):
    """intensity -1 (phase A's (c + 2) % H, flat c - 2 and row - 2 fallbacks are taken, BatchMultiBevGen.cpp:146-160, and read
    the strips' halo columns) at: the first and last two columns of the rows around N - G and of the two bottom rows; two
    columns either side of the sampled strip boundaries in those rows; a seventh of the last strip's records in the ground rows"""
    N, H, G = p.n_scan, p.horizon_scan, p.ground_upper_scan
    rng = np.random.default_rng(seed)
    rows = np.array(sorted({r for r in list(range(N - G - 2, N - G + 2)) + [N - 2, N - 1] if 0 <= r < N}))
    cols = {0, 1, H - 2, H - 1}
    for b in boundaries(H).tolist():
        cols |= {b - 2, b - 1, b, b + 1}
    cols = np.array(sorted(c for c in cols if 0 <= c < H))
    real = (f["x"] != 0) | (f["y"] != 0) | (f["z"] != 0)
    m = np.isin(f["row"], rows) & np.isin(f["col"], cols) & real
    last0 = (strips(H) - 1) * STRIP_COLS
    m |= (f["col"] >= last0) & (f["col"] < H) & (f["row"] >= N - G - 1) & (f["row"] < N) & real & (rng.random(len(f)) < 1.0 / 7.0)
    f["intensity"][m] = -1.0
    return f


def out_of_range_records(p, seed=0):
    """records whose row or column is just past the sensor (row == N, col == H) or 65535, with finite coordinates inside the
    image: getOrderedCloud drops them (BatchMultiBevGen.cpp:106-111); a few in-range duplicates of one slot among them"""
    N, H = p.n_scan, p.horizon_scan
    rc = [(N, 0), (N, H - 1), (0, H), (N - 1, H), (N, H), (65535, 0), (0, 65535), (65535, 65535), (N - 1, 65535), (65535, H - 1),
          (N - 1, H - 1), (N - 1, H - 1), (0, 0)]
    f = np.zeros(len(rc), POINT_DTYPE)
    rng = np.random.default_rng(seed)
    f["x"], f["y"] = rng.uniform(-30, 30, len(rc)), rng.uniform(-30, 30, len(rc))
    f["z"], f["intensity"], f["label"] = rng.uniform(-1, 2, len(rc)), 0.5, -2
    f["row"] = np.array([r & 0xffff for r, _ in rc], np.uint16)
    f["col"] = np.array([c & 0xffff for _, c in rc], np.uint16)
    f["t"] = np.arange(len(rc))
    return f


def nonfinite_records(p, seed=0):
    """in-range records with a NaN, an infinity or a huge value in one coordinate, in the two bottom rows (phase A's angle
    test sees them) and in row 0"""
    N, H = p.n_scan, p.horizon_scan
    vals = [("x", np.nan), ("y", np.inf), ("z", -np.inf), ("z", 3.0e38), ("x", -3.0e38), ("z", np.nan)]
    f = np.zeros(len(vals), POINT_DTYPE)
    f["x"], f["y"], f["z"], f["intensity"], f["label"] = 4.0, 1.0, -1.7, 0.5, -2
    for i, (c, v) in enumerate(vals):
        f[c][i] = v
    f["row"] = [N - 1, N - 2, N - 1, 0, N - 2, 0]
    f["col"] = [(seed + 1 + 2 * i) % H for i in range(len(vals))]
    f["t"] = 100 + np.arange(len(vals))
    return f


def sweep_with_tail(p, fid, keep=0.97, n_dup=1000):
    return plant_ground(p, place_invalid(p, synth.sweep(p, fid, keep=keep, n_dup=n_dup).copy(), fid))


def structured(p, fid, keep=0.95):
    return plant_ground(p, place_invalid(p, synth.structured(p, fid, keep).copy(), fid))


def firing_order(p, fid):
    return plant_ground(p, place_invalid(p, synth.firing_order(p, fid).copy(), fid))


def firing_real(p, fid, **kw):
    """(no-return records, 3 % by default, land in column 0 of their row)"""
    return plant_ground(p, place_invalid(p, synth.firing_real(p, fid, **kw).copy(), fid))


def adversarial(p, seed):
    """synth.adversarial (non-finite values, duplicates, rows up to N + 2, columns up to H + 4, row 65535) with the
    out-of-range and the non-finite records above spliced in at the start, in the middle and at the end"""
    a = synth.adversarial(p, min(max(p.slots // 2, 64), 150000), seed, nonfinite=True).copy()
    o = out_of_range_records(p, seed)
    return np.concatenate([o, a[:len(a) // 2], nonfinite_records(p, seed), o, a[len(a) // 2:], o])


def corner_frames(name: str):
    """The six frames an admitted corner runs in one call, with the mode each must end in (None: not asserted) and, for a
    frame that goes general, k_probe's reason.  Ordered so that the two frames of a sub-batch of a max_batch 4 context
    (process_batch cuts a call into chunks of max_batch / 2) differ in layout."""
    n, h, g = ADMITTED_BY_NAME[name]
    p = params(n, h, g)
    if name == "tiny":
        # 15 slots: a sweep with a tail of 4, real firing order without stagger (H = 5 has no room for +-9 columns); the
        # first frame ids whose frames have the content `covered` asks for
        makers = [lambda fid: sweep_with_tail(p, fid, keep=1.0, n_dup=4), lambda fid: structured(p, fid, 1.0), lambda fid: firing_order(p, fid),
                  lambda fid: firing_real(p, fid, phase=2, direction=-1, stagger=0.0, noret=0.0)]
        frames = [next(f for f in (make(fid) for fid in range(11, 400)) if covered(p, f)) for make in makers]
    else:
        frames = [sweep_with_tail(p, 11), structured(p, 12), firing_order(p, 13), firing_real(p, 14)]
    frames += [adversarial(p, 15), np.empty(0, POINT_DTYPE)]
    sw = frames[0]
    can_stream = stream_eligible(n, h) and len(sw) >= STREAM_MIN_PREFIX and probe_samples(len(sw), n, h) <= MAX_SAMPLES
    expect = [(STREAM, None) if can_stream else (GENERAL, NOT_ELIGIBLE), (STRUCTURED, None), (COLMAJOR, None),
              (None, None), (None, None), (GENERAL, NOT_ELIGIBLE)]
    # (the real sweep: no corner has a route for it — more than kCmMaxRows rows or kCmMaxStrips strips — but `tiny`, where
    # k_probe cannot tell it from the plain sweep: with 5 columns every in-range column is within kPlainDisp = 8 of its
    # firing, the frame is handed to the plain walk and ends in mode 4 or, caught, in mode 2.  Route 5 at its own limits:
    # the kCmMaxRows / kCmMaxStrips pairs below.)
    assert not cm_gen_eligible(n, h) or name == "tiny"
    return p, frames, expect


def unsampled(i: int) -> int:
    """the next position k_probe looks at under none of its strides (every 61st, 63rd or 127th record and its successor)"""
    while any(i % s in (0, 1) for s in (STRIDE, STRIDE_DENSE, STRIDE_PRIME)):
        i += 1
    return i


def hidden_defects(p, frames, expect):
    """One defect per in-place route that ran, at a position the probe does not sample, in the style of test_gpu_stream.py,
    test_gpu_structured.py and test_gpu_colmajor.py: two neighbouring prefix points swapped (sorted sweep), a record that
    claims a column seven further on (structured), a wrong beam (firing order, plain and real).  Returns (frames, the route
    each was made from); every one must be caught by the walk and redone: mode 2."""
    N, H, S = p.n_scan, p.horizon_scan, p.slots
    out, routes = [], []
    for f, (mode, _) in zip(frames, expect):
        if mode not in (STREAM, STRUCTURED, COLMAJOR, COLMAJOR_GEN) or len(f) < 8:
            continue
        d = f.copy()
        i = min(unsampled(len(f) // 3), len(f) - 2)
        if mode == STREAM:
            assert int(d["row"][i]) * H + int(d["col"][i]) < int(d["row"][i + 1]) * H + int(d["col"][i + 1])   # (inside the sorted prefix)
            d[[i, i + 1]] = d[[i + 1, i]]
        elif mode == STRUCTURED:
            while not d["label"][i]:      # (a real point, not a dropped return)
                i = unsampled(i + 1)
            d["col"][i] = (int(d["col"][i]) + 7) % H
        else:
            while d["col"][i] == 0 or d["col"][i] >= H:   # (not a no-return record)
                i = unsampled(i + 1)
            d["row"][i] = (int(d["row"][i]) + 1) % N
        out.append(d)
        routes.append(mode)
    return out, routes


# ---- the threshold pairs: (name, (N, H, G), frames(p) -> [(frame, mode, reason)]) ---------------------------------------
def _cut(f, n):
    """f thinned evenly to n records (a sorted frame stays sorted)"""
    assert len(f) >= n
    return np.ascontiguousarray(f[(np.arange(n, dtype=np.int64) * len(f)) // n])


def _sorted_plus_tail(p, fid, keep, tail_rc):
    """a sorted sweep (every slot with probability `keep`) followed by tail records at the given (row, col)s: copies of the
    full sweep's points of those slots, 5 cm higher; the first tail record lies below the prefix's last slot"""
    H = p.horizon_scan
    full = synth.sweep(p, fid, keep=1.0, n_dup=0)
    assert len(full) == p.slots
    rng = np.random.default_rng(fid)
    prefix = full[rng.random(len(full)) < keep]
    tail = full[np.asarray([r * H + c for r, c in tail_rc], np.int64)].copy()
    tail["z"] += np.float32(0.05)
    tail["t"] = 7
    return plant_ground(p, np.concatenate([prefix, tail]))


def _stream_rows(p):
    return [(sweep_with_tail(p, 21, keep=0.85, n_dup=300), *((STREAM, None) if p.n_scan <= STREAM_MAX_ROWS else (GENERAL, NOT_ELIGIBLE)))]


def _tail_buckets(p):
    inside = p.n_scan * strips(p.horizon_scan) <= TAIL_BUCKETS
    return [(sweep_with_tail(p, 22, keep=0.95, n_dup=500), *((STREAM, None) if inside else (GENERAL, NOT_ELIGIBLE)))]


def _real_sweep(p, fid, **kw):
    """a real sweep with no-return records in column 0, a tenth of its inner returns invalid and none at the row ends: a wrap-around halo that falls
    back on column 0 (BatchMultiBevGen.cpp:146-149) may take another record than strip 0 put there, and k_verdict then has the
    frame redone (tests/test_gpu_colmajor.py) — right, but not the route these cases are about"""
    f = synth.firing_real(p, fid, **kw).copy()
    rng = np.random.default_rng(fid)
    inner = (f["col"] >= 4) & (f["col"] < p.horizon_scan - 4)      # (their fallbacks stay away from columns 0 and 1)
    f["intensity"][inner & (rng.random(len(f)) < 0.1)] = -1.0
    return plant_ground(p, f)


def _wrong_beam(p, f):
    d = f.copy()
    i = unsampled(len(f) // 3)
    while d["col"][i] == 0 or d["col"][i] >= p.horizon_scan:
        i = unsampled(i + 1)
    d["row"][i] = (int(d["row"][i]) + 1) % p.n_scan
    return d


def _cm_frames(p, fid, inside, outside_reason):
    a, b = _real_sweep(p, fid), _real_sweep(p, fid + 1, noret=0.2, direction=-1)
    route = (COLMAJOR_GEN, None) if inside else (GENERAL, outside_reason)
    rows = [(a, *route), (b, *route), (firing_order(p, fid + 2), COLMAJOR, None)]
    if inside:      # the route ran: a wrong beam hidden from the probe's samples must end in mode 2
        rows.append((_wrong_beam(p, a), REDO, None))
    return rows


def _cm_rows(p):
    # (more than kStreamMaxRows rows: a frame without a route of its own is not eligible for the sorted one either)
    return _cm_frames(p, 23, p.n_scan <= CM_MAX_ROWS, NOT_ELIGIBLE)


def _cm_strips(p):
    # (64 rows, N * strips <= kTailBuckets: the sorted route looks at the frame and finds a prefix of one firing)
    return _cm_frames(p, 26, strips(p.horizon_scan) <= CM_MAX_STRIPS, SHORT_PREFIX)


def _max_samples(p):
    """a sorted sweep with a tail of 200, cut to exactly 258,048 records (4096 samples at stride 63) and to 258,049 (4097)"""
    n_in = (MAX_SAMPLES - 1) * STRIDE + STRIDE    # 258,048: the most records with 4096 samples
    assert n_in < p.slots - p.slots // 10         # (the stride stays 63)
    sw = synth.sweep(p, 29, keep=0.9, n_dup=0)
    tail = synth.sweep(p, 30, keep=0.5, n_dup=0)[::700][:200]      # spread over the rows: one or two per (row, strip)
    out = []
    for n, mode, reason in ((n_in, STREAM, None), (n_in + 1, GENERAL, NOT_ELIGIBLE)):
        f = plant_ground(p, np.concatenate([_cut(sw, n - len(tail)), tail]))
        assert len(tail) == 200 and len(f) == n and probe_samples(n, p.n_scan, p.horizon_scan) == (MAX_SAMPLES if mode == STREAM else MAX_SAMPLES + 1)
        out.append((f, mode, reason))
    return out


def _min_prefix(p):
    sw = synth.sweep(p, 31, keep=1.0, n_dup=0)
    late = synth.sweep(p, 32, keep=1.0, n_dup=0)[p.slots - 4000:]      # the bottom rows: ground content
    short = np.concatenate([late[:STREAM_MIN_PREFIX - 1], sw[:300]])   # sorted up to record 2046, then a lower slot
    return [(late[:STREAM_MIN_PREFIX - 1].copy(), GENERAL, NOT_ELIGIBLE), (late[:STREAM_MIN_PREFIX].copy(), STREAM, None),
            (short, GENERAL, SHORT_PREFIX)]


def _tail_max(p):
    """tails of 16384 and 16385 records dealt round robin to the (row, strip) pairs, at columns that are in no neighbour's
    halo: 29 records per pair at most"""
    N, H = p.n_scan, p.horizon_scan
    st = strips(H)
    width = min(STRIP_COLS, H - (st - 1) * STRIP_COLS) - 4     # the last strip's own columns, without two at either edge
    out = []
    for n_tail, mode, reason in ((TAIL_MAX, STREAM, None), (TAIL_MAX + 1, GENERAL, LONG_TAIL)):
        j = np.arange(n_tail)
        b, k = j % (N * st), j // (N * st)
        rc = list(zip((b // st).tolist(), ((b % st) * STRIP_COLS + 2 + (k * 5) % width).tolist()))
        assert k.max() + 1 <= TAIL_CAP
        out.append((_sorted_plus_tail(p, 33, 0.9, rc), mode, reason))
    return out


def _tail_cap(p):
    """64 and 65 tail records in (row N - 3, strip 3), two per column (the later one wins its slot), none in a halo"""
    out = []
    for n_tail, mode, reason in ((TAIL_CAP, STREAM, None), (TAIL_CAP + 1, GENERAL, LIST_OVERFLOW)):
        rc = [(p.n_scan - 3, 3 * STRIP_COLS + 2 + (k // 2) * 3) for k in range(n_tail)]
        out.append((_sorted_plus_tail(p, 34, 0.9, rc), mode, reason))
    return out


THRESHOLDS = [
    ("stream_rows_in", (64, 1024, 40), _stream_rows), ("stream_rows_out", (65, 1024, 40), _stream_rows),
    ("tail_buckets_in", (64, 7552, 30), _tail_buckets), ("tail_buckets_out", (64, 7553, 30), _tail_buckets),
    ("cm_rows_in", (128, 1024, 100), _cm_rows), ("cm_rows_out", (129, 1024, 100), _cm_rows),
    ("cm_strips_in", (64, 3776, 30), _cm_strips), ("cm_strips_out", (64, 3777, 30), _cm_strips),
    ("max_samples", (64, 4800, 30), _max_samples),
    ("min_prefix", (32, 1056, 20), _min_prefix),
    ("tail_max", (64, 2083, 50), _tail_max),
    ("tail_cap", (64, 2083, 50), _tail_cap),
]


def coverage(p, pts, want):
    """what a frame exercises, from the oracle's outputs `want` (oracle_lib.process_frame) and the closed forms' phase A:
    ground slots, slots phase A could not judge, points labelled 0 by the marking, candidates phase C put back"""
    import hostcheck_lib as hc
    o_ord, o_gm = want[0], want[1]
    _, gm_a = hc.phase_a_ground_mat(p, pts)
    return dict(ground=int((o_gm == 1).sum()), unknown=int((o_gm == -1).sum()),
                label0=int(((o_ord["label"] == 0) & (o_gm.reshape(-1) == 1)).sum()),
                put_back=int(((gm_a == 1) & (o_gm == 0)).sum()))


def covered(p, pts, want=None) -> bool:
    """the frame has ground slots, slots phase A could not judge, points the marking labelled 0 and a candidate that phase
    C put back"""
    import oracle_lib as orc
    c = coverage(p, pts, want if want is not None else orc.process_frame(orc.sensor_from_params(p), pts))
    return min(c.values()) > 0
