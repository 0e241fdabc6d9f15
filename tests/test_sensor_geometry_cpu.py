"""CPU: the sensor geometries bev_create admits (tests/geometry_cases.py).
  - the table of admitted corners and refused neighbours equals validate_params (bev_multi_bytes zero or not) and its own
    arithmetic (slots, strips, segments; which threshold pair sits on which side of which constant);
  - the closed forms the kernels evaluate (tests/hostcheck, csrc/bev_exact.h) equal the checker byte for byte at every
    admitted corner, on one frame of each layout;
  - the checker equals the Python restatement at the corners small enough for pure-Python loops."""
import ctypes as C

import numpy as np
import pytest

import bev_amd
import geometry_cases as gc
import hostcheck_lib as hc
import oracle_lib as orc
import py_restatement as py

CORNERS = [name for name, _, _ in gc.ADMITTED]
# the restatement loops over every slot in Python (some 15 s per 2^18 slots): the corners of about 2^20 slots are left out
PY_LEFT_OUT = ("square_max", "tall_max", "wide_max")
PY_CORNERS = [name for name in CORNERS if gc.case_params(name).slots <= 1 << 18]


def _multi_bytes(n, h, g):
    p = gc.params(1, 1, 1)
    p.n_scan, p.horizon_scan, p.ground_upper_scan = n, h, g    # (c_int32: 65536 is representable)
    return int(bev_amd.load_lib().bev_multi_bytes(C.byref(p)))


def test_admission_table():
    for name, (n, h, g), _ in gc.ADMITTED:
        assert gc.status(n, h, g) == 0, name
        assert _multi_bytes(n, h, g) == 24 * 224 * 224, name
        assert (n * h, gc.strips(h), gc.segs(h, g)) == gc.ADMITTED_ARITHMETIC[name], name
    for (n, h, g), want in gc.REFUSED:
        assert gc.status(n, h, g) == want, (n, h, g)
        assert _multi_bytes(n, h, g) == 0, (n, h, g)
    for _, (n, h, g), _ in gc.THRESHOLDS:
        assert gc.status(n, h, g) == 0 and _multi_bytes(n, h, g) != 0, (n, h, g)
    # every refused neighbour differs from an admitted corner in one field by one, or names the field's own limit
    assert [gc.status(*c) for c in gc.REFUSED_UNSUPPORTED] == [gc.BEV_ERR_UNSUPPORTED] * 7
    assert {c[0] for c in gc.REFUSED_INVALID} >= {65536, 2} and {c[1] for c in gc.REFUSED_INVALID} >= {65536, 4}
    assert (64, 1024, 0) in gc.REFUSED_INVALID and (64, 1024, 63) in gc.REFUSED_INVALID     # G of 0 and N - 1


def test_what_the_corners_pin():
    A = gc.ADMITTED_BY_NAME
    n, h, g = A["square_max"]
    assert n * h == gc.MAX_SLOTS and h - (gc.strips(h) - 1) * gc.STRIP_COLS == 80
    n, h, g = A["tall_max"]
    assert n == 65535 and gc.strips(h) == 1 and gc.segs(h, g) == gc.MAX_SEGS
    n, h, g = A["wide_max"]
    assert h == 65535 and gc.strips(h) == 278 <= gc.MAX_STRIPS and gc.strips(h) + gc.RESOLVE_PARTS == 282
    assert h - 277 * gc.STRIP_COLS == 163 and len(gc.boundaries(h)) >= 20
    assert A["wide_3rows"][0] == 3 and gc.strips(A["wide_3rows"][1]) == 278
    n, h, g = A["segs_one_strip"]
    assert h == gc.STRIP_COLS and gc.segs(h, g) == gc.MAX_SEGS and g == n - 3
    n, h, g = A["segs_four_strips"]
    assert h == 4 * gc.STRIP_COLS and gc.segs(h, g) == gc.MAX_SEGS and n == 257
    assert A["tiny"] == (3, 5, 1)


def test_what_the_threshold_pairs_straddle():
    T = {name: nhg for name, nhg, _ in gc.THRESHOLDS}
    assert T["stream_rows_in"][0] == gc.STREAM_MAX_ROWS and T["stream_rows_out"][0] == gc.STREAM_MAX_ROWS + 1
    n, h, _ = T["tail_buckets_in"]
    assert n * gc.strips(h) == gc.TAIL_BUCKETS and n <= gc.STREAM_MAX_ROWS
    n, h, _ = T["tail_buckets_out"]
    assert n * gc.strips(h) == gc.TAIL_BUCKETS + n and h == T["tail_buckets_in"][1] + 1
    assert T["cm_rows_in"][0] == gc.CM_MAX_ROWS and T["cm_rows_out"][0] == gc.CM_MAX_ROWS + 1
    assert gc.cm_gen_eligible(*T["cm_rows_in"][:2]) and not gc.cm_gen_eligible(*T["cm_rows_out"][:2])
    assert gc.strips(T["cm_strips_in"][1]) == gc.CM_MAX_STRIPS and gc.strips(T["cm_strips_out"][1]) == gc.CM_MAX_STRIPS + 1
    assert gc.cm_gen_eligible(*T["cm_strips_in"][:2]) and T["cm_strips_out"][1] == T["cm_strips_in"][1] + 1
    # (the frames of exactly S records of both kCmMaxStrips cases stay within kCmMaxSamples: the strips decide)
    assert gc.probe_samples(64 * 3777, 64, 3777) <= gc.MAX_SAMPLES
    n, h, _ = T["max_samples"]
    assert gc.stream_eligible(n, h)
    assert gc.probe_samples(258048, n, h) == gc.MAX_SAMPLES and gc.probe_samples(258049, n, h) == gc.MAX_SAMPLES + 1
    # kMaxSamples under the DENSE stride (frames of 0.9 S points or more, every 127th sampled) cannot be reached: 4097
    # samples need more than 4096 * 127 = 520,192 points; a geometry whose sorted sweeps are read in place has N * strips
    # <= kTailBuckets (2048), hence at most 2048 * 236 = 483,328 slots — a strictly ascending prefix is no longer than that
    # — plus a tail of kTailMax (16,384): 499,712 points at the most.  The pair above (stride 63) is the test of the cap.
    assert gc.TAIL_BUCKETS * gc.STRIP_COLS + gc.TAIL_MAX == 499712 < gc.MAX_SAMPLES * gc.STRIDE_DENSE == 520192
    assert T["min_prefix"] == (32, 1056, 20) and T["tail_max"] == (64, 2083, 50) == T["tail_cap"]


@pytest.mark.parametrize("name", CORNERS)
def test_closed_forms_equal_the_checker_at_every_corner(name):
    """sweep with a tail, structured, firing order (plain and real), adversarial with non-finite values and out-of-range rows
    and columns, empty"""
    p, frames, _ = gc.corner_frames(name)
    sp = orc.sensor_from_params(p)
    for i, f in enumerate(frames):
        o_ord, o_gm, o_multi, o_single = orc.process_frame(sp, f)
        _, _, o_avg = orc.mark_ground(sp, orc.order_cloud(sp, f))
        h_ord, h_gm, h_avg, h_multi, h_single = hc.process_frame(p, f)
        assert h_ord.tobytes() == o_ord.tobytes(), (name, i, "ordered cloud / labels")
        assert np.array_equal(h_gm, o_gm), (name, i, "ground_mat")
        assert h_avg.tobytes() == o_avg.tobytes(), (name, i, "cell averages")
        assert np.array_equal(h_multi, o_multi) and np.array_equal(h_single, o_single), (name, i, "BEVs")
        if i < 4:       # the four sweeps: every state of the ground marking
            assert gc.covered(p, f, (o_ord, o_gm)), (name, i, gc.coverage(p, f, (o_ord, o_gm)))
    adv = frames[4]     # the adversarial frame holds what it says
    N, H = p.n_scan, p.horizon_scan
    assert (adv["row"] == N).any() and (adv["col"] == H).any() and (adv["row"] == 65535).any() and (adv["col"] == 65535).any()
    assert not np.isfinite(adv["x"]).all() and not np.isfinite(adv["z"]).all()
    assert ((adv["row"] == N - 1) & (adv["col"] == H - 1)).sum() >= 2
    assert (adv["intensity"] == -1).any()


def test_invalid_returns_sit_where_the_halos_are_read():
    for name in ("square_max", "wide_max"):
        p = gc.case_params(name)
        N, H, G = p.n_scan, p.horizon_scan, p.ground_upper_scan
        f = gc.sweep_with_tail(p, 11)
        bad = f[f["intensity"] == -1]
        rows_cols = set(zip(bad["row"].tolist(), bad["col"].tolist()))
        for r in range(max(0, N - G - 2), N - G + 2):
            hit = [c for c in (0, 1, H - 2, H - 1) if (r, c) in rows_cols]
            assert len(hit) >= 3, (name, r, hit)            # (a sweep drops 3 % of its returns)
        for b in gc.boundaries(H).tolist():
            assert sum((r, c) in rows_cols for r in (N - 2, N - 1) for c in (b - 2, b - 1, b, b + 1)) >= 5, (name, b)
        last0 = (gc.strips(H) - 1) * gc.STRIP_COLS
        in_last = bad[(bad["col"] >= last0) & (bad["row"] >= N - G - 1)]
        # spread over the last strip's 80 / 163 columns (wide_max has three ground rows, a seventh of their records invalid:
        # 1 - (6 / 7)^3 = 37 % of the columns are expected)
        assert len(np.unique(in_last["col"])) >= (H - last0) // 4, name


def test_the_restatement_leaves_out_the_largest_corners_only():
    assert sorted(PY_CORNERS + list(PY_LEFT_OUT)) == sorted(CORNERS) and len(PY_LEFT_OUT) <= 4
    assert all(gc.case_params(name).slots > 1 << 18 for name in PY_LEFT_OUT)


@pytest.mark.parametrize("name", PY_CORNERS)
def test_checker_equals_python_restatement(name):
    p = gc.case_params(name)
    if name == "tiny":
        f = gc.corner_frames(name)[1][0]
    else:
        f = gc.sweep_with_tail(p, 11)
    f = np.concatenate([f, gc.out_of_range_records(p, 3)])
    sp = orc.sensor_from_params(p)
    o_ord, o_gm, o_multi, o_single = orc.process_frame(sp, f)
    _, _, o_avg = orc.mark_ground(sp, orc.order_cloud(sp, f))
    p_ord, p_gm, p_avg, p_multi, p_single = py.process_frame(p.n_scan, p.horizon_scan, p.ground_upper_scan, p.height_res, f)
    assert o_ord.tobytes() == p_ord.tobytes(), "ordered cloud / labels"
    assert np.array_equal(o_gm, p_gm), "ground_mat"
    assert np.array_equal(np.asarray(o_avg).reshape(75, 50), p_avg, equal_nan=True), "cell averages"
    assert np.array_equal(o_multi, p_multi) and np.array_equal(o_single, p_single), "BEVs"
