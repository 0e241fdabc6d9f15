"""GPU: ordering, ground marking and the rasters over the sensor geometries bev_create admits (tests/geometry_cases.py):
the corners of the admitted range (2^20 slots, 1024 segments, 278 strips, row and column indices up to 65534), the refused
neighbour of each, and the case just inside and just outside every eligibility threshold of the in-place routes
(kStreamMaxRows, kTailBuckets, kCmMaxRows, kCmMaxStrips, kMaxSamples, kStreamMinPrefix, kTailMax, kTailCap).

Every output — the ordered cloud with its labels, ground_mat, both BEVs — is compared byte for byte with the oracle.
Before that each case asserts what it covers: the mode bev_debug_get_frame_info reports per frame (and, for a frame that
went general, k_probe's reason), and that the sweeps hold ground slots, slots phase A could not judge, points labelled 0
and candidates that phase C put back (geometry_cases.covered; where a sensor's synthetic sweep does not give that by
itself — 15 slots, or 1023 ground rows a fraction of a degree apart — geometry_cases.plant_ground puts it there).

One context per case, max_batch 4: process_batch cuts a call into sub-batches of two frames, frame_info describes the
last one, so the frames go up two at a time (two layouts per sub-batch) and then once more all in one call.  The
context's size by bev_create's allocation arithmetic (geometry_cases.context_bytes, max_batch 4, ground_mat wanted):
wide_max 3.5 GB (94 MB of code lists per frame and workspace set: 282 emitters x 20 bands x 4160 words; 8 sets x 4
frames), wide_3rows 3.1 GB, square_max 0.61 GB, tall_max 0.58 GB; every other case below 0.7 GB.

Measured on an MI355X (seconds per test, frame generation and the oracle included): every layout in one call tall_max 1.4,
wide_max 0.9, square_max 0.85, the other corners 0.25 or less; the hidden defects 0.35 or less; the per-function entry
points 0.46 or less; the overflowing code lists 0.2; a threshold case 0.28 or less; a refused neighbour under 0.005 — 44
tests in 9 s."""
import functools

import numpy as np
import pytest

import bev_amd
import geometry_cases as gc
import oracle_lib as orc

pytestmark = pytest.mark.gpu
CORNERS = [name for name, _, _ in gc.ADMITTED]
MAX_BATCH = 4


@pytest.fixture(autouse=True)
def _stream_on(monkeypatch):
    """reading in place is the default (BEV_STREAM=0, read by bev_create, turns it off): pinned here so that a stray
    environment cannot make these tests pass on the general path alone"""
    monkeypatch.setenv("BEV_STREAM", "1")
    monkeypatch.delenv("BEV_CODE_CAP", raising=False)


def _want(p, frames):
    sp = orc.sensor_from_params(p)
    return [orc.process_frame(sp, f) for f in frames]


@functools.lru_cache(maxsize=None)
def _corner(name):
    """(params, frames, expected (mode, reason) per frame, the oracle's outputs per frame): made once per corner"""
    p, frames, expect = gc.corner_frames(name)
    return p, frames, expect, _want(p, frames)


@functools.lru_cache(maxsize=None)
def _corner_defects(name):
    p, frames, expect, _ = _corner(name)
    bad, routes = gc.hidden_defects(p, frames, expect)
    return bad, routes, _want(p, bad)


def _assert_equal(got, want, first, what):
    ordered, multi, single, gm = got
    for i in range(len(ordered)):
        o_ord, o_gm, o_multi, o_single = want[first + i]
        assert ordered[i].tobytes() == o_ord.tobytes(), f"{what}: frame {first + i}: ordered cloud / labels differ"
        assert np.array_equal(gm[i], o_gm), f"{what}: frame {first + i}: ground_mat differs"
        assert np.array_equal(multi[i], o_multi), f"{what}: frame {first + i}: multi BEV differs"
        assert np.array_equal(single[i], o_single), f"{what}: frame {first + i}: single BEV differs"


def _run(p, frames, want, what, whole=True):
    """The frames through one context, two at a time (one sub-batch each: frame_info and code_overflow cover it), then all in
    one call; every output against `want`.  Returns (frame_info rows, code_overflow) per frame."""
    ctx = bev_amd.BevContext(p, device=0, max_batch=MAX_BATCH, max_points=max(8, max(len(f) for f in frames)))
    try:
        chunk = MAX_BATCH // 2
        info, ovf = [], []
        for f0 in range(0, len(frames), chunk):
            part = frames[f0:f0 + chunk]
            got = ctx.process_batch(part, want_ground_mat=True)
            info.append(ctx.frame_info(0, len(part)).astype(np.int64))
            ovf.append(ctx.code_overflow(0, len(part)).astype(np.int64))
            _assert_equal(got, want, f0, what)
        info, ovf = np.concatenate(info), np.concatenate(ovf)
        if whole and len(frames) > chunk:
            _assert_equal(ctx.process_batch(frames, want_ground_mat=True), want, 0, what + ", one call")
            n_last = len(frames) - (len(frames) - 1) // chunk * chunk
            again = ctx.frame_info(0, n_last).astype(np.int64)
            assert again[:, 1].tolist() == info[len(frames) - n_last:, 1].tolist(), (what, again, info)
        return info, ovf
    finally:
        ctx.close()


def _assert_routes(info, expect, what):
    for i, (mode, reason) in enumerate(expect):
        T, got_mode, consumed, failed = (int(v) for v in info[i])
        if mode is None:
            continue
        assert got_mode == mode, (what, i, "mode", info.tolist(), "expected", expect)
        if mode == gc.REDO:
            continue
        if mode == gc.GENERAL:
            assert consumed == reason, (what, i, "reason", info[i].tolist(), "expected", reason)
        else:                       # read in place: every record consumed, no check failed
            assert consumed == T and (failed & 1) == 0, (what, i, info[i].tolist())


# ---- every admitted corner ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CORNERS)
def test_corner_every_layout_in_one_call(name):
    """a sorted sweep with a tail, a structured cloud, firing order (plain, real), an adversarial cloud (non-finite values,
    duplicates, row == N, col == H, 65535 in either field) and an empty frame; invalid returns at the row ends around row
    N - G, at the strip boundaries and all over the last strip (geometry_cases.place_invalid)"""
    p, frames, expect, want = _corner(name)
    for i in range(4):
        assert gc.covered(p, frames[i], want[i]), (name, i, gc.coverage(p, frames[i], want[i]))
    info, _ = _run(p, frames, want, name)
    _assert_routes(info, expect, name)


@pytest.mark.parametrize("name", CORNERS)
def test_corner_defects_hidden_from_the_probe_are_redone(name):
    """per in-place route that the corner's frames took: the same frame with one defect at a position k_probe does not
    sample — the walk catches it, the frame is redone the general way (mode 2), the outputs are the oracle's"""
    p, frames, expect, _ = _corner(name)
    bad, routes, want = _corner_defects(name)
    assert gc.STRUCTURED in routes and gc.COLMAJOR in routes, routes          # (no geometry limit on these two)
    assert (gc.STREAM in routes) == (expect[0][0] == gc.STREAM)
    info, _ = _run(p, bad, want, name + " (defects)", whole=False)
    assert info[:, 1].tolist() == [gc.REDO] * len(bad), (name, routes, info)


@pytest.mark.parametrize("name", gc.LARGE)
def test_corner_per_function_entry_points(name):
    """bev_order_cloud, bev_mark_ground (the identity walk and the ground_mat kernel), bev_multi_bev / bev_single_bev of the
    marked cloud, and bev_process_device_resident with two frames"""
    import torch

    p, frames, _, want = _corner(name)
    sp = orc.sensor_from_params(p)
    S, M, L = p.slots, p.mat_size, p.n_layers
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=max(len(f) for f in frames))
    try:
        for k in (0, 4):            # the sweep with its tail, the adversarial cloud
            plain = ctx.order_cloud(frames[k])
            assert plain.tobytes() == orc.order_cloud(sp, frames[k]).tobytes(), (name, k, "order_cloud")
            marked, gm = ctx.mark_ground(plain)
            assert marked.tobytes() == want[k][0].tobytes(), (name, k, "mark_ground: labels")
            assert np.array_equal(gm, want[k][1]), (name, k, "mark_ground: ground_mat")
            assert np.array_equal(ctx.multi_bev(marked), want[k][2]), (name, k, "multi_bev")
            assert np.array_equal(ctx.single_bev(marked), want[k][3]), (name, k, "single_bev")
        pair = [frames[2], frames[0]]      # firing order, the sweep
        offs = np.zeros(3, np.uint64)
        offs[1:] = np.cumsum([len(f) for f in pair])
        dev = torch.device("cuda:0")
        d_in = torch.from_numpy(np.concatenate(pair).view(np.uint8).reshape(-1)).to(dev)
        outs = [torch.zeros(2 * k, dtype=torch.uint8, device=dev) for k in (S * 32, L * M * M, M * M, S)]
        torch.cuda.synchronize()
        ctx.process_device(2, d_in.data_ptr(), offs, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr())
        ctx.synchronize()
        o, m, s, g = (t.cpu().numpy() for t in outs)
        for i, k in enumerate((2, 0)):
            assert o[i * S * 32:(i + 1) * S * 32].tobytes() == want[k][0].tobytes(), (name, k, "process_device: ordered")
            assert np.array_equal(g[i * S:(i + 1) * S].view(np.int8), want[k][1].reshape(-1)), (name, k, "process_device: ground_mat")
            assert np.array_equal(m[i * L * M * M:(i + 1) * L * M * M], want[k][2].reshape(-1)), (name, k, "process_device: multi")
            assert np.array_equal(s[i * M * M:(i + 1) * M * M], want[k][3].reshape(-1)), (name, k, "process_device: single")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["wide_max", "square_max"])
def test_corner_with_code_lists_that_overflow(name, monkeypatch):
    """BEV_CODE_CAP=300: (writer, band) lists overflow and the raster's fallback reads all S slots of the ordered cloud —
    through the 278 strips' list ends of wide_max (kRasterTailWords) and the 2^20 slots of square_max"""
    p, frames, expect, want = _corner(name)
    monkeypatch.setenv("BEV_CODE_CAP", "300")
    info, ovf = _run(p, frames[:4], want[:4], name + " (BEV_CODE_CAP=300)")
    assert (ovf > 0).all(), (name, ovf)
    _assert_routes(info, expect[:4], name)


# ---- the refused neighbours ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nhg,status", gc.REFUSED, ids=["x".join(str(v) for v in nhg) for nhg, _ in gc.REFUSED])
def test_refused_neighbours(nhg, status):
    p = gc.params(*nhg)
    with pytest.raises(bev_amd.BevError, match=rf"\(status {status}\)"):
        bev_amd.BevContext(p, device=0, max_batch=1, max_points=1024).close()


# ---- the threshold pairs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nhg,make", gc.THRESHOLDS, ids=[t[0] for t in gc.THRESHOLDS])
def test_threshold(name, nhg, make):
    """the case inside the threshold takes the in-place route, the one outside goes general with k_probe's reason; both
    equal the oracle (the kCm* pairs: real sweeps with no-return records in column 0, 3 % and 20 % of the records)"""
    p = gc.params(*nhg)
    rows = make(p)
    frames, expect = [r[0] for r in rows], [(r[1], r[2]) for r in rows]
    want = _want(p, frames)
    for i, f in enumerate(frames):
        assert gc.covered(p, f, want[i]), (name, i, gc.coverage(p, f, want[i]))
    if name.startswith("cm_"):
        for f in frames[:2]:
            noret = (f["x"] == 0) & (f["y"] == 0) & (f["z"] == 0)
            assert noret.sum() > 100 and (f["col"][noret] == 0).all(), name
    info, _ = _run(p, frames, want, name)
    _assert_routes(info, expect, name)
