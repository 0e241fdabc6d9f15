"""GPU: the batched, device-resident projection of raw sweeps (bev_project_device_resident, bev_process_batch_xyzi;
DESIGN.md §6e).  The checker is the oracle's literal restatement of the selectors' loops (orc.project) and, behind it, the
oracle's hot path (orc.process_frame); every comparison is of bytes.

Measured on the MI355X: k_probe gives the projected MulRan batch of test_projected_frames_take_the_in_place_routes mode 4
(the plain firing-order sweep, as for synth.firing_order frames) and the projected KITTI sweeps mode 3; nothing fails."""
import numpy as np
import pytest
import torch

import bev_amd
import oracle_lib as orc
from bev_amd import KITTI_SLOTS, POINT_DTYPE
from projection_data import KITTI_VARIANTS, kitti_returns, raw_returns

pytestmark = pytest.mark.gpu
MULRAN, OXFORD, KITTI = 0, 1, 2
SENSOR = {MULRAN: "OS1_64", OXFORD: "HDL_32E", KITTI: "HDL_64E"}
GUARD = 4096          # records behind d_out (and between the frames of the one-frame KITTI calls)
PATTERN = 0xA5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(torch.device("cuda:0"))


def _as_input(kind, returns):
    """(n, 4) returns as the kind's file holds them: interleaved, or Oxford's four planes"""
    return np.ascontiguousarray(returns.T) if kind == OXFORD else np.ascontiguousarray(returns)


def _pack(frames):
    offs = np.zeros(len(frames) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([f.size // 4 for f in frames])
    flat = np.concatenate([f.reshape(-1) for f in frames] + [np.zeros(4, np.float32)])
    return offs, flat


def _records(t, first, n):
    return t[first * 32:(first + n) * 32].cpu().numpy().view(POINT_DTYPE)


def _ragged_frames(kind):
    """40 frames: empty ones first, last and next to each other; lengths around the workgroup's 256 / 1024 returns and the
    KITTI acceptance limit (1250); returns with non-finite values; for KITTI every variant of kitti_returns, two seeds each,
    and one frame of 480 k returns"""
    pool = [raw_returns(70000, seed) for seed in (0, 1)]
    small = [0, 0, 1, 2, 255, 256, 257, 1250, 1251, 1023, 1024, 1025, 0, 4097]
    frames = [pool[i % 2][37 * i:37 * i + n] for i, n in enumerate(small)]
    if kind == KITTI:
        seam = kitti_returns(3, "noisy_seam")
        frames += [seam[:n] for n in (1, 2, 255, 256, 257, 1250, 1251, 5000)]
        frames += [kitti_returns(seed, v) for v in KITTI_VARIANTS for seed in (0, 1)]
        frames += [np.concatenate([kitti_returns(s, "sweep") for s in range(4)])]   # 480 k returns: rings run out after 64
        frames += [pool[1][:20000]]
    else:
        rng = np.random.default_rng(7)
        frames += [pool[i % 2][:int(n)] for i, n in enumerate(rng.integers(3000, 70001, 22))]
        frames += [pool[0][:65536], pool[1][:0]]
    frames += [pool[0][:0], pool[0][:0]]
    assert len(frames) == 40
    return [_as_input(kind, f) for f in frames]


@pytest.mark.parametrize("kind", [MULRAN, OXFORD, KITTI])
def test_one_call_projects_ragged_frames_bit_identically(kind):
    frames = _ragged_frames(kind)
    nf = len(frames)
    offs, flat = _pack(frames)
    p = bev_amd.params_for_sensor(SENSOR[kind])
    ctx = bev_amd.BevContext(p, device=0, max_batch=4, max_points=600000)
    try:
        n_out = bev_amd.project_batch_out_points(kind, nf, offs)
        assert n_out == (nf * KITTI_SLOTS if kind == KITTI else int(offs[-1]))
        d_in = _dev(flat)
        d_out = torch.full(((n_out + GUARD) * 32,), PATTERN, dtype=torch.uint8, device=d_in.device)
        torch.cuda.synchronize()
        ctx.project_device(kind, nf, d_in.data_ptr(), offs, d_out.data_ptr())
        ctx.synchronize()
        for f, raw in enumerate(frames):
            want = orc.project(kind, raw)
            first = f * KITTI_SLOTS if kind == KITTI else int(offs[f])
            assert _records(d_out, first, len(want)).tobytes() == want.tobytes(), (f, raw.size // 4)
        assert bool((d_out[n_out * 32:] == PATTERN).all()), "records were written behind d_out"
        if kind == KITTI:   # a frame's structured cloud is exactly 64 * 2083 records: guards between one-frame calls
            pick = [0, 2, 9, 22, 35, 36]
            stride = KITTI_SLOTS + GUARD
            d_sep = torch.full((len(pick) * stride * 32,), PATTERN, dtype=torch.uint8, device=d_in.device)
            torch.cuda.synchronize()
            for j, f in enumerate(pick):
                ctx.project_device(kind, 1, d_in.data_ptr(), offs[f:f + 2], d_sep.data_ptr() + j * stride * 32)
            ctx.synchronize()
            for j, f in enumerate(pick):
                assert _records(d_sep, j * stride, KITTI_SLOTS).tobytes() == orc.project(kind, frames[f]).tobytes(), f
                guard = d_sep[(j * stride + KITTI_SLOTS) * 32:(j + 1) * stride * 32]
                assert bool((guard == PATTERN).all()), f
    finally:
        ctx.close()


def _kitti_batch(n):
    """ragged sweeps, a different variant on either side of every frame boundary"""
    out = []
    for f in range(n):
        r = kitti_returns(f % 2, KITTI_VARIANTS[f % len(KITTI_VARIANTS)])
        out.append(np.ascontiguousarray(r[:len(r) - 1500 * f]))
    return out


@pytest.mark.parametrize("group", [None, 5])
def test_kitti_launch_groups(monkeypatch, group):
    """more frames than one launch group: two boundaries are crossed (2 * group + 3 frames), whatever the group size is"""
    if group is not None:
        monkeypatch.setenv("BEV_PROJECT_GROUP", str(group))
    nf = 2 * bev_amd.PROJECT_KITTI_GROUP + 3
    frames = _kitti_batch(nf)
    offs, flat = _pack(frames)
    p = bev_amd.params_for_sensor("HDL_64E")
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        d_in = _dev(flat)
        d_out = torch.full(((nf * KITTI_SLOTS + GUARD) * 32,), PATTERN, dtype=torch.uint8, device=d_in.device)
        torch.cuda.synchronize()
        ctx.project_device(KITTI, nf, d_in.data_ptr(), offs, d_out.data_ptr())
        ctx.synchronize()
        for f, raw in enumerate(frames):
            assert _records(d_out, f * KITTI_SLOTS, KITTI_SLOTS).tobytes() == orc.project(KITTI, raw).tobytes(), f
        assert bool((d_out[nf * KITTI_SLOTS * 32:] == PATTERN).all())
    finally:
        ctx.close()


class _Outputs:
    def __init__(self, p, nf, dev):
        self.p, self.nf = p, nf
        self.ordered = torch.zeros(nf * p.slots * 32, dtype=torch.uint8, device=dev)
        self.multi = torch.zeros(nf * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device=dev)
        self.single = torch.zeros(nf * p.mat_size ** 2, dtype=torch.uint8, device=dev)
        self.gm = torch.zeros(nf * p.slots, dtype=torch.int8, device=dev)

    def process(self, ctx, d_pts, offs):
        ctx.process_device(self.nf, d_pts, offs, self.ordered.data_ptr(), self.multi.data_ptr(), self.single.data_ptr(),
                           self.gm.data_ptr())

    def check(self, clouds, what):
        p, sp = self.p, orc.sensor_from_params(self.p)
        ordered = self.ordered.cpu().numpy().view(POINT_DTYPE).reshape(self.nf, p.slots)
        multi = self.multi.cpu().numpy().reshape(self.nf, p.n_layers, p.mat_size, p.mat_size)
        single = self.single.cpu().numpy().reshape(self.nf, p.mat_size, p.mat_size)
        gm = self.gm.cpu().numpy().reshape(self.nf, p.n_scan, p.horizon_scan)
        for f, cloud in enumerate(clouds):
            o_ord, o_gm, o_multi, o_single = orc.process_frame(sp, cloud)
            assert ordered[f].tobytes() == o_ord.tobytes(), (what, f, "ordered cloud / labels")
            assert np.array_equal(gm[f], o_gm), (what, f, "ground_mat")
            assert np.array_equal(multi[f], o_multi) and np.array_equal(single[f], o_single), (what, f, "rasters")


def test_stream_ordering_with_the_bev_path():
    """torch fills d_xyzi on the default stream; project_device and process_device follow back to back, twice with
    batches of different sizes, and one synchronize() ends it.  Then the reverse: a process_device whose input the next
    project_device overwrites."""
    p = bev_amd.params_for_sensor("OS1_64")
    dev = torch.device("cuda:0")
    pool = raw_returns(70000, 5, nonfinite=False)
    sizes = [[65536, 30000, 0, 51234, 65536], [12345, 65536, 65536, 40000, 1, 65536, 22222, 65536, 60000]]
    ctx = bev_amd.BevContext(p, device=0, max_batch=4, max_points=65536)
    try:
        calls = []
        for c, ns in enumerate(sizes):
            frames = [np.ascontiguousarray(np.roll(pool, 1000 * (c + 3 * i), axis=0)[:n]) for i, n in enumerate(ns)]
            offs, flat = _pack(frames)
            calls.append(dict(frames=frames, offs=offs, src=_dev(flat), xyzi=torch.zeros(flat.size, dtype=torch.float32, device=dev),
                              recs=torch.full((int(offs[-1]) * 32 + 32,), PATTERN, dtype=torch.uint8, device=dev),
                              out=_Outputs(p, len(frames), dev)))
        busy = torch.randn(4096, 4096, device=dev)
        torch.cuda.synchronize()
        for c in calls:
            for _ in range(4):   # the default stream is busy when the library is called: the fill below is still queued
                busy = busy @ busy * 1e-3
            c["xyzi"].copy_(c["src"].view(torch.float32))
            ctx.project_device(MULRAN, len(c["frames"]), c["xyzi"].data_ptr(), c["offs"], c["recs"].data_ptr())
            c["out"].process(ctx, c["recs"].data_ptr(), c["offs"])
        ctx.synchronize()
        for k, c in enumerate(calls):
            c["out"].check([orc.project(MULRAN, f) for f in c["frames"]], f"call {k}")

        # reverse order: the pipeline of call 1 still reads its records when the projection that overwrites them is issued
        c = calls[1]
        first = [orc.project(MULRAN, f) for f in c["frames"]]
        other = [np.ascontiguousarray(f[::-1]) for f in c["frames"]]
        _, flat2 = _pack(other)
        d_other = _dev(flat2)
        again = _Outputs(p, len(first), dev)
        torch.cuda.synchronize()
        again.process(ctx, c["recs"].data_ptr(), c["offs"])
        ctx.project_device(MULRAN, len(other), d_other.data_ptr(), c["offs"], c["recs"].data_ptr())
        ctx.synchronize()
        again.check(first, "overwritten input")
        for f, raw in enumerate(other):
            n = raw.size // 4
            assert _records(c["recs"], int(c["offs"][f]), n).tobytes() == orc.project(MULRAN, raw).tobytes(), f
    finally:
        ctx.close()


def _mulran_firing_sweep(seed):
    """return k = firing * 64 + beam at azimuth 2 pi (firing + 0.25) / 1024, the beams' elevations spread over +-16.6
    degrees, range 20"""
    rng = np.random.default_rng(seed)
    firing, beam = np.divmod(np.arange(65536), 64)
    az = 2 * np.pi * (firing + 0.25) / 1024
    el = np.deg2rad(16.6 - 33.2 * beam / 63.0)
    r = 20.0
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), rng.random(65536)],
                    axis=1).astype(np.float32)


def test_projected_frames_take_the_in_place_routes():
    dev = torch.device("cuda:0")
    # MulRan: firing-order frames
    frames = [_mulran_firing_sweep(s) for s in range(5)]
    firing, beam = np.divmod(np.arange(65536), 64)
    want = [orc.project(MULRAN, f) for f in frames]
    for w in want:
        assert np.array_equal(w["col"], firing) and np.array_equal(w["row"], beam)
    p = bev_amd.params_for_sensor("OS1_64")
    ctx = bev_amd.BevContext(p, device=0, max_batch=16, max_points=65536)
    try:
        offs, flat = _pack(frames)
        d_in, d_rec = _dev(flat), torch.zeros(int(offs[-1]) * 32, dtype=torch.uint8, device=dev)
        out = _Outputs(p, len(frames), dev)
        torch.cuda.synchronize()
        ctx.project_device(MULRAN, len(frames), d_in.data_ptr(), offs, d_rec.data_ptr())
        out.process(ctx, d_rec.data_ptr(), offs)
        ctx.synchronize()
        info = ctx.frame_info(0, len(frames))
        print("MulRan frame_info (T, mode, consumed, failed):", info.tolist())
        out.check(want, "mulran")
        assert all(int(m) in (4, 5) for m in info[:, 1]), info
        assert all((int(x) & 1) == 0 for x in info[:, 3]), info
    finally:
        ctx.close()
    # KITTI: structured frames
    sweeps = [kitti_returns(s, v) for s, v in [(9, "sweep"), (2, "noisy_seam"), (4, "short_rings"), (1, "late_start")]]
    p = bev_amd.params_for_sensor("HDL_64E")
    ctx = bev_amd.BevContext(p, device=0, max_batch=16, max_points=p.slots)
    try:
        offs, flat = _pack(sweeps)
        offs_s = np.arange(len(sweeps) + 1, dtype=np.uint64) * np.uint64(KITTI_SLOTS)
        d_in, d_rec = _dev(flat), torch.zeros(len(sweeps) * KITTI_SLOTS * 32, dtype=torch.uint8, device=dev)
        out = _Outputs(p, len(sweeps), dev)
        torch.cuda.synchronize()
        ctx.project_device(KITTI, len(sweeps), d_in.data_ptr(), offs, d_rec.data_ptr())
        out.process(ctx, d_rec.data_ptr(), offs_s)
        ctx.synchronize()
        info = ctx.frame_info(0, len(sweeps))
        print("KITTI frame_info (T, mode, consumed, failed):", info.tolist())
        out.check([orc.project(KITTI, f) for f in sweeps], "kitti")
        assert [int(m) for m in info[:, 1]] == [3] * len(sweeps), info
        assert all((int(x) & 1) == 0 for x in info[:, 3]), info
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", [MULRAN, OXFORD, KITTI])
def test_host_route_equals_process_batch_of_the_projected_clouds(kind):
    """11 frames through a context of max_batch 4: six chunks, both halves of the staging"""
    if kind == KITTI:
        raws = [kitti_returns(s, KITTI_VARIANTS[s % len(KITTI_VARIANTS)]) for s in range(9)]
        raws = [r[:len(r) - 3000 * i] for i, r in enumerate(raws)] + [raws[0][:0], raws[1][:700]]
    else:
        pool = raw_returns(70000, 11)
        cap = 65536 if kind == MULRAN else 40000
        raws = [np.roll(pool, 777 * i, axis=0)[:cap - 2500 * i] for i in range(9)] + [pool[:0], pool[:300]]
    frames = [_as_input(kind, r) for r in raws]
    p = bev_amd.params_for_sensor(SENSOR[kind])
    ctx = bev_amd.BevContext(p, device=0, max_batch=4, max_points=max(p.slots, 70000))
    try:
        got = ctx.process_batch_xyzi(kind, frames, want_ground_mat=True)
        want = ctx.process_batch([orc.project(kind, f) for f in frames], want_ground_mat=True)
        for name, g, w in zip(("ordered", "multi", "single", "ground_mat"), got, want):
            for f in range(len(frames)):
                assert g[f].tobytes() == w[f].tobytes(), (name, f)
        for other in (MULRAN, OXFORD, KITTI):
            if other != kind:
                with pytest.raises(bev_amd.BevError, match=r"status -5"):
                    ctx.process_batch_xyzi(other, frames[:1])
        again = ctx.process_batch_xyzi(kind, frames[:3], want_ground_mat=True)
        for g, w in zip(again, want):
            assert g.tobytes() == w[:3].tobytes()
    finally:
        ctx.close()


def test_arguments():
    p = bev_amd.params_for_sensor("OS1_64")
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=70000)
    dev = torch.device("cuda:0")
    try:
        raw = raw_returns(70000, 2)
        frames = [raw[:3000], raw[3000:8000]]
        offs, flat = _pack(frames)
        d_in = _dev(flat)
        d_out = torch.full((8000 * 32 + 64,), PATTERN, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        L = ctx.lib
        u64p = lambda a: a.ctypes.data_as(bev_amd.C.POINTER(bev_amd.C.c_uint64))
        call = lambda kind, n, din, o, dout: L.bev_project_device_resident(ctx._h, kind, n, din, u64p(o), dout)
        assert call(3, 2, d_in.data_ptr(), offs, d_out.data_ptr()) == -1          # bad kind
        assert call(-1, 2, d_in.data_ptr(), offs, d_out.data_ptr()) == -1
        down = np.array([0, 5000, 3000], dtype=np.uint64)
        assert call(MULRAN, 2, d_in.data_ptr(), down, d_out.data_ptr()) == -1     # decreasing offsets
        assert bev_amd.project_batch_out_points(MULRAN, 2, down) == 0
        assert bev_amd.project_batch_out_points(7, 2, offs) == 0
        big = np.array([0, 70001], dtype=np.uint64)
        assert call(MULRAN, 1, d_in.data_ptr(), big, d_out.data_ptr()) == -6      # a frame above max(max_points, S)
        assert call(MULRAN, 2, None, offs, d_out.data_ptr()) == -1                # NULL pointers with work to do
        assert call(MULRAN, 2, d_in.data_ptr(), offs, None) == -1
        assert L.bev_project_device_resident(ctx._h, MULRAN, 2, d_in.data_ptr(), None, d_out.data_ptr()) == -1
        assert call(MULRAN, -1, d_in.data_ptr(), offs, d_out.data_ptr()) == -1
        ctx.synchronize()
        assert bool((d_out == PATTERN).all()), "a refused call wrote records"
        empty = np.zeros(3, dtype=np.uint64)
        assert call(MULRAN, 2, None, empty, None) == 0                            # nothing to do
        assert call(MULRAN, 0, None, empty, None) == 0
        ctx.project_device(MULRAN, 2, d_in.data_ptr(), offs, d_out.data_ptr())    # a valid call still works
        ctx.synchronize()
        for f, fr in enumerate(frames):
            assert _records(d_out, int(offs[f]), len(fr)).tobytes() == orc.project(MULRAN, fr).tobytes()
        assert bool((d_out[8000 * 32:] == PATTERN).all())
    finally:
        ctx.close()
