"""GPU: the float max-height BEV of a batch of frames under per-frame poses (bev_float_bev_device_resident,
bev_float_bev_batch).  The checkers are the oracle's saveAsMat and transformPointCloud (orc.float_bev,
orc.transform_cloud); every comparison is of bytes."""
import functools

import numpy as np
import pytest
import torch

import bev_amd
import oracle_lib as orc
import packed_cases
from bev_amd import FLOAT_BEV_MAX_POSES, POINT_DTYPE, synth
from packed_cases import (FAR, GUARD, INVALID, PATTERN, POSES, TOO_LARGE, UNSUPPORTED, _adversarial, _dev, _marked, _matrix,
                          _one_cell, _p, _pack)

pytestmark = pytest.mark.gpu
_ragged_frames = functools.partial(packed_cases._ragged_frames, 9, 24, (0,))


def _out(n_grids, M):
    return torch.full((n_grids * M * M * 4 + GUARD,), PATTERN, dtype=torch.uint8, device=torch.device("cuda:0"))


def _grids(t, n_grids, M):
    return t[:n_grids * M * M * 4].cpu().numpy().view(np.float32).reshape(n_grids, M, M)


def _guard_ok(t, n_grids, M):
    return bool((t[n_grids * M * M * 4:] == PATTERN).all())


def _want(cloud, interval, skip, m=None):
    return orc.float_bev(cloud if m is None else orc.transform_cloud(cloud, m), interval, skip)


@pytest.mark.parametrize("interval,skip", [(1.0, 1), (2.0, 0), (0.5, 1)])
def test_one_call_rasters_ragged_frames_bit_identically(interval, skip):
    frames = _ragged_frames()
    nf = len(frames)
    offs, flat = _pack(frames)
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=4, max_points=p.slots)
    try:
        M = int(ctx.lib.bev_float_bev_size(interval))
        assert M == {1.0: 201, 2.0: 101, 0.5: 401}[interval]
        d_in, d_out = _dev(flat), _out(nf, M)
        torch.cuda.synchronize()
        ctx.float_bev_device(nf, d_in.data_ptr(), offs, d_out.data_ptr(), interval, bool(skip))
        ctx.synchronize()
        got = _grids(d_out, nf, M)
        for f, cloud in enumerate(frames):
            assert got[f].tobytes() == _want(cloud, interval, bool(skip)).tobytes(), (f, len(cloud))
            if len(cloud) == 0:
                assert not got[f].any(), f
        assert got[-3].any()   # the full sweep
        assert _guard_ok(d_out, nf, M), "something was written behind d_out"
    finally:
        ctx.close()


def test_contention_and_the_zero_threshold():
    """every point of a frame in ONE cell: the atomic's maximum under contention, and what must not be stored
    (z + 2 <= 0, NaN)"""
    fmax = np.finfo(np.float32).max
    rng = np.random.default_rng(5)
    plain = rng.permutation(np.linspace(-1.99, 60.0, 20000 - 9).astype(np.float32))
    assert len(np.unique(plain)) == len(plain)
    special = np.array([-5.0, -2.0, -2.0000002, 0.0, -0.0, np.nan, -np.inf, fmax, np.inf], dtype=np.float32)
    with_inf = np.concatenate([plain[:7000], special, plain[7000:]])
    finite = np.concatenate([plain[:7000], special[:-2], plain[7000:]])
    low = np.array([-5.0, -2.0, -2.0000002, -np.inf, np.nan, -1e30] * 50, dtype=np.float32)   # nothing is stored
    frames = [_one_cell(with_inf), _one_cell(finite), _one_cell(low), _one_cell(np.full(4096, 1.625, np.float32)),
              _one_cell(np.concatenate([finite, [np.float32(fmax)]]))]
    assert len(frames[0]) == 20000
    nf = len(frames)
    offs, flat = _pack(frames)
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        for skip in (True, False):
            d_in, d_out = _dev(flat), _out(nf, 201)
            torch.cuda.synchronize()
            ctx.float_bev_device(nf, d_in.data_ptr(), offs, d_out.data_ptr(), 1.0, skip)
            ctx.synchronize()
            got = _grids(d_out, nf, 201)
            for f, cloud in enumerate(frames):
                assert got[f].tobytes() == _want(cloud, 1.0, skip).tobytes(), f
            assert [int(np.count_nonzero(g)) for g in got] == [1, 1, 0, 1, 1]
            assert got[0].max() == np.inf and got[1].max() == np.float32(plain.max()) + np.float32(2)
            assert got[3].max() == np.float32(3.625) and got[4].max() == fmax
            assert _guard_ok(d_out, nf, 201)
    finally:
        ctx.close()


def _nonfinite_cloud():
    """the non-finite adversarial cloud plus points whose z is not finite while x and y are on the grid: an identity
    matrix turns their x and y into NaN (0 * inf), the raw coordinates keep them"""
    extra = np.zeros(4, dtype=POINT_DTYPE)
    extra["x"], extra["y"], extra["label"] = [1.0, 2.0, -3.0, 4.0], [1.0, -2.0, 3.0, 4.5], 1
    extra["z"] = [np.inf, np.inf, np.nan, -np.inf]
    return np.concatenate([_adversarial()[:30000], extra])


def test_poses():
    adv, marked = _adversarial(), _marked()
    frames = [marked[:50001], adv[:0], _nonfinite_cloud(), marked[60000:60257], adv[100:1125], marked[90000:133312]]
    nf, n_poses = len(frames), 5
    poses = np.stack([np.stack([_matrix((POSES + POSES)[f + k][:3] + (POSES[k][3] + f,)) for k in range(4)] + [_matrix(FAR)])
                      for f in range(nf)])
    assert poses.shape == (nf, n_poses, 12)
    offs, flat = _pack(frames)
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        d_in = _dev(flat)
        for interval, skip in ((1.0, False), (2.0, True)):
            M = int(ctx.lib.bev_float_bev_size(interval))
            d_out = _out(nf * n_poses, M)
            torch.cuda.synchronize()
            ctx.float_bev_device(nf, d_in.data_ptr(), offs, d_out.data_ptr(), interval, skip, poses=poses)
            ctx.synchronize()
            got = _grids(d_out, nf * n_poses, M).reshape(nf, n_poses, M, M)
            for f, cloud in enumerate(frames):
                for k in range(n_poses):
                    assert got[f, k].tobytes() == _want(cloud, interval, skip, poses[f, k]).tobytes(), (interval, f, k)
            if not skip:   # FAR pushes most points off the grid
                assert got[0, 0].any() and np.count_nonzero(got[0, 4]) < np.count_nonzero(got[0, 0]) // 2
            assert _guard_ok(d_out, nf * n_poses, M)

        # the most poses a call takes, and one pose, on a frame that does not fill its last workgroup
        cloud = marked[20000:24097]
        o1, flat1 = _pack([cloud])
        d_one = _dev(flat1)
        rng = np.random.default_rng(2)
        many = np.stack([_matrix((rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(-1, 1), rng.uniform(-180, 180)))
                         for _ in range(FLOAT_BEV_MAX_POSES)])[None]
        for ps in (many, many[:, 7:8]):
            n = ps.shape[1]
            d_out = _out(n, 201)
            torch.cuda.synchronize()
            ctx.float_bev_device(1, d_one.data_ptr(), o1, d_out.data_ptr(), 1.0, True, poses=ps)
            ctx.synchronize()
            got = _grids(d_out, n, 201)
            for k in range(n):
                assert got[k].tobytes() == _want(cloud, 1.0, True, ps[0, k]).tobytes(), (n, k)
            assert _guard_ok(d_out, n, 201)

        # no poses is NOT the identity pose
        cloud = _nonfinite_cloud()
        identity = _matrix((0, 0, 0, 0))
        assert np.array_equal(identity, np.eye(3, 4, dtype=np.float32).reshape(12))
        raw, through_identity = _want(cloud, 1.0, False), _want(cloud, 1.0, False, identity)
        assert raw.tobytes() != through_identity.tobytes()
        o1, flat1 = _pack([cloud])
        d_one, d_out = _dev(flat1), _out(2, 201)
        torch.cuda.synchronize()
        ctx.float_bev_device(1, d_one.data_ptr(), o1, d_out.data_ptr(), 1.0, False)
        ctx.float_bev_device(1, d_one.data_ptr(), o1, d_out.data_ptr() + 201 * 201 * 4, 1.0, False, poses=identity[None, None])
        ctx.synchronize()
        got = _grids(d_out, 2, 201)
        assert got[0].tobytes() == raw.tobytes() and got[1].tobytes() == through_identity.tobytes()
    finally:
        ctx.close()


def test_stream_ordering_with_the_bev_path():
    """process_device, then float_bev_device on its d_ordered with nothing between them while the default stream is busy;
    then float_bev_device followed at once by a process_device that overwrites d_ordered; then two float_bev_device calls
    of different sizes back to back.  One synchronize() ends each."""
    p = _p()
    sp = orc.sensor_from_params(p)
    S, M = p.slots, 201
    dev = torch.device("cuda:0")
    first = [synth.sweep(p, 30), synth.sweep(p, 31)[:70000], synth.adversarial(p, 20000, 4)]
    other = [synth.sweep(p, 32)[:90000], synth.adversarial(p, 30000, 6), synth.sweep(p, 33)]
    nf = len(first)
    want = {k: [orc.mark_ground(sp, orc.order_cloud(sp, c))[0] for c in fs] for k, fs in (("first", first), ("other", other))}
    offs_s = np.arange(nf + 1, dtype=np.uint64) * np.uint64(S)
    ctx = bev_amd.BevContext(p, device=0, max_batch=4, max_points=S + 8192)
    try:
        (o1, flat1), (o2, flat2) = _pack(first), _pack(other)
        src1, d_other = _dev(flat1), _dev(flat2)
        d_pts = torch.zeros_like(src1)
        d_ordered = torch.zeros(nf * S * 32, dtype=torch.uint8, device=dev)
        d_multi = torch.zeros(nf * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device=dev)
        d_single = torch.zeros(nf * p.mat_size ** 2, dtype=torch.uint8, device=dev)
        g1, g2 = _out(nf, M), _out(nf, M)
        busy = torch.randn(4096, 4096, device=dev)
        torch.cuda.synchronize()
        for _ in range(4):   # the default stream is busy when the library is called: the fill below is still queued
            busy = busy @ busy * 1e-3
        d_pts.copy_(src1)
        ctx.process_device(nf, d_pts.data_ptr(), o1, d_ordered.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
        ctx.float_bev_device(nf, d_ordered.data_ptr(), offs_s, g1.data_ptr(), 1.0, True)
        ctx.synchronize()
        for f in range(nf):
            assert _grids(g1, nf, M)[f].tobytes() == _want(want["first"][f], 1.0, True).tobytes(), f

        # reverse order: the raster still reads d_ordered when the pipeline that overwrites it is issued
        ctx.float_bev_device(nf, d_ordered.data_ptr(), offs_s, g2.data_ptr(), 1.0, False)
        ctx.process_device(nf, d_other.data_ptr(), o2, d_ordered.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
        ctx.synchronize()
        got_ordered = d_ordered.cpu().numpy().view(POINT_DTYPE).reshape(nf, S)
        for f in range(nf):
            assert _grids(g2, nf, M)[f].tobytes() == _want(want["first"][f], 1.0, False).tobytes(), f
            assert got_ordered[f].tobytes() == want["other"][f].tobytes(), f
        assert _guard_ok(g1, nf, M) and _guard_ok(g2, nf, M)

        # two calls of different sizes back to back: the second call's table follows the first call's launch
        frames = _ragged_frames()[4:11]
        ox, flatx = _pack(frames)
        d_x = _dev(flatx)
        poses = np.stack([np.stack([_matrix(POSES[1]), _matrix(POSES[(f % 3) + 2])]) for f in range(nf)])
        ga, gb = _out(nf * 2, M), _out(len(frames), M)
        torch.cuda.synchronize()
        ctx.float_bev_device(nf, d_ordered.data_ptr(), offs_s, ga.data_ptr(), 1.0, True, poses=poses)
        ctx.float_bev_device(len(frames), d_x.data_ptr(), ox, gb.data_ptr(), 1.0, True)
        ctx.synchronize()
        for f in range(nf):
            for k in range(2):
                assert _grids(ga, nf * 2, M)[2 * f + k].tobytes() == _want(want["other"][f], 1.0, True, poses[f, k]).tobytes(), (f, k)
        for f, cloud in enumerate(frames):
            assert _grids(gb, len(frames), M)[f].tobytes() == _want(cloud, 1.0, True).tobytes(), f
        assert _guard_ok(ga, nf * 2, M) and _guard_ok(gb, len(frames), M)
    finally:
        ctx.close()


def test_status_codes():
    p = _p()
    C = bev_amd.C
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=1000)   # frames of up to max(max_points, S) = S records
    try:
        frames = [_marked()[:3000], _marked()[3000:8000]]
        offs, flat = _pack(frames)
        d_in, d_out = _dev(flat), _out(2 * 2, 201)
        pose = np.ascontiguousarray(np.stack([_matrix(POSES[1])] * 4).reshape(2, 2, 12))
        torch.cuda.synchronize()
        L = ctx.lib
        u64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64)) if a is not None else None
        fp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None

        def call(h=ctx._h, n=2, din=d_in.data_ptr(), o=offs, interval=1.0, n_poses=0, poses=None, dout=d_out.data_ptr()):
            return L.bev_float_bev_device_resident(h, n, din, u64p(o), interval, 1, n_poses, fp(poses), dout)

        assert call(h=None) == INVALID
        assert call(n=-1) == INVALID
        assert call(o=None) == INVALID
        assert call(o=np.array([0, 5000, 3000], dtype=np.uint64)) == INVALID          # decreasing offsets
        assert call(n_poses=-1, poses=pose) == INVALID
        assert call(n_poses=FLOAT_BEV_MAX_POSES + 1, poses=pose) == INVALID
        assert call(n_poses=2, poses=None) == INVALID
        assert call(din=None) == INVALID                                              # NULL pointers with work to do
        assert call(dout=None) == INVALID
        assert call(dout=None, o=np.zeros(3, dtype=np.uint64)) == INVALID             # (empty frames still get their grids)
        for interval in (0.0, -1.0, float("nan"), 0.1):                               # M = 0, or above 1024
            assert L.bev_float_bev_size(interval) == 0
            assert call(interval=interval) == UNSUPPORTED
        assert call(n=1, o=np.array([0, p.slots + 1], dtype=np.uint64)) == TOO_LARGE  # a frame above max(max_points, S)
        assert call(n=0, o=offs[:1].copy(), din=None, dout=None) == 0                 # nothing to do
        ctx.synchronize()
        assert bool((d_out == PATTERN).all()), "a refused call wrote to d_out"

        # the host-buffer call refuses the same things
        cl = (C.c_void_p * 2)(*[f.ctypes.data for f in frames])
        n_pts = (C.c_uint32 * 2)(3000, 5000)
        host = np.full((2, 2, 201, 201), -7.0, dtype=np.float32)
        outs = (C.c_void_p * 2)(*[host[i].ctypes.data for i in range(2)])

        def hcall(h=ctx._h, n=2, clouds=cl, npts=n_pts, interval=1.0, n_poses=0, poses=None, out=outs):
            return L.bev_float_bev_batch(h, n, clouds, npts, interval, 1, n_poses, fp(poses), out)

        assert hcall(h=None) == INVALID and hcall(n=-1) == INVALID
        assert hcall(clouds=None) == INVALID and hcall(npts=None) == INVALID and hcall(out=None) == INVALID
        assert hcall(clouds=(C.c_void_p * 2)(frames[0].ctypes.data, None)) == INVALID
        assert hcall(out=(C.c_void_p * 2)(host[0].ctypes.data, None)) == INVALID
        assert hcall(n_poses=FLOAT_BEV_MAX_POSES + 1, poses=pose) == INVALID and hcall(n_poses=1, poses=None) == INVALID
        assert hcall(interval=0.0) == UNSUPPORTED
        assert hcall(npts=(C.c_uint32 * 2)(3000, p.slots + 1)) == TOO_LARGE
        assert hcall(n=0, clouds=None, npts=None, out=None) == 0
        assert (host == -7.0).all(), "a refused call wrote to its outputs"

        # valid calls still work
        assert call(n_poses=2, poses=pose) == 0
        ctx.synchronize()
        got = _grids(d_out, 4, 201)
        for f, cloud in enumerate(frames):
            for k in range(2):
                assert got[2 * f + k].tobytes() == _want(cloud, 1.0, True, pose[f, k]).tobytes()
        assert _guard_ok(d_out, 4, 201)
        assert hcall(n_poses=2, poses=pose) == 0
        assert host.tobytes() == got.tobytes()
    finally:
        ctx.close()


def test_host_buffers_in_chunks():
    """7 frames through a context of max_batch 2: four chunks; against the per-cloud entry points and the oracle"""
    adv, marked = _adversarial(), _marked()
    frames = [marked, adv[:40000], adv[:0], marked[5000:5257], adv[7:1032], marked[:100000], adv[20000:60000]]
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        for interval, skip in ((1.0, True), (2.0, False)):
            got = ctx.float_bev_batch(frames, interval, skip)
            M = got.shape[-1]
            assert got.shape == (7, 1, M, M)
            for f, cloud in enumerate(frames):
                assert got[f, 0].tobytes() == _want(cloud, interval, skip).tobytes(), (interval, f)
                assert got[f, 0].tobytes() == ctx.float_bev(cloud, interval, skip).tobytes(), (interval, f)
        poses = np.stack([np.stack([_matrix(POSES[(f + k) % 5]) for k in range(2)] + [_matrix(FAR)]) for f in range(7)])
        got = ctx.float_bev_batch(frames, 1.0, True, poses=poses)
        assert got.shape == (7, 3, 201, 201)
        for f, cloud in enumerate(frames):
            for k in range(3):
                assert got[f, k].tobytes() == _want(cloud, 1.0, True, poses[f, k]).tobytes(), (f, k)
                moved = ctx.transform_cloud(cloud, poses[f, k])
                assert got[f, k].tobytes() == ctx.float_bev(moved, 1.0, True).tobytes(), (f, k)
        again = ctx.float_bev_batch(frames[:3], 1.0, True)      # a smaller call behind a larger one
        for f in range(3):
            assert again[f, 0].tobytes() == _want(frames[f], 1.0, True).tobytes()
        assert ctx.float_bev_batch([], 1.0, True).shape == (0, 1, 201, 201)
    finally:
        ctx.close()
