"""GPU: the 24-layer occupancy BEV and the uint8 max-height BEV of a batch of frames under per-frame poses
(bev_posed_bev_device_resident, bev_posed_bev_batch).  The checker is the oracle's composition — multi_bev /
single_bev of transform_cloud — and, where noted, the per-cloud entry points; every comparison is of bytes."""
import functools
import os

import numpy as np
import pytest
import torch

import bev_amd
import oracle_lib as orc
import packed_cases
from bev_amd import POINT_DTYPE, POSED_BEV_MAX_POSES, synth
from packed_cases import (FAR, GENERAL, INVALID, PATTERN, POSES, TOO_LARGE, _adversarial, _dev, _marked, _matrix, _one_cell, _Out, _p,
                          _pack)

pytestmark = pytest.mark.gpu
_ragged_frames = functools.partial(packed_cases._ragged_frames, 9, 23)


def _want(p, cloud, m=None):
    """(multi, single) of the oracle: the rasters of the moved cloud"""
    moved = cloud if m is None else orc.transform_cloud(cloud, m)
    return orc.multi_bev(orc.sensor_from_params(p), moved, p.interval), orc.single_bev(moved, p.interval)


def _call(ctx, frames, poses=None, multi=True, single=True):
    """one bev_posed_bev_device_resident call over the frames; returns the images (grids, ...) after the guards were checked"""
    offs, flat = _pack(frames)
    K = 1 if poses is None else poses.shape[1]
    d_in, out = _dev(flat), _Out(ctx.params, len(frames) * K, multi, single)
    torch.cuda.synchronize()
    ctx.posed_bev_device(len(frames), d_in.data_ptr(), offs, *out.ptrs(), poses=poses)
    ctx.synchronize()
    assert out.guards_ok(), "something was written behind an output"
    return out.images()


def _check(p, frames, poses, got_multi, got_single, want=None):
    """every grid against the oracle (want: precomputed {(f, k): (multi, single)})"""
    K = 1 if poses is None else poses.shape[1]
    for f, cloud in enumerate(frames):
        for k in range(K):
            wm, ws = want[f, k] if want is not None else _want(p, cloud, None if poses is None else poses[f, k])
            if got_multi is not None:
                assert got_multi[f * K + k].tobytes() == wm.tobytes(), (f, k, len(cloud))
            if got_single is not None:
                assert got_single[f * K + k].tobytes() == ws.tobytes(), (f, k, len(cloud))


def test_one_call_rasters_ragged_frames_bit_identically():
    frames = _ragged_frames()
    p = _p()
    want = {(f, 0): _want(p, c) for f, c in enumerate(frames)}
    ctx = bev_amd.BevContext(p, device=0, max_batch=4, max_points=p.slots)
    try:
        for multi, single in ((True, True), (True, False), (False, True)):
            gm, gs = _call(ctx, frames, None, multi, single)
            assert (gm is not None) == multi and (gs is not None) == single
            _check(p, frames, None, gm, gs, want)
            for f, cloud in enumerate(frames):
                if len(cloud) == 0:
                    assert (gm is None or not gm[f].any()) and (gs is None or not gs[f].any()), f
            assert (gm is None or gm[-3].any()) and (gs is None or gs[-3].any())   # the full sweep
    finally:
        ctx.close()


def test_contention_and_exclusions():
    """every point of a frame in ONE cell: both atomics under contention; all 24 layers, heights outside the layers on both
    sides, both clamps; what must leave no trace (label 0), and non-finite heights"""
    rng = np.random.default_rng(5)
    plain = rng.permutation(np.linspace(-3.0, 5.0, 20000 - 14).astype(np.float32))     # layers 0 .. 22, and below layer 0
    special = np.array([np.nan, np.inf, -np.inf, 70.0, 3.0e38, -3.0e38, 5.25, 5.6], dtype=np.float32)   # (5.25: layer 23, 5.6: above it)
    ghosts = np.array([4.9, 61.0, 80.0, 5.6, -0.4, np.inf], dtype=np.float32)       # label 0
    zs = np.concatenate([plain[:7000], special, plain[7000:13000], ghosts, plain[13000:]])
    labels = np.ones(len(zs), dtype=np.int16)
    labels[7000 + 8 + 6000:7000 + 8 + 6000 + 6] = 0
    assert len(zs) == 20000 and (zs[labels == 0] == ghosts).all()
    low = plain[plain < 2.0]                                                         # layers 0 .. 10 only, heights up to 15
    low_labels = np.ones(len(low) + 6, dtype=np.int16)
    low_labels[100:106] = 0
    frames = [_one_cell(zs, labels),
              _one_cell(np.concatenate([low[:100], ghosts, low[100:]]), low_labels),  # the ghosts alone would reach layer 23 and 255
              _one_cell(np.concatenate([ghosts] * 50), 0),                            # nothing but label-0 points
              _one_cell(np.full(4096, 1.625, np.float32)),
              _one_cell(np.array([np.nan, -np.inf, -3.0e38] * 40, dtype=np.float32))]  # a cell that is hit but stays 0 everywhere
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        gm, gs = _call(ctx, frames)
        _check(p, frames, None, gm, gs)
        assert [int(np.count_nonzero(g)) for g in gs] == [1, 1, 0, 1, 0]
        assert [int(g.max()) for g in gs] == [255, 15, 0, 14, 0]
        assert [int(np.count_nonzero(g)) for g in gm] == [24, 11, 0, 1, 0]             # layers of the one cell
    finally:
        ctx.close()


def _every_cell_cloud(height_res=0.25):
    """tests/posedcheck's cloud: one point at the centre of every cell of the 224 x 224 grid, z through the centres of layers
    -2 .. 26, every 37th point with label 0"""
    i = np.arange(224 * 224)
    cloud = np.zeros(len(i), dtype=POINT_DTYPE)
    cloud["x"], cloud["y"] = (i // 224).astype(np.float32) - np.float32(112.5), (i % 224).astype(np.float32) - np.float32(112.5)
    cloud["z"] = ((i % 29) - 4).astype(np.float32) * np.float32(height_res)
    cloud["label"] = np.where(i % 37 == 0, 0, 1)
    return cloud


def test_every_cell_and_every_band_edge():
    p = _p()
    cloud = _every_cell_cloud(p.height_res)
    poses = np.stack([_matrix((1.0, 0, 0, 0)), _matrix((-1.0, 0, 0, 0)), _matrix((0, 0, 0, 90))])[None]
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        gm, gs = _call(ctx, [cloud])
        _check(p, [cloud], None, gm, gs)
        hit = np.ones(224 * 224, bool)
        hit[::37] = False                                              # label 0: no trace
        assert np.array_equal(gs[0] > 0, hit.reshape(224, 224))        # every other cell holds its own point's height
        assert gm[0].any(axis=(1, 2)).all()                            # ... and every layer is reached
        pm, ps = _call(ctx, [cloud], poses)
        _check(p, [cloud], poses, pm, ps)
        # a whole row further: image row r of the raw cloud is row r + 1 / r - 1, the first / last row leaves the grid
        assert np.array_equal(ps[0][1:], gs[0][:-1]) and not ps[0][0].any()
        assert np.array_equal(ps[1][:-1], gs[0][1:]) and not ps[1][-1].any()
        assert np.array_equal(pm[0][:, 1:], gm[0][:, :-1]) and np.array_equal(pm[1][:, :-1], gm[0][:, 1:])
    finally:
        ctx.close()


def _nonfinite_cloud():
    """the non-finite adversarial cloud plus points whose z is not finite while x and y are on the grid"""
    extra = np.zeros(4, dtype=POINT_DTYPE)
    extra["x"], extra["y"], extra["label"] = [1.0, 2.0, -3.0, 4.0], [1.0, -2.0, 3.0, 4.5], 1
    extra["z"] = [np.inf, np.inf, np.nan, -np.inf]
    return np.concatenate([_adversarial()[:30000], extra])


def test_poses():
    adv, marked = _adversarial(), _marked()
    frames = [marked[:50001], adv[:0], _nonfinite_cloud(), marked[60000:60257], adv[100:1125], marked[90000:133312]]
    nf, n_poses = len(frames), 6
    # (the last pose is a general matrix: every cloud, the non-finite one too, meets m[2], m[6], m[8], m[9] != 0)
    poses = np.stack([np.stack([_matrix((POSES + POSES)[f + k][:3] + (POSES[k][3] + f,)) for k in range(4)] + [_matrix(FAR), GENERAL])
                      for f in range(nf)])
    assert (np.abs(poses[:, 5]) > 0.01).all() and not (poses[:, :5, [2, 6, 8, 9]] != 0).any()
    assert poses.shape == (nf, n_poses, 12)
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        gm, gs = _call(ctx, frames, poses)
        _check(p, frames, poses, gm, gs)
        assert gs[0].any() and np.count_nonzero(gs[4]) < np.count_nonzero(gs[0]) // 2   # FAR pushes most points off the grid
        assert not gm[n_poses:2 * n_poses].any() and not gs[n_poses:2 * n_poses].any()   # the empty frame

        # the most poses a call takes, and one pose, on a frame that does not fill its last workgroup
        cloud = marked[20000:24097]
        rng = np.random.default_rng(2)
        many = np.stack([_matrix((rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(-1, 1), rng.uniform(-180, 180)))
                         for _ in range(POSED_BEV_MAX_POSES)])[None]
        for ps in (many, many[:, 7:8]):
            gm, gs = _call(ctx, [cloud], ps)
            _check(p, [cloud], ps, gm, gs)

        # no poses and the identity pose: each is its own oracle's
        cloud = _nonfinite_cloud()
        identity = _matrix((0, 0, 0, 0))
        assert np.array_equal(identity, np.eye(3, 4, dtype=np.float32).reshape(12))
        gm, gs = _call(ctx, [cloud])
        _check(p, [cloud], None, gm, gs)
        gm, gs = _call(ctx, [cloud], identity[None, None])
        _check(p, [cloud], identity[None, None], gm, gs)
    finally:
        ctx.close()


def test_launch_groups_do_not_change_the_bytes():
    """BEV_POSED_GROUP=3: a frame's five grids exceed the cap, every frame is a group of its own; 12: two frames per group,
    the last group has one; default: one group.  The launch counts of the profiling slots show that the variable was read."""
    adv, marked = _adversarial(), _marked()
    frames = [marked[:9000], adv[:5000], adv[:0], marked[70000:70257], adv[7:4104], marked[40000:52000], adv[20000:23000]]
    poses = np.stack([np.stack([_matrix(POSES[(f + k) % 5]) for k in range(4)] + [_matrix(FAR)]) for f in range(7)])
    p = _p()
    got, launches = {}, {}
    saved = os.environ.get("BEV_POSED_GROUP")
    try:
        for group in ("3", None, "12"):
            if group is None:
                os.environ.pop("BEV_POSED_GROUP", None)
            else:
                os.environ["BEV_POSED_GROUP"] = group
            ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
            try:
                ctx.profile_reset()
                ctx.profile_enable(True)
                got[group] = _call(ctx, frames, poses)
                launches[group] = {k["name"]: k["launches"] for k in ctx.profile_get()}
            finally:
                ctx.close()
    finally:
        if saved is None:
            os.environ.pop("BEV_POSED_GROUP", None)
        else:
            os.environ["BEV_POSED_GROUP"] = saved
    # (the expand pass runs for every group, the splat's launch is left out for a group without points: frame 2 under "3")
    assert [launches[g]["k_posed_expand"] for g in ("3", "12", None)] == [7, 4, 1], launches
    _check(p, frames, poses, *got[None])
    for group in ("3", "12"):
        assert got[group][0].tobytes() == got[None][0].tobytes() and got[group][1].tobytes() == got[None][1].tobytes(), group


@pytest.mark.parametrize("sensor,interval", [("OS1_64", 1.0), ("HDL_32E", 1.0), ("HDL_64E", 2.0)])
def test_sensors_and_interval(sensor, interval):
    p = bev_amd.params_for_sensor(sensor)
    p.interval = interval
    assert p.mat_size == {1.0: 224, 2.0: 112}[interval]
    sp = orc.sensor_from_params(p)
    full = orc.mark_ground(sp, orc.order_cloud(sp, synth.sweep(p, 5)))[0]
    frames = [full, synth.sweep(p, 6)[:20001], _adversarial()[:3000]]
    poses = np.stack([np.stack([_matrix(POSES[1 + f]), _matrix((0.5, -1.0, 0.25, 90 + f))]) for f in range(3)])
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        assert ctx.M == p.mat_size
        for ps in (None, poses):
            gm, gs = _call(ctx, frames, ps)
            _check(p, frames, ps, gm, gs)
            assert gm[0].any() and gs[0].any()
    finally:
        ctx.close()


def test_stream_ordering_with_the_bev_path():
    """process_device, then posed_bev_device without poses on its d_ordered with nothing between them while the default stream
    is busy: the images are those process_device wrote in the same run; then posed_bev_device followed at once by a
    process_device that overwrites d_ordered; then two posed_bev_device calls of different sizes back to back."""
    p = _p()
    sp = orc.sensor_from_params(p)
    S = p.slots
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
        g1, g2 = _Out(p, nf), _Out(p, nf)
        busy = torch.randn(4096, 4096, device=dev)
        torch.cuda.synchronize()
        for _ in range(4):   # the default stream is busy when the library is called: the fill below is still queued
            busy = busy @ busy * 1e-3
        d_pts.copy_(src1)
        ctx.process_device(nf, d_pts.data_ptr(), o1, d_ordered.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
        ctx.posed_bev_device(nf, d_ordered.data_ptr(), offs_s, *g1.ptrs())
        ctx.synchronize()
        gm, gs = g1.images()
        assert gm.tobytes() == d_multi.cpu().numpy().tobytes() and gs.tobytes() == d_single.cpu().numpy().tobytes()
        _check(p, want["first"], None, gm, gs)

        # reverse order: the splat still reads d_ordered when the pipeline that overwrites it is issued
        ctx.posed_bev_device(nf, d_ordered.data_ptr(), offs_s, *g2.ptrs())
        ctx.process_device(nf, d_other.data_ptr(), o2, d_ordered.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
        ctx.synchronize()
        got_ordered = d_ordered.cpu().numpy().view(POINT_DTYPE).reshape(nf, S)
        assert g2.images()[0].tobytes() == gm.tobytes() and g2.images()[1].tobytes() == gs.tobytes()
        for f in range(nf):
            assert got_ordered[f].tobytes() == want["other"][f].tobytes(), f
        assert g1.guards_ok() and g2.guards_ok()

        # two calls of different sizes back to back: the second call's table and planes follow the first call's launches
        frames = _ragged_frames()[4:11]
        ox, flatx = _pack(frames)
        d_x = _dev(flatx)
        poses = np.stack([np.stack([_matrix(POSES[1]), _matrix(POSES[(f % 3) + 2])]) for f in range(nf)])
        ga, gb = _Out(p, nf * 2), _Out(p, len(frames))
        torch.cuda.synchronize()
        ctx.posed_bev_device(nf, d_ordered.data_ptr(), offs_s, *ga.ptrs(), poses=poses)
        ctx.posed_bev_device(len(frames), d_x.data_ptr(), ox, *gb.ptrs())
        ctx.synchronize()
        _check(p, want["other"], poses, *ga.images())
        _check(p, frames, None, *gb.images())
        assert ga.guards_ok() and gb.guards_ok()
    finally:
        ctx.close()


def test_status_codes():
    p = _p()
    C = bev_amd.C
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=1000)   # frames of up to max(max_points, S) = S records
    try:
        frames = [_marked()[:3000], _marked()[3000:8000]]
        offs, flat = _pack(frames)
        d_in, out = _dev(flat), _Out(p, 2 * 2)
        pose = np.ascontiguousarray(np.stack([_matrix(POSES[1])] * 4).reshape(2, 2, 12))
        torch.cuda.synchronize()
        L = ctx.lib
        u64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64)) if a is not None else None
        fp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        dm, ds = out.ptrs()

        def call(h=ctx._h, n=2, din=d_in.data_ptr(), o=offs, n_poses=0, poses=None, multi=dm, single=ds):
            return L.bev_posed_bev_device_resident(h, n, din, u64p(o), n_poses, fp(poses), multi, single)

        assert call(h=None) == INVALID
        assert call(n=-1) == INVALID
        assert call(o=None) == INVALID
        assert call(o=np.array([0, 5000, 3000], dtype=np.uint64)) == INVALID          # decreasing offsets
        assert call(n_poses=-1, poses=pose) == INVALID
        assert call(n_poses=POSED_BEV_MAX_POSES + 1, poses=pose) == INVALID
        assert call(n_poses=2, poses=None) == INVALID
        assert call(din=None) == INVALID                                              # NULL clouds with records to read
        assert call(multi=None, single=None) == INVALID                               # neither output wanted
        assert call(multi=None, single=None, o=np.zeros(3, dtype=np.uint64)) == INVALID
        assert call(n=1, o=np.array([0, p.slots + 1], dtype=np.uint64)) == TOO_LARGE  # a frame above max(max_points, S)
        assert call(n=0, o=offs[:1].copy(), din=None, multi=None, single=None) == 0   # nothing to do
        ctx.synchronize()
        assert out.untouched(), "a refused call wrote to its outputs"

        # the host-buffer call refuses the same things
        cl = (C.c_void_p * 2)(*[f.ctypes.data for f in frames])
        n_pts = (C.c_uint32 * 2)(3000, 5000)
        hm = np.full((2, 2, p.n_layers, p.mat_size, p.mat_size), PATTERN, dtype=np.uint8)
        hs = np.full((2, 2, p.mat_size, p.mat_size), PATTERN, dtype=np.uint8)
        mo = (C.c_void_p * 2)(*[hm[i].ctypes.data for i in range(2)])
        so = (C.c_void_p * 2)(*[hs[i].ctypes.data for i in range(2)])

        def hcall(h=ctx._h, n=2, clouds=cl, npts=n_pts, n_poses=0, poses=None, multi=mo, single=so):
            return L.bev_posed_bev_batch(h, n, clouds, npts, n_poses, fp(poses), multi, single)

        assert hcall(h=None) == INVALID and hcall(n=-1) == INVALID
        assert hcall(clouds=None) == INVALID and hcall(npts=None) == INVALID and hcall(multi=None, single=None) == INVALID
        assert hcall(clouds=(C.c_void_p * 2)(frames[0].ctypes.data, None)) == INVALID
        assert hcall(multi=(C.c_void_p * 2)(hm[0].ctypes.data, None)) == INVALID
        assert hcall(single=(C.c_void_p * 2)(hs[0].ctypes.data, None)) == INVALID
        assert hcall(n_poses=-1, poses=pose) == INVALID
        assert hcall(n_poses=POSED_BEV_MAX_POSES + 1, poses=pose) == INVALID and hcall(n_poses=1, poses=None) == INVALID
        assert hcall(npts=(C.c_uint32 * 2)(3000, p.slots + 1)) == TOO_LARGE
        assert hcall(n=0, clouds=None, npts=None, multi=None, single=None) == 0
        assert (hm == PATTERN).all() and (hs == PATTERN).all(), "a refused call wrote to its outputs"

        # valid calls still work
        assert call(n_poses=2, poses=pose) == 0
        ctx.synchronize()
        gm, gs = out.images()
        _check(p, frames, pose, gm, gs)
        assert out.guards_ok()
        assert hcall(n_poses=2, poses=pose) == 0
        assert hm.tobytes() == gm.tobytes() and hs.tobytes() == gs.tobytes()
        hs[:] = PATTERN
        assert hcall(n_poses=2, poses=pose, multi=None) == 0                          # one output alone
        assert hs.tobytes() == gs.tobytes()
    finally:
        ctx.close()


def test_host_buffers_in_chunks():
    """7 frames through a context of max_batch 2: four chunks; against the oracle and the per-cloud entry points"""
    adv, marked = _adversarial(), _marked()
    frames = [marked, adv[:40000], adv[:0], marked[5000:5257], adv[7:1032], marked[:100000], adv[20000:60000]]
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        multi, single = ctx.posed_bev_batch(frames)
        assert multi.shape == (7, 1, 24, 224, 224) and single.shape == (7, 1, 224, 224)
        _check(p, frames, None, multi.reshape(7, 24, 224, 224), single.reshape(7, 224, 224))
        for f, cloud in enumerate(frames):
            assert multi[f, 0].tobytes() == ctx.multi_bev(cloud).tobytes(), f
            assert single[f, 0].tobytes() == ctx.single_bev(cloud).tobytes(), f
        poses = np.stack([np.stack([_matrix(POSES[(f + k) % 5]) for k in range(2)] + [_matrix(FAR)]) for f in range(7)])
        multi, single = ctx.posed_bev_batch(frames, poses=poses)
        assert multi.shape == (7, 3, 24, 224, 224) and single.shape == (7, 3, 224, 224)
        _check(p, frames, poses, multi.reshape(21, 24, 224, 224), single.reshape(21, 224, 224))
        for f, cloud in enumerate(frames):
            for k in range(3):
                moved = ctx.transform_cloud(cloud, poses[f, k])
                assert multi[f, k].tobytes() == ctx.multi_bev(moved).tobytes(), (f, k)
                assert single[f, k].tobytes() == ctx.single_bev(moved).tobytes(), (f, k)
        only_multi, none = ctx.posed_bev_batch(frames[:3], want_single=False)   # a smaller call behind a larger one
        assert none is None
        _check(p, frames[:3], None, only_multi.reshape(3, 24, 224, 224), None)
        multi, single = ctx.posed_bev_batch([])
        assert multi.shape == (0, 1, 24, 224, 224) and single.shape == (0, 1, 224, 224)
    finally:
        ctx.close()
