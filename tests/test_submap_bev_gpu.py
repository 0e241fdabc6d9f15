"""GPU: the 24-layer occupancy BEV and the uint8 max-height BEV of submaps — windows of frames, each under its own pose, rastered
into one grid per map (bev_submap_bev_device_resident, bev_submap_bev_batch).  The checker is the oracle's
composition: multi_bev / single_bev of the concatenation of transform_cloud(frame, pose) over a map's entries; and, where
noted, the posed call of the same context.  Every comparison is of bytes."""
import functools
import os

import numpy as np
import pytest
import torch

import bev_amd
import oracle_lib as orc
import packed_cases
from bev_amd import POINT_DTYPE, SUBMAP_MAX_ENTRIES, synth
from packed_cases import (FAR, GENERAL, INVALID, PATTERN, POSES, TOO_LARGE, _adversarial, _dev, _marked, _matrix, _one_cell, _Out, _p,
                          _pack)

pytestmark = pytest.mark.gpu
_ragged_frames = functools.partial(packed_cases._ragged_frames, 4, 18)

IDENTITY = np.eye(3, 4, dtype=np.float32).reshape(12)


def _entries(maps):
    """maps: per map a list of (frame, matrix) -> (map_offsets, entry_frame, entry_pose)"""
    offs = np.zeros(len(maps) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(m) for m in maps])
    frame = np.array([f for m in maps for f, _ in m], dtype=np.int32)
    pose = np.array([mat for m in maps for _, mat in m], dtype=np.float32).reshape(-1, 12)
    return offs, frame, pose


def _want(p, frames, entries):
    """(multi, single) of the oracle for one map: the rasters of its entries' moved clouds, concatenated"""
    moved = [orc.transform_cloud(np.ascontiguousarray(frames[f]), m) for f, m in entries]
    cloud = np.concatenate(moved) if moved else np.empty(0, POINT_DTYPE)
    return orc.multi_bev(orc.sensor_from_params(p), cloud, p.interval), orc.single_bev(cloud, p.interval)


def _call(ctx, frames, maps, multi=True, single=True):
    """one bev_submap_bev_device_resident call; returns the images (maps, ...) after the guards were checked"""
    offs, flat = _pack(frames)
    d_in, out = _dev(flat), _Out(ctx.params, len(maps), multi, single)
    torch.cuda.synchronize()
    ctx.submap_bev_device(len(frames), d_in.data_ptr(), offs, *_entries(maps), *out.ptrs())
    ctx.synchronize()
    assert out.guards_ok(), "something was written behind an output"
    return out.images()


def _check(p, frames, maps, got_multi, got_single, want=None):
    for g, entries in enumerate(maps):
        wm, ws = want[g] if want is not None else _want(p, frames, entries)
        if got_multi is not None:
            assert got_multi[g].tobytes() == wm.tobytes(), (g, len(entries))
        if got_single is not None:
            assert got_single[g].tobytes() == ws.tobytes(), (g, len(entries))


def test_maps_over_ragged_frames():
    frames = _ragged_frames()
    nf = len(frames)
    order = np.random.default_rng(3).permutation(nf)
    assert list(order) != sorted(order)
    maps = [[],
            [(10, _matrix(POSES[1]))],
            [(16, _matrix(POSES[2])), (17, _matrix(POSES[3]))],                                  # the two empty frames only
            [(int(f), _matrix((0.5 * f - 5, 3 - 0.25 * f, 0.01 * f, 7.0 * f))) for f in order],  # every frame once
            [(12, _matrix(POSES[1])), (12, _matrix(POSES[3])), (12, _matrix(POSES[4]))],         # one frame three times
            [(15, _matrix(FAR)), (6, _matrix(POSES[2]))],                                        # the full sweep, far off
            [(15, GENERAL), (12, GENERAL), (4, _matrix(POSES[1])), (11, GENERAL)]]               # a general matrix: m[2], m[6], m[8], m[9] != 0
    p = _p()
    want = [_want(p, frames, m) for m in maps]
    assert not want[0][0].any() and not want[2][1].any() and want[5][1].any() and want[6][0].any() and want[6][1].any()
    # the union really is one: map 4's image is not any single entry's
    assert want[4][1].tobytes() != _want(p, frames, maps[4][:1])[1].tobytes()
    ctx = bev_amd.BevContext(p, device=0, max_batch=4, max_points=p.slots)
    try:
        for multi, single in ((True, True), (True, False), (False, True)):
            gm, gs = _call(ctx, frames, maps, multi, single)
            assert (gm is not None) == multi and (gs is not None) == single
            _check(p, frames, maps, gm, gs, want)
    finally:
        ctx.close()


def test_one_entry_per_map_is_the_posed_call():
    adv, marked = _adversarial(), _marked()
    frames = [marked[:9000], adv[:0], adv[100:1125], marked[60000:60257], adv[7:4104]]
    nf, K = len(frames), 3
    poses = np.stack([np.stack([_matrix(POSES[(f + k) % 5]) for k in range(2)] + [_matrix(FAR)]) for f in range(nf)])
    maps = [[(f, poses[f, k])] for f in range(nf) for k in range(K)]
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        gm, gs = _call(ctx, frames, maps)
        offs, flat = _pack(frames)
        d_in, out = _dev(flat), _Out(p, nf * K)
        torch.cuda.synchronize()
        ctx.posed_bev_device(nf, d_in.data_ptr(), offs, *out.ptrs(), poses=poses)
        ctx.synchronize()
        pm, ps = out.images()
        assert gm.tobytes() == pm.tobytes() and gs.tobytes() == ps.tobytes()
        assert gs[0].any() and not gs[K:2 * K].any()
    finally:
        ctx.close()


def _windows(n, h, pose_of):
    """sliding windows of half width h at stride 1 over n frames: map i = frames i - h .. i + h under pose_of(j - i)"""
    return [[(j, pose_of(j - i)) for j in range(max(0, i - h), min(n - 1, i + h) + 1)] for i in range(n)]


def test_sliding_windows_and_launch_groups():
    """12 maps of up to 5 frames; BEV_POSED_GROUP 1, 5 and unset: 12, 3 and 1 launch groups, the same bytes"""
    adv, marked = _adversarial(), _marked()
    sizes = [257, 12000, 3000, 1025, 7000, 4097, 900, 11000, 2048, 5000, 1024, 8000]
    frames = [(marked if i % 2 else adv)[3000 * i:3000 * i + n] for i, n in enumerate(sizes)]
    maps = _windows(12, 2, lambda d: IDENTITY if d == 0 else _matrix((2.0 * d, 0.3 * d, 0.0, 1.0 * d)))
    assert len(maps) == 12 and sum(len(m) for m in maps) == 54
    p = _p()
    got, launches = {}, {}
    saved = os.environ.get("BEV_POSED_GROUP")
    try:
        for group in ("1", "5", None):
            if group is None:
                os.environ.pop("BEV_POSED_GROUP", None)
            else:
                os.environ["BEV_POSED_GROUP"] = group
            ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
            try:
                ctx.profile_reset()
                ctx.profile_enable(True)
                got[group] = _call(ctx, frames, maps)
                launches[group] = {k["name"]: k["launches"] for k in ctx.profile_get()}
            finally:
                ctx.close()
    finally:
        if saved is None:
            os.environ.pop("BEV_POSED_GROUP", None)
        else:
            os.environ["BEV_POSED_GROUP"] = saved
    assert [launches[g]["k_posed_expand"] for g in ("1", "5", None)] == [12, 3, 1], launches
    assert [launches[g]["k_submap_splat"] for g in ("1", "5", None)] == [12, 3, 1], launches
    _check(p, frames, maps, *got[None])
    for group in ("1", "5"):
        assert got[group][0].tobytes() == got[None][0].tobytes() and got[group][1].tobytes() == got[None][1].tobytes(), group


def test_long_entry_lists():
    """a frame feeding 150 one-entry maps, and one map of 150 entries of one frame: both past the posed call's 64 poses"""
    marked = _marked()
    frames = [marked[20000:24097], marked[60000:60257]]
    rng = np.random.default_rng(2)
    mats = [_matrix((rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(-1, 1), rng.uniform(-180, 180))) for _ in range(150)]
    maps = [[(0, m)] for m in mats] + [[(1, m) for m in mats]]
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        gm, gs = _call(ctx, frames, maps)
        _check(p, frames, maps, gm, gs)
        assert gs[0].any() and gs[149].any() and gs[150].any()
    finally:
        ctx.close()


def test_contention_across_frames_and_exclusions():
    """five frames whose points all lie in ONE cell, in one map: both atomics under contention within and across frames.  The
    frames that must leave no trace (label 0; heights that are not finite or far below) are shifted by 5 m: their cell stays
    empty."""
    rng = np.random.default_rng(5)
    plain = rng.permutation(np.linspace(-3.0, 5.0, 20000 - 14).astype(np.float32))     # layers 0 .. 22, and below layer 0
    special = np.array([70.0, 3.0e38, -3.0e38, 5.25, 5.6], dtype=np.float32)           # (5.25: layer 23, 5.6: above it)
    ghosts = np.array([4.9, 61.0, 80.0, 5.6, -0.4, np.inf], dtype=np.float32)          # label 0
    low = plain[plain < 2.0]                                                           # layers 0 .. 10 only
    frames = [_one_cell(plain[:9000]),
              _one_cell(np.concatenate([low[:100], ghosts, low[100:]]), np.r_[np.ones(100), np.zeros(6), np.ones(len(low) - 100)].astype(np.int16)),
              _one_cell(np.concatenate([ghosts] * 50), 0),                                   # nothing but label-0 points
              _one_cell(np.concatenate([plain[9000:], special])),
              _one_cell(np.array([np.nan, -np.inf, np.inf, -3.0e38] * 40, dtype=np.float32))]  # not finite, or clamped to 0 below every layer
    shift = _matrix((5, 0, 0, 0))
    maps = [[(0, IDENTITY), (1, IDENTITY), (2, shift), (3, IDENTITY), (4, shift)],
            [(1, IDENTITY)]]
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        gm, gs = _call(ctx, frames, maps)
        _check(p, frames, maps, gm, gs)
        assert [int(np.count_nonzero(g)) for g in gs] == [1, 1]
        assert [int(g.max()) for g in gs] == [255, 15]
        assert [int(np.count_nonzero(g)) for g in gm] == [24, 11]              # the layers of the one cell
    finally:
        ctx.close()


@pytest.mark.parametrize("sensor,interval", [("OS1_64", 1.0), ("HDL_32E", 1.0), ("HDL_64E", 2.0)])
def test_sensors_and_interval(sensor, interval):
    p = bev_amd.params_for_sensor(sensor)
    p.interval = interval
    assert p.mat_size == {1.0: 224, 2.0: 112}[interval]
    sp = orc.sensor_from_params(p)
    full = orc.mark_ground(sp, orc.order_cloud(sp, synth.sweep(p, 5)))[0]
    frames = [full, synth.sweep(p, 6)[:20001], _adversarial()[:3000]]
    maps = [[(0, IDENTITY), (1, _matrix(POSES[1])), (2, _matrix(POSES[2]))], [(2, _matrix((0.5, -1.0, 0.25, 91)))], []]
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        assert ctx.M == p.mat_size
        gm, gs = _call(ctx, frames, maps)
        _check(p, frames, maps, gm, gs)
        assert gm[0].any() and gs[0].any() and not gs[2].any()
    finally:
        ctx.close()


def test_stream_ordering_with_the_bev_path():
    """process_device, then the submap call on its d_ordered with nothing between them while the default stream is busy; then
    the submap call followed at once by a process_device that overwrites d_ordered"""
    p = _p()
    sp = orc.sensor_from_params(p)
    S = p.slots
    dev = torch.device("cuda:0")
    first = [synth.sweep(p, 30), synth.sweep(p, 31)[:70000], synth.adversarial(p, 20000, 4)]
    other = [synth.sweep(p, 32)[:90000], synth.adversarial(p, 30000, 6), synth.sweep(p, 33)]
    nf = len(first)
    want = {k: [orc.mark_ground(sp, orc.order_cloud(sp, c))[0] for c in fs] for k, fs in (("first", first), ("other", other))}
    offs_s = np.arange(nf + 1, dtype=np.uint64) * np.uint64(S)
    maps = [[(0, IDENTITY), (1, _matrix(POSES[1])), (2, _matrix(POSES[2]))], [(1, IDENTITY)], [(2, _matrix(POSES[4])), (0, _matrix(POSES[3]))]]
    want_maps = [_want(p, want["first"], m) for m in maps]
    ctx = bev_amd.BevContext(p, device=0, max_batch=4, max_points=S + 8192)
    try:
        (o1, flat1), (o2, flat2) = _pack(first), _pack(other)
        src1, d_other = _dev(flat1), _dev(flat2)
        d_pts = torch.zeros_like(src1)
        d_ordered = torch.zeros(nf * S * 32, dtype=torch.uint8, device=dev)
        d_multi = torch.zeros(nf * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device=dev)
        d_single = torch.zeros(nf * p.mat_size ** 2, dtype=torch.uint8, device=dev)
        g1, g2 = _Out(p, len(maps)), _Out(p, len(maps))
        busy = torch.randn(4096, 4096, device=dev)
        torch.cuda.synchronize()
        for _ in range(4):   # the default stream is busy when the library is called: the fill below is still queued
            busy = busy @ busy * 1e-3
        d_pts.copy_(src1)
        ctx.process_device(nf, d_pts.data_ptr(), o1, d_ordered.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
        ctx.submap_bev_device(nf, d_ordered.data_ptr(), offs_s, *_entries(maps), *g1.ptrs())
        ctx.synchronize()
        _check(p, want["first"], maps, *g1.images(), want_maps)

        # reverse order: the splat still reads d_ordered when the pipeline that overwrites it is issued
        ctx.submap_bev_device(nf, d_ordered.data_ptr(), offs_s, *_entries(maps), *g2.ptrs())
        ctx.process_device(nf, d_other.data_ptr(), o2, d_ordered.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
        ctx.synchronize()
        got_ordered = d_ordered.cpu().numpy().view(POINT_DTYPE).reshape(nf, S)
        _check(p, want["first"], maps, *g2.images(), want_maps)
        for f in range(nf):
            assert got_ordered[f].tobytes() == want["other"][f].tobytes(), f
        assert g1.guards_ok() and g2.guards_ok()
    finally:
        ctx.close()


def test_status_codes():
    p = _p()
    C = bev_amd.C
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=1000)   # frames of up to max(max_points, S) = S records
    try:
        frames = [_marked()[:3000], _marked()[3000:8000]]
        offs, flat = _pack(frames)
        maps = [[(0, _matrix(POSES[1])), (1, _matrix(POSES[2]))], [(1, IDENTITY)]]
        moffs, eframe, epose = _entries(maps)
        d_in, out = _dev(flat), _Out(p, 2)
        torch.cuda.synchronize()
        L = ctx.lib
        u64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64)) if a is not None else None
        vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        dm, ds = out.ptrs()
        bad_frame, neg_frame = eframe.copy(), eframe.copy()
        bad_frame[2], neg_frame[0] = 2, -1
        many = np.array([0, SUBMAP_MAX_ENTRIES + 1], dtype=np.uint64)         # real arrays of that length
        many_frame = np.zeros(SUBMAP_MAX_ENTRIES + 1, dtype=np.int32)
        many_pose = np.tile(IDENTITY, (SUBMAP_MAX_ENTRIES + 1, 1))

        def call(h=ctx._h, n=2, din=d_in.data_ptr(), o=offs, n_maps=2, mo=moffs, ef=eframe, ep=epose, multi=dm, single=ds):
            return L.bev_submap_bev_device_resident(h, n, din, u64p(o), n_maps, u64p(mo), vp(ef), vp(ep), multi, single)

        assert call(h=None) == INVALID
        assert call(n=-1) == INVALID and call(n_maps=-1) == INVALID
        assert call(o=None) == INVALID and call(mo=None) == INVALID
        assert call(o=np.array([0, 5000, 3000], dtype=np.uint64)) == INVALID          # decreasing frame offsets
        assert call(mo=np.array([0, 3, 2], dtype=np.uint64)) == INVALID               # decreasing map offsets
        assert call(ef=None) == INVALID and call(ep=None) == INVALID                  # entries, but no entry array
        assert call(ef=bad_frame) == INVALID and call(ef=neg_frame) == INVALID        # an entry frame outside 0 .. n_frames - 1
        assert call(din=None) == INVALID                                              # NULL clouds with records to read
        assert call(multi=None, single=None) == INVALID                               # neither output wanted
        assert call(n=1, o=np.array([0, p.slots + 1], dtype=np.uint64), n_maps=1, mo=np.array([0, 1], dtype=np.uint64)) == TOO_LARGE
        assert call(n_maps=1, mo=many, ef=many_frame, ep=many_pose) == TOO_LARGE
        assert call(n_maps=1, mo=many, ef=None, ep=None) == TOO_LARGE                 # the count is checked before the arrays are read
        assert call(n_maps=0, mo=moffs[:1].copy(), ef=None, ep=None, multi=None, single=None) == 0   # nothing to do
        ctx.synchronize()
        assert out.untouched(), "a refused call wrote to its outputs"

        # the host-buffer call refuses the same things
        cl = (C.c_void_p * 2)(*[f.ctypes.data for f in frames])
        n_pts = (C.c_uint32 * 2)(3000, 5000)
        hm = np.full((2, p.n_layers, p.mat_size, p.mat_size), PATTERN, dtype=np.uint8)
        hs = np.full((2, p.mat_size, p.mat_size), PATTERN, dtype=np.uint8)
        mo_ = (C.c_void_p * 2)(*[hm[i].ctypes.data for i in range(2)])
        so_ = (C.c_void_p * 2)(*[hs[i].ctypes.data for i in range(2)])

        def hcall(h=ctx._h, n=2, clouds=cl, npts=n_pts, n_maps=2, mo=moffs, ef=eframe, ep=epose, multi=mo_, single=so_):
            return L.bev_submap_bev_batch(h, n, clouds, npts, n_maps, u64p(mo), vp(ef), vp(ep), multi, single)

        assert hcall(h=None) == INVALID and hcall(n=-1) == INVALID and hcall(n_maps=-1) == INVALID
        assert hcall(clouds=None) == INVALID and hcall(npts=None) == INVALID and hcall(multi=None, single=None) == INVALID
        assert hcall(clouds=(C.c_void_p * 2)(frames[0].ctypes.data, None)) == INVALID
        assert hcall(multi=(C.c_void_p * 2)(hm[0].ctypes.data, None)) == INVALID
        assert hcall(single=(C.c_void_p * 2)(hs[0].ctypes.data, None)) == INVALID
        assert hcall(mo=None) == INVALID and hcall(mo=np.array([0, 3, 2], dtype=np.uint64)) == INVALID
        assert hcall(ef=None) == INVALID and hcall(ep=None) == INVALID
        assert hcall(ef=bad_frame) == INVALID and hcall(ef=neg_frame) == INVALID
        assert hcall(npts=(C.c_uint32 * 2)(3000, p.slots + 1)) == TOO_LARGE
        assert hcall(n_maps=1, mo=many, ef=many_frame, ep=many_pose) == TOO_LARGE
        assert hcall(n_maps=1, mo=many, ef=None, ep=None) == TOO_LARGE
        assert hcall(n_maps=0, mo=moffs[:1].copy(), ef=None, ep=None, multi=None, single=None) == 0
        assert (hm == PATTERN).all() and (hs == PATTERN).all(), "a refused call wrote to its outputs"

        # valid calls still work
        assert call() == 0
        ctx.synchronize()
        gm, gs = out.images()
        _check(p, frames, maps, gm, gs)
        assert out.guards_ok()
        assert hcall() == 0
        assert hm.tobytes() == gm.tobytes() and hs.tobytes() == gs.tobytes()
        hs[:] = PATTERN
        assert hcall(multi=None) == 0                                                 # one output alone
        assert hs.tobytes() == gs.tobytes()
    finally:
        ctx.close()


def test_host_buffers_in_chunks():
    """7 frames, 5 maps through a context of max_batch 2: three chunks of maps; map 1 names 5 distinct frames, which go through
    the staging in three pieces; against the device-resident call and the oracle"""
    adv, marked = _adversarial(), _marked()
    frames = [marked, adv[:40000], adv[:0], marked[5000:5257], adv[7:1032], marked[:100000], adv[20000:60000]]
    maps = [[(1, _matrix(POSES[1]))],
            [(6, _matrix(POSES[2])), (0, IDENTITY), (3, _matrix(POSES[3])), (4, _matrix(FAR)), (5, _matrix(POSES[4])), (3, _matrix(POSES[1]))],
            [],
            [(2, IDENTITY), (0, _matrix(POSES[2]))],
            [(5, _matrix(POSES[3])), (1, _matrix(POSES[0]))]]
    assert len({f for f, _ in maps[1]}) == 5
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        multi, single = ctx.submap_bev_batch(frames, *_entries(maps))
        assert multi.shape == (5, 24, 224, 224) and single.shape == (5, 224, 224)
        _check(p, frames, maps, multi, single)
        gm, gs = _call(ctx, frames, maps)
        assert multi.tobytes() == gm.tobytes() and single.tobytes() == gs.tobytes()
        only_multi, none = ctx.submap_bev_batch(frames, *_entries(maps[:2]), want_single=False)   # a smaller call behind a larger one
        assert none is None and only_multi.tobytes() == gm[:2].tobytes()
        multi, single = ctx.submap_bev_batch([], *_entries([]))
        assert multi.shape == (0, 24, 224, 224) and single.shape == (0, 224, 224)
    finally:
        ctx.close()
