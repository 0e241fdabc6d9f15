"""GPU: the float max-height BEV of submaps — windows of frames, each under its own pose, rastered into one grid per map
(bev_submap_float_bev_device_resident, bev_submap_float_bev_batch).  The checker is the oracle's composition:
float_bev of the concatenation of transform_cloud(frame, pose) over a map's entries; and, where noted, the float call of the
same context.  Every comparison is of bytes."""
import functools

import numpy as np
import pytest
import torch

import bev_amd
import oracle_lib as orc
import packed_cases
from bev_amd import POINT_DTYPE, SUBMAP_MAX_ENTRIES, synth
from packed_cases import (FAR, GUARD, INVALID, PATTERN, POSES, TOO_LARGE, UNSUPPORTED, _adversarial, _dev, _marked, _matrix,
                          _one_cell, _p, _pack)

pytestmark = pytest.mark.gpu
# frames of 0, 0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 4097, 63, 65 records, four of 3000 .. 40000, the full sweep, two empty
_ragged_frames = functools.partial(packed_cases._ragged_frames, 4, 20, (63, 65))

IDENTITY = np.eye(3, 4, dtype=np.float32).reshape(12)


def _entries(maps):
    """maps: per map a list of (frame, matrix) -> (map_offsets, entry_frame, entry_pose)"""
    offs = np.zeros(len(maps) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(m) for m in maps])
    frame = np.array([f for m in maps for f, _ in m], dtype=np.int32)
    pose = np.array([mat for m in maps for _, mat in m], dtype=np.float32).reshape(-1, 12)
    return offs, frame, pose


def _want(frames, entries, interval=1.0, skip=True):
    """the oracle's grid of one map: the float BEV of its entries' moved clouds, concatenated"""
    moved = [orc.transform_cloud(np.ascontiguousarray(frames[f]), m) for f, m in entries]
    return orc.float_bev(np.concatenate(moved) if moved else np.empty(0, POINT_DTYPE), interval, skip)


def _out(n_grids, M):
    return torch.full((n_grids * M * M * 4 + GUARD,), PATTERN, dtype=torch.uint8, device=torch.device("cuda:0"))


def _grids(t, n_grids, M):
    return t[:n_grids * M * M * 4].cpu().numpy().view(np.float32).reshape(n_grids, M, M)


def _guard_ok(t, n_grids, M):
    return bool((t[n_grids * M * M * 4:] == PATTERN).all())


def _call(ctx, frames, maps, interval=1.0, skip=True):
    """one bev_submap_float_bev_device_resident call; returns the grids (maps, M, M) after the guard was checked"""
    offs, flat = _pack(frames)
    M = int(ctx.lib.bev_float_bev_size(interval))
    d_in, d_out = _dev(flat), _out(len(maps), M)
    torch.cuda.synchronize()
    ctx.submap_float_bev_device(len(frames), d_in.data_ptr(), offs, *_entries(maps), d_out.data_ptr(), interval, skip)
    ctx.synchronize()
    assert _guard_ok(d_out, len(maps), M), "something was written behind d_out"
    return _grids(d_out, len(maps), M)


def _check(frames, maps, got, interval=1.0, skip=True, want=None):
    for g, entries in enumerate(maps):
        w = want[g] if want is not None else _want(frames, entries, interval, skip)
        assert got[g].tobytes() == w.tobytes(), (g, len(entries))


@pytest.mark.parametrize("interval,skip", [(1.0, 1), (2.0, 0), (0.5, 1)])
def test_maps_over_ragged_frames(interval, skip):
    frames = _ragged_frames()
    nf = len(frames)
    assert sorted({len(f) for f in frames} & {0, 1, 63, 65, 257, 1023, 1025, 4097, 133312}) == [0, 1, 63, 65, 257, 1023, 1025, 4097, 133312]
    order = np.random.default_rng(3).permutation(nf)
    assert list(order) != sorted(order)
    maps = [[],
            [(10, _matrix(POSES[1]))],
            [(18, _matrix(POSES[2])), (19, _matrix(POSES[3]))],                                  # the two empty frames only
            [(int(f), _matrix((0.5 * f - 5, 3 - 0.25 * f, 0.01 * f, 7.0 * f))) for f in order],  # every frame once
            [(14, _matrix(POSES[1])), (14, _matrix(POSES[3])), (14, _matrix(POSES[4]))],         # one frame three times
            [(17, _matrix(FAR)), (6, _matrix(POSES[2]))]]                                        # the full sweep, far off
    skip = bool(skip)
    want = [_want(frames, m, interval, skip) for m in maps]
    assert not want[0].any() and not want[2].any() and want[1].any() and want[3].any() and want[5].any()
    # the union really is one: map 4's grid is not any single entry's
    assert all(want[4].tobytes() != _want(frames, [e], interval, skip).tobytes() for e in maps[4])
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=4, max_points=p.slots)
    try:
        M = int(ctx.lib.bev_float_bev_size(interval))
        assert M == {1.0: 201, 2.0: 101, 0.5: 401}[interval]
        got = _call(ctx, frames, maps, interval, skip)
        assert got.shape == (len(maps), M, M)
        _check(frames, maps, got, want=want)
    finally:
        ctx.close()


def test_one_entry_per_map_is_the_float_call():
    adv, marked = _adversarial(), _marked()
    frames = [marked[:9000], adv[:0], adv[100:1125], marked[60000:60257], adv[7:4104]]
    nf, K, M = len(frames), 3, 201
    poses = np.stack([np.stack([_matrix(POSES[(f + k) % 5]) for k in range(2)] + [_matrix(FAR)]) for f in range(nf)])
    maps = [[(f, poses[f, k])] for f in range(nf) for k in range(K)]
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        for skip in (True, False):
            got = _call(ctx, frames, maps, 1.0, skip)
            offs, flat = _pack(frames)
            d_in, d_out = _dev(flat), _out(nf * K, M)
            torch.cuda.synchronize()
            ctx.float_bev_device(nf, d_in.data_ptr(), offs, d_out.data_ptr(), 1.0, skip, poses=poses)
            ctx.synchronize()
            assert got.tobytes() == _grids(d_out, nf * K, M).tobytes()
            assert got.any() and not got[K:2 * K].any()
    finally:
        ctx.close()


def test_contention_across_frames_and_what_must_not_be_stored():
    """five frames whose points all lie in ONE cell, in one map under the identity: the atomic's maximum under contention
    within and across frames.  The frames that must leave no trace (label 0 under skip; heights that are NaN or <= -2) are
    shifted by 5 m: their cell stays empty."""
    fmax = np.finfo(np.float32).max
    rng = np.random.default_rng(5)
    plain = rng.permutation(np.linspace(-1.99, 60.0, 20000 - 9).astype(np.float32))
    assert len(np.unique(plain)) == len(plain)
    special = np.array([-5.0, -2.0, -2.0000002, 0.0, -0.0, np.nan, -np.inf, fmax, np.inf], dtype=np.float32)
    low = np.array([-5.0, -2.0, -2.0000002, -np.inf, np.nan, -1e30] * 50, dtype=np.float32)   # nothing is stored
    ghosts = np.array([70.0, fmax, np.inf, 61.0], dtype=np.float32)                           # label 0, above everything else
    parts = np.array_split(plain, 3)                                                          # unique heights spread over frames
    # (under a matrix a height that is not finite makes x and y NaN, 0 * inf: such a point is off the grid)
    frames = [_one_cell(np.concatenate([parts[0][:3000], special[:7], special[8:], parts[0][3000:]])),
              _one_cell(parts[1]),
              _one_cell(np.concatenate([ghosts] * 64), 0),                                    # nothing but label-0 points
              _one_cell(np.concatenate([parts[2], special[:5]])),
              _one_cell(low)]
    shift = _matrix((5, 0, 0, 0))
    top = np.float32(plain.max()) + np.float32(2)
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        for skip in (True, False):
            # without the label test frame 2 counts: it then stays out of the first map and has the second to itself
            maps = [[(0, IDENTITY), (1, IDENTITY), (3, IDENTITY), (4, shift)] + ([(2, shift)] if skip else []),
                    [(2, IDENTITY), (4, shift)],
                    [(0, IDENTITY), (3, IDENTITY), (1, IDENTITY), (0, IDENTITY), (2, IDENTITY)]]
            want = [_want(frames, m, 1.0, skip) for m in maps]
            assert [int(np.count_nonzero(w)) for w in want] == [1, 0 if skip else 1, 1]
            got = _call(ctx, frames, maps, 1.0, skip)
            _check(frames, maps, got, want=want)
            assert [int(np.count_nonzero(g)) for g in got] == [1, 0 if skip else 1, 1]
            assert got[0].max() == top and got[0][101, 93] == top                # the cell of x = 0.3, y = -7.2
            assert got[1].max() == (0.0 if skip else fmax)                       # FLT_MAX + 2 is FLT_MAX
            assert got[2].max() == (top if skip else fmax)
    finally:
        ctx.close()


def test_in_wave_combine_across_entries():
    """a frame of 4096 equal heights (every lane but a wave's last is covered by its neighbour) and a frame of strictly
    descending heights (no lane is) in one cell, in one map, two entries each under small translations that keep them in the
    cell: the chains of float_bev_put when the entry loop runs more than once"""
    equal = _one_cell(np.full(4096, 1.625, np.float32))
    desc = _one_cell(np.linspace(9.0, -1.5, 4096).astype(np.float32))
    assert (np.diff(desc["z"]) < 0).all()
    asc = _one_cell(np.ascontiguousarray(desc["z"][::-1]))
    frames = [equal, desc, asc]
    t = lambda dx, dy, dz: _matrix((dx, dy, dz, 0))
    maps = [[(0, t(0.05, 0.1, 0.5)), (1, t(0.1, -0.05, 0.0)), (0, t(-0.1, 0.05, 0.25)), (1, t(0.02, 0.03, -1.0))],
            [(0, t(0.05, 0.1, 0.5)), (0, t(-0.1, 0.05, 0.25))],
            [(1, t(0.1, -0.05, -8.0)), (0, t(0.0, 0.0, 0.0))],          # the equal frame wins
            [(2, t(0.1, 0.1, 0.125)), (1, t(0.0, 0.0, 0.0)), (2, t(0.0, 0.0, -0.5))]]
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        got = _call(ctx, frames, maps)
        _check(frames, maps, got)
        assert [int(np.count_nonzero(g)) for g in got] == [1, 1, 1, 1]
        assert [float(g.max()) for g in got] == [11.0, 4.125, 3.625, 11.125]
    finally:
        ctx.close()


def test_long_entry_lists():
    """a frame feeding 150 one-entry maps, and one map of 150 entries of one 257-record frame"""
    marked = _marked()
    frames = [marked[20000:24097], marked[60000:60257]]
    rng = np.random.default_rng(2)
    mats = [_matrix((rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(-1, 1), rng.uniform(-180, 180))) for _ in range(150)]
    maps = [[(0, m)] for m in mats] + [[(1, m) for m in mats]]
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        got = _call(ctx, frames, maps)
        _check(frames, maps, got)
        assert got[0].any() and got[149].any() and got[150].any()
    finally:
        ctx.close()


def _windows(n, h, pose_of):
    """sliding windows of half width h at stride 1 over n frames: map i = frames i - h .. i + h under pose_of(j - i)"""
    return [[(j, pose_of(j - i)) for j in range(max(0, i - h), min(n - 1, i + h) + 1)] for i in range(n)]


def test_sliding_windows_are_one_launch():
    """12 maps of up to 5 frames: ONE splat launch, no planes and no expand pass"""
    adv, marked = _adversarial(), _marked()
    sizes = [257, 12000, 3000, 1025, 7000, 4097, 900, 11000, 2048, 5000, 1024, 8000]
    frames = [(marked if i % 2 else adv)[3000 * i:3000 * i + n] for i, n in enumerate(sizes)]
    maps = _windows(12, 2, lambda d: IDENTITY if d == 0 else _matrix((2.0 * d, 0.3 * d, 0.0, 1.0 * d)))
    assert len(maps) == 12 and sum(len(m) for m in maps) == 54
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=p.slots)
    try:
        ctx.profile_reset()
        ctx.profile_enable(True)
        got = _call(ctx, frames, maps)
        launches = {k["name"]: k["launches"] for k in ctx.profile_get()}
        ctx.profile_enable(False)
        _check(frames, maps, got)
        assert launches["k_submap_float_splat"] == 1, launches
        assert launches.get("k_posed_expand", 0) == 0 and launches.get("k_submap_splat", 0) == 0, launches
        assert launches.get("k_float_bev_batch", 0) == 0 and launches.get("k_posed_splat", 0) == 0, launches
        # maps of empty frames only: no point, no launch
        ctx.profile_reset()
        ctx.profile_enable(True)
        empty = _call(ctx, [adv[:0], adv[:0]], [[(0, IDENTITY), (1, IDENTITY)], []])
        launches = {k["name"]: k["launches"] for k in ctx.profile_get()}
        assert not empty.any() and launches.get("k_submap_float_splat", 0) == 0, launches
    finally:
        ctx.close()


def test_stream_ordering_with_the_bev_path():
    """process_device, then the submap float call on its d_ordered with nothing between them while the default stream is busy;
    then the submap float call followed at once by a process_device that overwrites d_ordered"""
    p = _p()
    sp = orc.sensor_from_params(p)
    S, M = p.slots, 201
    dev = torch.device("cuda:0")
    first = [synth.sweep(p, 30), synth.sweep(p, 31)[:70000], synth.adversarial(p, 20000, 4)]
    other = [synth.sweep(p, 32)[:90000], synth.adversarial(p, 30000, 6), synth.sweep(p, 33)]
    nf = len(first)
    want = {k: [orc.mark_ground(sp, orc.order_cloud(sp, c))[0] for c in fs] for k, fs in (("first", first), ("other", other))}
    offs_s = np.arange(nf + 1, dtype=np.uint64) * np.uint64(S)
    maps = [[(0, IDENTITY), (1, _matrix(POSES[1])), (2, _matrix(POSES[2]))], [(1, IDENTITY)], [(2, _matrix(POSES[4])), (0, _matrix(POSES[3]))]]
    want_maps = [_want(want["first"], m) for m in maps]
    ctx = bev_amd.BevContext(p, device=0, max_batch=4, max_points=S + 8192)
    try:
        (o1, flat1), (o2, flat2) = _pack(first), _pack(other)
        src1, d_other = _dev(flat1), _dev(flat2)
        d_pts = torch.zeros_like(src1)
        d_ordered = torch.zeros(nf * S * 32, dtype=torch.uint8, device=dev)
        d_multi = torch.zeros(nf * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device=dev)
        d_single = torch.zeros(nf * p.mat_size ** 2, dtype=torch.uint8, device=dev)
        g1, g2 = _out(len(maps), M), _out(len(maps), M)
        busy = torch.randn(4096, 4096, device=dev)
        torch.cuda.synchronize()
        for _ in range(4):   # the default stream is busy when the library is called: the fill below is still queued
            busy = busy @ busy * 1e-3
        d_pts.copy_(src1)
        ctx.process_device(nf, d_pts.data_ptr(), o1, d_ordered.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
        ctx.submap_float_bev_device(nf, d_ordered.data_ptr(), offs_s, *_entries(maps), g1.data_ptr())
        ctx.synchronize()
        _check(want["first"], maps, _grids(g1, len(maps), M), want=want_maps)

        # reverse order: the splat still reads d_ordered when the pipeline that overwrites it is issued
        ctx.submap_float_bev_device(nf, d_ordered.data_ptr(), offs_s, *_entries(maps), g2.data_ptr())
        ctx.process_device(nf, d_other.data_ptr(), o2, d_ordered.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
        ctx.synchronize()
        got_ordered = d_ordered.cpu().numpy().view(POINT_DTYPE).reshape(nf, S)
        _check(want["first"], maps, _grids(g2, len(maps), M), want=want_maps)
        for f in range(nf):
            assert got_ordered[f].tobytes() == want["other"][f].tobytes(), f
        assert _guard_ok(g1, len(maps), M) and _guard_ok(g2, len(maps), M)
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
        d_in, d_out = _dev(flat), _out(2, 201)
        torch.cuda.synchronize()
        L = ctx.lib
        u64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64)) if a is not None else None
        vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        bad_frame, neg_frame = eframe.copy(), eframe.copy()
        bad_frame[2], neg_frame[0] = 2, -1
        many = np.array([0, SUBMAP_MAX_ENTRIES + 1], dtype=np.uint64)         # real arrays of that length
        many_frame = np.zeros(SUBMAP_MAX_ENTRIES + 1, dtype=np.int32)
        many_pose = np.tile(IDENTITY, (SUBMAP_MAX_ENTRIES + 1, 1))
        host_arrays = [a.copy() for a in (offs, moffs, eframe, epose)]

        def call(h=ctx._h, n=2, din=d_in.data_ptr(), o=offs, interval=1.0, n_maps=2, mo=moffs, ef=eframe, ep=epose,
                 dout=d_out.data_ptr()):
            return L.bev_submap_float_bev_device_resident(h, n, din, u64p(o), interval, 1, n_maps, u64p(mo), vp(ef), vp(ep), dout)

        assert call(h=None) == INVALID
        assert call(n=-1) == INVALID and call(n_maps=-1) == INVALID
        assert call(o=None) == INVALID and call(mo=None) == INVALID
        assert call(o=np.array([0, 5000, 3000], dtype=np.uint64)) == INVALID          # decreasing frame offsets
        assert call(mo=np.array([0, 3, 2], dtype=np.uint64)) == INVALID               # decreasing map offsets
        assert call(ef=None) == INVALID and call(ep=None) == INVALID                  # entries, but no entry array
        assert call(ef=bad_frame) == INVALID and call(ef=neg_frame) == INVALID        # an entry frame outside 0 .. n_frames - 1
        assert call(din=None) == INVALID                                              # NULL clouds with records to read
        assert call(dout=None) == INVALID                                             # NULL output with maps
        assert call(dout=None, n_maps=1, mo=np.zeros(2, dtype=np.uint64), ef=None, ep=None) == INVALID   # (an empty map still gets its grid)
        for interval in (0.0, -1.0, float("nan"), 0.1):                               # M = 0, or above 1024
            assert L.bev_float_bev_size(interval) == 0
            assert call(interval=interval) == UNSUPPORTED
        assert call(n=1, o=np.array([0, p.slots + 1], dtype=np.uint64), n_maps=1, mo=np.array([0, 1], dtype=np.uint64)) == TOO_LARGE
        assert call(n_maps=1, mo=many, ef=many_frame, ep=many_pose) == TOO_LARGE
        assert call(n_maps=1, mo=many, ef=None, ep=None) == TOO_LARGE                 # the count is checked before the arrays are read
        assert call(n_maps=0, mo=moffs[:1].copy(), ef=None, ep=None, dout=None) == 0  # nothing to do
        ctx.synchronize()
        assert bool((d_out == PATTERN).all()), "a refused call wrote to d_out"

        # the host-buffer call refuses the same things
        cl = (C.c_void_p * 2)(*[f.ctypes.data for f in frames])
        n_pts = (C.c_uint32 * 2)(3000, 5000)
        host = np.full((2, 201, 201), -7.0, dtype=np.float32)
        outs = (C.c_void_p * 2)(*[host[i].ctypes.data for i in range(2)])

        def hcall(h=ctx._h, n=2, clouds=cl, npts=n_pts, interval=1.0, n_maps=2, mo=moffs, ef=eframe, ep=epose, out=outs):
            return L.bev_submap_float_bev_batch(h, n, clouds, npts, interval, 1, n_maps, u64p(mo), vp(ef), vp(ep), out)

        assert hcall(h=None) == INVALID and hcall(n=-1) == INVALID and hcall(n_maps=-1) == INVALID
        assert hcall(clouds=None) == INVALID and hcall(npts=None) == INVALID and hcall(out=None) == INVALID
        assert hcall(clouds=(C.c_void_p * 2)(frames[0].ctypes.data, None)) == INVALID
        assert hcall(out=(C.c_void_p * 2)(host[0].ctypes.data, None)) == INVALID
        assert hcall(mo=None) == INVALID and hcall(mo=np.array([0, 3, 2], dtype=np.uint64)) == INVALID
        assert hcall(ef=None) == INVALID and hcall(ep=None) == INVALID
        assert hcall(ef=bad_frame) == INVALID and hcall(ef=neg_frame) == INVALID
        for interval in (0.0, -1.0, float("nan"), 0.1):
            assert hcall(interval=interval) == UNSUPPORTED
        assert hcall(npts=(C.c_uint32 * 2)(3000, p.slots + 1)) == TOO_LARGE
        assert hcall(n_maps=1, mo=many, ef=many_frame, ep=many_pose) == TOO_LARGE
        assert hcall(n_maps=1, mo=many, ef=None, ep=None) == TOO_LARGE
        assert hcall(n_maps=0, mo=moffs[:1].copy(), ef=None, ep=None, out=None) == 0
        assert (host == -7.0).all(), "a refused call wrote to its outputs"
        for a, b in zip(host_arrays, (offs, moffs, eframe, epose)):
            assert a.tobytes() == b.tobytes(), "a call wrote to a host array"

        # valid calls still work
        assert call() == 0
        ctx.synchronize()
        got = _grids(d_out, 2, 201)
        _check(frames, maps, got)
        assert got[0].any() and _guard_ok(d_out, 2, 201)
        assert hcall() == 0
        assert host.tobytes() == got.tobytes()
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
        for interval, skip in ((1.0, True), (2.0, False)):
            got = ctx.submap_float_bev_batch(frames, *_entries(maps), interval, skip)
            M = {1.0: 201, 2.0: 101}[interval]
            assert got.shape == (5, M, M) and got.dtype == np.float32
            _check(frames, maps, got, interval, skip)
            assert got.tobytes() == _call(ctx, frames, maps, interval, skip).tobytes()
            assert got[1].any() and not got[2].any()
        first = ctx.submap_float_bev_batch(frames, *_entries(maps))
        again = ctx.submap_float_bev_batch(frames, *_entries(maps[:2]))      # a smaller call behind a larger one
        assert again.shape == (2, 201, 201) and again.tobytes() == first[:2].tobytes()
        assert ctx.submap_float_bev_batch([], *_entries([])).shape == (0, 201, 201)          # zero maps and zero frames
        assert ctx.submap_float_bev_batch(frames, *_entries([])).shape == (0, 201, 201)      # zero maps
        none = ctx.submap_float_bev_batch([], *_entries([[], []]))                           # zero frames: empty maps
        assert none.shape == (2, 201, 201) and not none.any()
    finally:
        ctx.close()
