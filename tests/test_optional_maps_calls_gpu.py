"""GPU: what the two device-resident calls over frames and OPTIONAL maps share (bev_place_descriptor_device_resident,
DESIGN.md §6z; bev_align_grid_device_resident, §6ab): the statuses of their common arguments and the order in which they are
reported; and bev_place_retrieval_batch's database of maps going through the staging in pieces, against the two
device-resident calls and the sequential checker.  Every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import bev_amd
import place_lib
from bev_amd import SUBMAP_MAX_ENTRIES, align_params, place_params
from packed_cases import FAR, INVALID, PATTERN, POSES, TOO_LARGE, _adversarial, _dev, _marked, _matrix, _p, _pack
from place_gpu_lib import HB, descriptors, guarded, match

pytestmark = pytest.mark.gpu

IDENTITY = np.eye(3, 4, dtype=np.float32).reshape(12)


def _entries(maps):
    """maps: per map a list of (frame, matrix) -> (map_offsets, entry_frame, entry_pose)"""
    offs = np.zeros(len(maps) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(m) for m in maps])
    frame = np.array([f for m in maps for f, _ in m], dtype=np.int32)
    pose = np.array([mat for m in maps for _, mat in m], dtype=np.float32).reshape(-1, 12)
    return offs, frame, pose


@pytest.mark.parametrize("which", ["place", "align"])
def test_statuses_and_their_order(which):
    p = _p()
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=1000)   # frames of up to max(max_points, S) = S records
    try:
        L = ctx.lib
        frames = [_marked()[:0], _marked()[20000:23000]]                  # frame 0 is empty
        offs, flat = _pack(frames)
        d_in = _dev(flat)
        if which == "place":
            prm, fn = place_params(), L.bev_place_descriptor_device_resident
            out_a, out_b = guarded(2 * 20 * 60), guarded(2 * HB)          # descriptors, unit records
        else:
            prm, fn = align_params(), L.bev_align_grid_device_resident
            out_a, out_b = guarded(2 * bev_amd.align_grid_bytes(prm)), guarded(2 * 4)   # grids, sums of squares
        u64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64)) if a is not None else None
        vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        u64 = lambda *v: np.array(v, dtype=np.uint64)
        one = np.tile(IDENTITY, (1, 1))
        big = u64(0, p.slots + 1)                                         # one frame that is too large
        many = u64(0, SUBMAP_MAX_ENTRIES + 1)

        def call(n=2, din=d_in.data_ptr(), o=offs, n_maps=0, mo=None, ef=None, ep=None, a=out_a.data_ptr(), b=out_b.data_ptr()):
            return fn(ctx._h, n, din, u64p(o), n_maps, vp(mo), vp(ef), vp(ep), C.byref(prm), a, b)

        def untouched():
            ctx.synchronize()
            return bool((out_a == PATTERN).all()) and bool((out_b == PATTERN).all())

        assert call(o=u64(0, 5000, 3000)) == INVALID                                       # descending frame offsets
        assert call(o=u64(0, 5000, 3000), n_maps=1, mo=u64(0, 1), ef=np.array([0], np.int32), ep=one) == INVALID
        # a frame that is too large is reported behind the arguments that are wrong ...
        assert call(n=1, o=big, n_maps=1, mo=u64(0, 1), ef=np.array([1], np.int32), ep=one) == INVALID   # entry frame out of range
        assert call(n=1, o=big, n_maps=1, mo=None, ef=None, ep=None) == INVALID            # maps without their offsets
        # ... and alone it is what the call returns, with and without maps
        assert call(n=1, o=big, n_maps=1, mo=u64(0, 1), ef=np.array([0], np.int32), ep=one) == TOO_LARGE
        assert call(n=1, o=big) == TOO_LARGE
        assert call(n=1, o=big, a=None, b=None) == TOO_LARGE                               # (ahead of the output pointers)
        # the count of entries is checked before the entry arrays are read
        assert call(n_maps=1, mo=many, ef=None, ep=None) == TOO_LARGE
        # no map offsets: n_maps must be 0 and both entry arrays NULL
        assert call(n_maps=1, mo=None) == INVALID
        assert call(n_maps=0, mo=None, ef=np.array([0], np.int32)) == INVALID
        assert call(n_maps=0, mo=None, ep=one) == INVALID
        # nothing to do: NULL outputs pass
        assert call(n=0, o=u64(0), a=None, b=None) == 0
        assert call(n=0, o=u64(0), din=None, a=None, b=None) == 0
        assert call(n_maps=0, mo=u64(0), a=None, b=None) == 0
        assert call(a=None, b=None) == INVALID                                             # ... but not with something to do
        assert call(n_maps=1, mo=u64(0, 0), a=None, b=None) == INVALID                     # (an empty map still gets its output)
        # NULL clouds with records to read
        assert call(din=None) == INVALID
        assert call(din=None, n_maps=1, mo=u64(0, 1), ef=np.array([1], np.int32), ep=one) == INVALID
        assert call(din=None, n_maps=2, mo=u64(0, 1, 2), ef=np.array([0, 1], np.int32), ep=np.tile(IDENTITY, (2, 1))) == INVALID
        assert untouched(), "a refused call or one with nothing to do wrote to its outputs"
        # ... and with only empty frames named there is nothing to read: all-zero outputs
        n_a, n_b = (20 * 60, HB) if which == "place" else (bev_amd.align_grid_bytes(prm), 4)
        assert call(n=1, din=None, o=u64(0, 0)) == 0
        ctx.synchronize()
        assert not out_a[:n_a].any() and not out_b[:n_b].any() and bool((out_a[n_a:] == PATTERN).all()) and bool((out_b[n_b:] == PATTERN).all())
        out_a.fill_(PATTERN)
        out_b.fill_(PATTERN)
        assert call(din=None, n_maps=2, mo=u64(0, 2, 2), ef=np.array([0, 0], np.int32), ep=np.tile(IDENTITY, (2, 1))) == 0
        ctx.synchronize()
        assert not out_a[:2 * n_a].any() and bool((out_a[2 * n_a:] == PATTERN).all()) and bool((out_b[2 * n_b:] == PATTERN).all())
        # a valid call over the same buffers still works: frame 1's output is not empty
        assert call() == 0
        ctx.synchronize()
        assert not out_a[:n_a].any() and out_a[n_a:2 * n_a].any() and bool((out_a[2 * n_a:] == PATTERN).all())
    finally:
        ctx.close()


def test_retrieval_batch_with_maps_through_pieces():
    """7 frames, 5 maps through a context of max_batch 2: four chunks of queries, three chunks of maps; map 1 names 5 distinct
    frames, which go through the staging in three pieces; against the two device-resident calls and the checker"""
    adv, marked = _adversarial(), _marked()
    frames = [adv[:0], adv[5:6], marked[5000:5255], adv[7:1032], marked[20000:24097], adv[30000:33000], marked[60000:65000]]
    assert [len(f) for f in frames] == [0, 1, 255, 1025, 4097, 3000, 5000]
    maps = [[(4, _matrix(POSES[1]))],
            [(6, _matrix(POSES[2])), (0, IDENTITY), (3, _matrix(POSES[3])), (4, _matrix(FAR)), (5, _matrix(POSES[4])), (3, _matrix(POSES[1]))],
            [],
            [(2, IDENTITY), (1, _matrix(POSES[2]))],
            [(5, _matrix(POSES[3])), (4, _matrix(POSES[0]))]]
    assert len({f for f, _ in maps[1]}) == 5
    limit = np.array([5, 0, 3, 5, 1, 4, 2], np.int32)
    top_k, prm = 3, place_params()
    mo, ef, ep = _entries(maps)
    ctx = bev_amd.BevContext(_p(), device=0, max_batch=2)
    try:
        got = ctx.place_retrieval_batch(frames, top_k, limit, prm, mo, ef, ep)
        assert got.shape == (7, top_k)
        units_q = descriptors(ctx, frames, prm, want_desc=False)[1]
        desc_db, units_db = descriptors(ctx, frames, prm, maps=(mo, ef, ep))
        assert desc_db[0].any() and desc_db[1].any() and not desc_db[2].any() and desc_db[4].any()
        assert got.tobytes() == match(ctx, prm, units_q, units_db, top_k, limit).tobytes()
        dq = np.stack([place_lib.descriptor([(f, None)], prm) for f in frames])
        ddb = np.stack([place_lib.descriptor([(frames[f], mat) for f, mat in m], prm) for m in maps])
        assert ddb.tobytes() == desc_db.tobytes()
        assert got.tobytes() == place_lib.match(dq, ddb, top_k, limit).tobytes()
        assert (got["match_idx"][1] == -1).all() and (got["match_idx"][3] >= 0).all() and (got["match_idx"][6, 2] == -1)
        again = ctx.place_retrieval_batch(frames, top_k, limit, prm, mo, ef, ep)     # the buffers of the call before are reused
        assert again.tobytes() == got.tobytes()
    finally:
        ctx.close()
