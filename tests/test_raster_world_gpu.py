"""GPU: the posed and submap rasters against a float64 world.  The four device calls, their *_batch forms and
the per-cloud chain raster the frames of raster_world_cases.py under general rigid matrices; every result is compared with
the float64 reference that rasters WORLD coordinates (bytes; for the float grid the same occupied cells and tol, 8 times the
reference's own float32-against-float64 difference) and, bit for bit, with the oracle's composition under the same float32
matrices: the first bit-for-bit check of the splat kernels under matrices whose 12 entries are all far from 0 and 1."""
import functools
import os

import numpy as np
import pytest
import torch

import bev_amd
import raster_world_cases as rw
import raster_world_checker as ck
from packed_cases import GUARD, PATTERN, _dev, _Out, _pack

pytestmark = pytest.mark.gpu
SENSORS = tuple(rw.CONFIGS)
K = len(rw.posed_origins())


def _entries(maps):
    offs = np.zeros(len(maps) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(m) for m in maps])
    frame = np.array([f for m in maps for f, _ in m], dtype=np.int32)
    pose = np.array([mat for m in maps for _, mat in m], dtype=np.float32).reshape(-1, 12)
    return offs, frame, pose


@functools.lru_cache(maxsize=None)
def _want(sensor):
    """per compared map, (the float64 reference's images, the oracle composition's): computed once per configuration"""
    c = rw.case(sensor)
    return {name: (ck.reference(c, name), ck.composition(c, c.entries(name))) for name in c.maps}


def _check(sensor, name, got, what):
    """the images got ({key: array}) of one compared map: within the float64 world's bounds, and the composition's bits"""
    c = rw.case(sensor)
    ref, comp = _want(sensor)[name]
    d = ck.compare(got, ref, c.tol(), f"{what}, {sensor}, map {name}")
    for key, g in got.items():
        assert g.tobytes() == comp[key].tobytes(), f"{what}, {sensor}, map {name}, {key}: not the oracle composition's bits"
    return d


@pytest.fixture(scope="module", params=SENSORS)
def world(request):
    c = rw.case(request.param)
    ctx = bev_amd.BevContext(ck.params(c), device=0, max_batch=4, max_points=4096)
    yield c, ctx
    ctx.close()


def _float_out(n, M):
    return torch.full((n * M * M * 4 + GUARD,), PATTERN, dtype=torch.uint8, device=torch.device("cuda:0"))


def _float_grids(t, n, M):
    assert bool((t[n * M * M * 4:] == PATTERN).all()), "something was written behind d_out"
    return t[:n * M * M * 4].cpu().numpy().view(np.float32).reshape(n, M, M)


def _submap_call(ctx, c, names):
    """the submap call and the submap float call (both label rules) over the named maps: {name: {key: image}}"""
    maps = [c.entries(n) for n in names]
    offs, flat = _pack(c.frames)
    d_in, out = _dev(flat), _Out(ctx.params, len(maps))
    f1, f0 = _float_out(len(maps), c.Mf), _float_out(len(maps), c.Mf)
    torch.cuda.synchronize()
    ctx.submap_bev_device(len(c.frames), d_in.data_ptr(), offs, *_entries(maps), *out.ptrs())
    ctx.submap_float_bev_device(len(c.frames), d_in.data_ptr(), offs, *_entries(maps), f1.data_ptr(), c.interval, True)
    ctx.submap_float_bev_device(len(c.frames), d_in.data_ptr(), offs, *_entries(maps), f0.data_ptr(), c.interval, False)
    ctx.synchronize()
    assert out.guards_ok(), "something was written behind an output"
    gm, gs = out.images()
    g1, g0 = _float_grids(f1, len(maps), c.Mf), _float_grids(f0, len(maps), c.Mf)
    return {n: {"multi": gm[i], "single": gs[i], "float1": g1[i], "float0": g0[i]} for i, n in enumerate(names)}


def _posed_call(ctx, c):
    """the posed call and the float call (both label rules) over all frames x K poses: {("posed", f, k): {key: image}}"""
    poses = c.posed_matrices()
    n = len(c.frames)
    offs, flat = _pack(c.frames)
    d_in, out = _dev(flat), _Out(ctx.params, n * K)
    f1, f0 = _float_out(n * K, c.Mf), _float_out(n * K, c.Mf)
    torch.cuda.synchronize()
    ctx.posed_bev_device(n, d_in.data_ptr(), offs, *out.ptrs(), poses=poses)
    ctx.float_bev_device(n, d_in.data_ptr(), offs, f1.data_ptr(), c.interval, True, poses=poses)
    ctx.float_bev_device(n, d_in.data_ptr(), offs, f0.data_ptr(), c.interval, False, poses=poses)
    ctx.synchronize()
    assert out.guards_ok(), "something was written behind an output"
    gm, gs = out.images()
    g1, g0 = _float_grids(f1, n * K, c.Mf), _float_grids(f0, n * K, c.Mf)
    return {("posed", f, k): {"multi": gm[f * K + k], "single": gs[f * K + k], "float1": g1[f * K + k], "float0": g0[f * K + k]}
            for f in range(n) for k in range(K)}


def test_the_four_device_calls_on_the_world(world):
    c, ctx = world
    assert c.tol() <= rw.CAP
    assert all(len(f) > 1024 for f in c.frames)                      # more than one workgroup per frame
    worst = {}
    for what, got in (("submap calls", _submap_call(ctx, c, rw.SUBMAPS)), ("posed and float calls", _posed_call(ctx, c))):
        worst[what] = max(_check(c.sensor, name, images, what) for name, images in got.items())
        assert any(images["multi"].any() for images in got.values()) and any(images["float0"].any() for images in got.values())
    print(f"{c.sensor}: 0 bytes from the float64 world in every uint8 image; float grids within "
          f"{ {k: f'{v:.2e}' for k, v in worst.items()} }, tol {c.tol():.2e}")


def test_the_batch_forms_and_the_per_cloud_chain(world):
    c, ctx = world
    names = ("T", "F")
    maps = [c.entries(n) for n in names]
    multi, single = ctx.submap_bev_batch(c.frames, *_entries(maps))
    for skip, key in ((True, "float1"), (False, "float0")):
        grids = ctx.submap_float_bev_batch(c.frames, *_entries(maps), c.interval, skip)
        for i, n in enumerate(names):
            _check(c.sensor, n, {key: grids[i]}, "submap float batch")
    for i, n in enumerate(names):
        _check(c.sensor, n, {"multi": multi[i], "single": single[i]}, "submap batch")
    # the posed forms: every frame about T's and F's origins (poses 1 and 2 of the posed grids)
    poses = np.ascontiguousarray(c.posed_matrices()[:, 1:])
    multi, single = ctx.posed_bev_batch(c.frames, poses=poses)
    f1 = ctx.float_bev_batch(c.frames, c.interval, True, poses=poses)
    f0 = ctx.float_bev_batch(c.frames, c.interval, False, poses=poses)
    for f in range(len(c.frames)):
        for k in (1, 2):
            _check(c.sensor, ("posed", f, k), {"multi": multi[f, k - 1], "single": single[f, k - 1], "float1": f1[f, k - 1],
                                                "float0": f0[f, k - 1]}, "posed and float batch")
    # the per-cloud chain: bev_transform_cloud, then the three rasters of the concatenation
    for n, entries in zip(names, maps):
        moved = np.concatenate([ctx.transform_cloud(c.frames[f], m) for f, m in entries])
        _check(c.sensor, n, {"multi": ctx.multi_bev(moved), "single": ctx.single_bev(moved),
                             "float1": ctx.float_bev(moved, c.interval, True), "float0": ctx.float_bev(moved, c.interval, False)},
               "per-cloud chain")


def test_launch_groups_do_not_change_the_bytes(world):
    """BEV_POSED_GROUP=2: every submap group holds two maps, and a frame's three posed grids exceed the cap, so every frame is
    a group of its own; the bytes are those of the one-group calls and of the float64 world"""
    c, whole = world
    want_sub, want_posed = _submap_call(whole, c, rw.SUBMAPS), _posed_call(whole, c)
    saved = os.environ.get("BEV_POSED_GROUP")
    os.environ["BEV_POSED_GROUP"] = "2"
    try:
        ctx = bev_amd.BevContext(ck.params(c), device=0, max_batch=4, max_points=4096)
        try:
            ctx.profile_reset()
            ctx.profile_enable(True)
            got_sub, got_posed = _submap_call(ctx, c, rw.SUBMAPS), _posed_call(ctx, c)
            launches = {k["name"]: k["launches"] for k in ctx.profile_get()}
        finally:
            ctx.close()
    finally:
        if saved is None:
            os.environ.pop("BEV_POSED_GROUP", None)
        else:
            os.environ["BEV_POSED_GROUP"] = saved
    assert launches["k_submap_splat"] == len(rw.SUBMAPS) // 2 and launches["k_posed_splat"] == len(c.frames), launches
    for got, want in ((got_sub, want_sub), (got_posed, want_posed)):
        for name, images in got.items():
            for key in ("multi", "single"):
                assert images[key].tobytes() == want[name][key].tobytes(), (name, key)
            _check(c.sensor, name, {k: images[k] for k in ("multi", "single")}, "small launch groups")
