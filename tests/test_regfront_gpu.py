"""GPU: the registration front end (top-part flatten -> voxel grid -> 2-D normals) byte for byte against the sequential
checker tests/regfront/regfront_oracle.c, per-cloud and as the batched device-resident chain over the BEV path's
d_ordered output."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bev_amd
import oracle_lib as orc
import regfront_lib as rl
from bev_amd import synth

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 4)
NAN = 0x7FC00000


@pytest.fixture(scope="module", autouse=True)
def _checker():
    rl.build()


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _cloud(xyz, label=1):
    c = np.zeros(len(xyz), dtype=bev_amd.POINT_DTYPE)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    c["x"], c["y"], c["z"], c["label"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], label
    return c


def _skipped_cells(cloud):
    ok = (cloud["label"] != 0) & np.isfinite(cloud["x"]) & np.isfinite(cloud["y"]) & np.isfinite(cloud["z"])
    gx = np.trunc((cloud["x"][ok] + np.float32(100)) / np.float32(20) + np.float32(0.5) * np.sign(cloud["x"][ok] + 100))
    gy = np.trunc((cloud["y"][ok] + np.float32(100)) / np.float32(20) + np.float32(0.5) * np.sign(cloud["y"][ok] + 100))
    inside = (gx >= 0) & (gx < 10) & (gy >= 0) & (gy < 10)
    cnt = np.bincount((gx[inside] * 10 + gy[inside]).astype(np.int64), minlength=100)
    return int(((cnt > 0) & (cnt < 20)).sum())


@pytest.mark.parametrize("sensor", ["HDL_32E", "HDL_64E", "OS1_64"])
def test_per_cloud_entries_on_labelled_ordered_clouds(sensor):
    p = bev_amd.params_for_sensor(sensor)
    pts = synth.sweep(p, 77, keep=0.9, n_dup=300)
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=len(pts))
    try:
        ordered = ctx.process_batch([pts])[0][0]
        flat = ctx.top_part_flatten(ordered)
        assert len(flat) > 100
        assert _same(flat, rl.top_part(ordered))
        vox = ctx.voxel_grid(flat, 0.2)
        assert 0 < len(vox) < len(flat)  # multi-point voxels
        assert _same(vox, rl.voxel(flat, 0.2))
        nrm = ctx.normals_2d(vox, 2.0)
        exp, nn = rl.normals(vox, 2.0, want_nn=True)
        assert _same(nrm, exp)
        assert (nn >= 3).any()
        # a 3-D voxel grid of the labelled cloud itself (z != 0) and a viewpoint off the origin
        xyz = np.c_[ordered["x"], ordered["y"], ordered["z"]][ordered["label"] != 0]
        assert _same(ctx.voxel_grid(xyz, 0.5), rl.voxel(xyz, 0.5))
        assert _same(ctx.normals_2d(vox[:3000], 1.0, (5.0, -3.0, 0.0)), rl.normals(vox[:3000], 1.0, (5.0, -3.0, 0.0)))
        with pytest.raises(bev_amd.BevError, match="status -5"):
            ctx.normals_2d(vox[:10], 2.0, k_search=10)  # setKSearch
    finally:
        ctx.close()


def test_f64_sqrt_and_division_are_correctly_rounded():
    """|N| = 2 and |N| >= 3 normals hinge on f64 sqrt and division: thousands of isolated random pairs and triples."""
    rng = np.random.default_rng(1234)
    g = np.stack(np.meshgrid(np.arange(70), np.arange(70)), -1).reshape(-1, 2).astype(np.float64) * 10.0 - 350.0
    pairs = np.concatenate([g, g + rng.uniform(-1.4, 1.4, g.shape)])
    h = g + 5.0
    triples = np.concatenate([h, h + rng.uniform(-1.1, 1.1, h.shape), h + rng.uniform(-1.1, 1.1, h.shape)])
    xy = np.concatenate([pairs, triples]).astype(np.float32)
    xyz = np.c_[xy, np.zeros(len(xy), np.float32)]
    p = bev_amd.params_for_sensor("HDL_32E")
    ctx = bev_amd.BevContext(p, device=0, max_batch=1, max_points=len(xyz))
    try:
        got = ctx.normals_2d(xyz, 2.0)
        exp, nn = rl.normals(xyz, 2.0, want_nn=True)
        assert (nn == 2).sum() > 4000 and (nn == 3).sum() > 4000
        bad = np.nonzero((got.view(np.uint32) != exp.view(np.uint32)).any(axis=1))[0]
        assert len(bad) == 0, f"{len(bad)} normals differ, first {bad[:5]}: {got[bad[:3]]} vs {exp[bad[:3]]}"
    finally:
        ctx.close()


def test_edge_clouds():
    p = bev_amd.params_for_sensor("HDL_64E")
    rng = np.random.default_rng(99)
    one_cell = _cloud(np.c_[rng.uniform(-9, 9, 70000), rng.uniform(-9, 9, 70000), rng.uniform(0, 5, 70000)])
    ground = _cloud(rng.uniform(-50, 50, (5000, 3)), label=0)
    dup = _cloud(np.repeat(rng.uniform(-20, 20, (40, 3)), 30, axis=0))
    nanc = _cloud(np.c_[rng.normal(0, 10, 3000), rng.normal(0, 10, 3000), rng.uniform(0, 4, 3000)])
    nanc["x"][::7] = np.nan
    nanc["z"][3::11] = np.inf
    clouds = [_cloud(np.zeros((0, 3))), ground, _cloud([[1.0, 2.0, 3.0]]), one_cell, dup, nanc]
    ctx = bev_amd.BevContext(p, device=0, max_batch=4, max_points=len(one_cell))
    try:
        assert len(rl.top_part(one_cell)) == 14000  # > the 8192 keys a workgroup sorts in LDS: the global fallback
        for c in clouds:
            flat = ctx.top_part_flatten(c)
            assert _same(flat, rl.top_part(c))
            if len(flat):
                assert _same(ctx.voxel_grid(flat, 0.2), rl.voxel(flat, 0.2))
        got = ctx.registration_front(clouds)  # packed clouds, two sub-batches
        lens = []
        for c, g in zip(clouds, got):
            exp = rl.chain(c)
            assert _same(g, exp)
            lens.append(len(g))
        assert lens[0] == lens[1] == lens[2] == 0 and lens[3] > 1000 and lens[4] > 0 and lens[5] > 0
        # the voxel stage's global sort (> 8192 flattened points) and its overflow branch
        big = rl.top_part(one_cell)
        assert _same(ctx.voxel_grid(big, 0.05), rl.voxel(big, 0.05))
        assert _same(ctx.voxel_grid(big, 1e-4), rl.voxel(big, 1e-4))
        assert rl.voxel(big, 1e-4, want_info=True)[1][0] == 1
    finally:
        ctx.close()


def _upload(frames, dev):
    import torch

    offs = np.zeros(len(frames) + 1, np.uint64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    return offs, torch.from_numpy(np.concatenate(frames).view(np.uint8).reshape(-1)).to(dev)


def test_chain_on_1000_hdl64_frames_from_d_ordered():
    """bench.py's launch: 1000 HDL_64E sweeps in one bev_process_device_resident call, sub-batches of 500; the chain
    reads its d_ordered output directly.  Every frame's count and records against the checker."""
    import torch

    p = bev_amd.params_for_sensor("HDL_64E")
    F, SB, S = 1000, 500, p.slots
    dev = torch.device("cuda:0")
    def gen(i):
        f = synth.sweep(p, 40000 + i, keep=0.98, n_dup=5000)
        if i % 10 == 0:  # a sparse cell (9, 9): five points of upper beams (never ground) moved to x, y ~ 85 m
            hi = np.nonzero(f["row"] >= 56)[0][:5]
            f["x"][hi] = np.float32(85.0) + np.arange(len(hi), dtype=np.float32)
            f["y"][hi] = np.float32(85.0)
        return f

    with ThreadPoolExecutor(THREADS) as ex:
        frames = list(ex.map(gen, range(F)))
    offs, d_in = _upload(frames, dev)
    n_max = max(len(f) for f in frames)
    del frames
    d_ord = torch.zeros(F * S * 32, dtype=torch.uint8, device=dev)
    d_multi = torch.zeros(F * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    d_single = torch.zeros(F * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    stride = bev_amd.regfront_max_out(S)
    d_out = torch.full((F * stride * 12,), -1.0, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(F, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx = bev_amd.BevContext(p, device=0, max_batch=SB, max_points=n_max)
    try:
        ctx.process_device(F, d_in.data_ptr(), offs, d_ord.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
        ctx.registration_front_device(F, d_ord.data_ptr(), None, d_out.data_ptr(), stride, d_cnt.data_ptr())
        ctx.synchronize()
    finally:
        ctx.close()
    del d_in, d_multi, d_single
    cnt = d_cnt.cpu().numpy().astype(np.int64)
    bad, skipped, multi_vox, nn_seen = [], 0, 0, set()
    chunk = 100
    for f0 in range(0, F, chunk):
        ordered = d_ord[f0 * S * 32:(f0 + chunk) * S * 32].cpu().numpy().view(bev_amd.POINT_DTYPE).reshape(chunk, S)
        out = d_out[f0 * stride * 12:(f0 + chunk) * stride * 12].cpu().numpy().reshape(chunk, stride, 12)
        with ThreadPoolExecutor(THREADS) as ex:
            exp = list(ex.map(lambda i: rl.chain(ordered[i]), range(chunk)))
        for i in range(chunk):
            f = f0 + i
            if cnt[f] != len(exp[i]) or not _same(out[i, : cnt[f]], exp[i]):
                bad.append(f)
        skipped += sum(_skipped_cells(ordered[i]) > 0 for i in range(0, chunk, 10))
        if f0 == 0:  # coverage of the voxel and normal stages on a few frames
            for i in range(3):
                flat = rl.top_part(ordered[i])
                vox = rl.voxel(flat, 0.2)
                multi_vox += len(vox) < len(flat)
                nn_seen |= set(np.minimum(rl.normals(vox, 2.0, want_nn=True)[1], 3).tolist())
    assert not bad, f"{len(bad)} of {F} frames differ from the checker, first: {bad[:8]}"
    assert cnt.min() > 0
    assert skipped > 0 and multi_vox == 3 and {1, 2, 3} <= nn_seen, (skipped, multi_vox, nn_seen)


def test_chain_between_two_bev_calls_without_a_sync():
    """BEV call A -> the chain on A's d_ordered -> BEV call B writing into the SAME d_ordered, no synchronisation in
    between.  The chain must see A's finished labels (B waits for it), and B's outputs must still equal the oracle."""
    import torch

    p = bev_amd.params_for_sensor("HDL_32E")
    sp = orc.sensor_from_params(p)
    SB, N, S, M, L = 4, 14, p.slots, p.mat_size, p.n_layers
    dev = torch.device("cuda:0")
    fa = [synth.sweep(p, 51000 + i, keep=0.9, n_dup=200) for i in range(N)]
    fb = [synth.sweep(p, 52000 + i, keep=0.9, n_dup=200) for i in range(N)]
    oa, da = _upload(fa, dev)
    ob, db = _upload(fb, dev)
    d_ord = torch.zeros(N * S * 32, dtype=torch.uint8, device=dev)
    outs = [torch.zeros(N * k, dtype=torch.uint8, device=dev) for k in (L * M * M, M * M, L * M * M, M * M)]
    stride = bev_amd.regfront_max_out(S)
    d_out = torch.zeros(N * stride * 12, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(N, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx = bev_amd.BevContext(p, device=0, max_batch=SB, max_points=max(len(f) for f in fa + fb))
    try:
        ctx.process_device(N, da.data_ptr(), oa, d_ord.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr())
        ctx.registration_front_device(N, d_ord.data_ptr(), None, d_out.data_ptr(), stride, d_cnt.data_ptr())
        ctx.process_device(N, db.data_ptr(), ob, d_ord.data_ptr(), outs[2].data_ptr(), outs[3].data_ptr())
        ctx.synchronize()
    finally:
        ctx.close()
    ordered = d_ord.cpu().numpy().view(bev_amd.POINT_DTYPE).reshape(N, S)
    multi = [o.cpu().numpy() for o in outs]
    out = d_out.cpu().numpy().reshape(N, stride, 12)
    cnt = d_cnt.cpu().numpy()
    ref_a = [orc.process_frame(sp, f) for f in fa]
    ref_b = [orc.process_frame(sp, f) for f in fb]
    for i in range(N):
        oa_ord, _, oa_multi, oa_single = ref_a[i]
        ob_ord, _, ob_multi, ob_single = ref_b[i]
        assert ordered[i].tobytes() == ob_ord.tobytes(), f"frame {i}: call B's ordered cloud"
        assert multi[2][i * L * M * M:(i + 1) * L * M * M].tobytes() == np.ascontiguousarray(ob_multi).tobytes()
        assert multi[3][i * M * M:(i + 1) * M * M].tobytes() == np.ascontiguousarray(ob_single).tobytes()
        assert multi[0][i * L * M * M:(i + 1) * L * M * M].tobytes() == np.ascontiguousarray(oa_multi).tobytes()
        exp = rl.chain(oa_ord)
        assert cnt[i] == len(exp) and _same(out[i, : cnt[i]], exp), f"frame {i}: the chain did not see call A's labels"
