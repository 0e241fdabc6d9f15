"""GPU: the fine stage (bev_fine.h) byte for byte against the sequential checker tests/fineicp/fine_icp_oracle.c —
VoxelGrid<PointXYZIRCT> on edge clouds and HDL_64E frames, point-to-point ICP on edge cases, and the batched
device-resident entry with both tools' settings over the BEV path's ordered clouds (half the pairs a frame against a
moved copy of the same sweep), its top-part guesses read from the coarse entry's device output, also between
unsynchronised BEV calls.  Covered here: uniform frames of S records, at most 200 matches and 200 distinct frames, so
one voxel group and one launch.  Ragged packed frames, more than 256 slots and 1024 problems, guesses from an uploaded
coarse table, skewed geometry and chunk-boundary sources are in test_registration_batch_gpu.py."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import icp_lib as il
from bev_amd import POINT_DTYPE, synth

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 4)
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _checker():
    fl.build()
    il.build()


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _pts(xyz, intensity=None, label=None):
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    out = np.zeros(len(xyz), POINT_DTYPE)
    out["x"], out["y"], out["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if intensity is not None:
        out["intensity"] = intensity
    if label is not None:
        out["label"] = label
    out["row"], out["col"], out["t"] = 7, 9, 11  # never accumulated: the voxels carry 0
    return out


def test_voxel_grid_irct_edge_clouds_equal_the_checker():
    rng = np.random.default_rng(3)
    p = bev_amd.params_for_sensor("HDL_64E")
    frames = [synth.sweep(p, 900 + i, keep=0.98, n_dup=3000) for i in range(3)]
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=max(len(f) for f in frames))
    try:
        n = 5000
        base = _pts(rng.uniform(-20, 20, (n, 3)), rng.uniform(0, 1, n), rng.integers(-3, 4, n))
        bad = base.copy()
        bad["x"][::7] = np.nan
        bad["z"][1::11] = np.inf
        one = _pts(np.full((40, 3), 0.05) + rng.uniform(0, 0.1, (40, 3)), rng.uniform(0, 1, 40),
                   np.r_[[-2] * 10, [5] * 10, [-1] * 10, [0] * 10])  # a four-way tie: 0 wins (smallest as uint32)
        neg = _pts(np.zeros((6, 3)), np.arange(6), [-5, -5, -7, -7, 3, 3])  # 3 wins; among negatives -7 < -5 as uint32
        onlyneg = _pts(np.zeros((4, 3)), None, [-5, -5, -7, -7])  # -7 (0xfff9) before -5 (0xfffb)
        huge = _pts(np.r_[rng.uniform(-1, 1, (50, 3)), [[1e6, 1e6, 1e6]]], rng.uniform(0, 1, 51), 1)  # overflow branch
        empty = _pts(np.zeros((0, 3)))
        allnan = _pts(np.full((10, 3), np.nan))
        ords = [ctx.process_batch([f], want_multi=False, want_single=False)[0][0] for f in frames]
        for name, cloud in [("random", base), ("non-finite", bad), ("one voxel", one), ("ties", neg), ("negative", onlyneg),
                            ("overflow", huge), ("empty", empty), ("all nan", allnan)] + \
                           [(f"hdl{i}", o) for i, o in enumerate(ords)] + [(f"hdl-raw{i}", f) for i, f in enumerate(frames)]:
            got = ctx.voxel_grid_irct(cloud, 0.2)
            exp = fl.voxel_irct(cloud, 0.2)
            assert len(got) == len(exp) and _same(got, exp), name
        assert fl.voxel_irct(one, 0.2)["label"].tolist() == [0]
        assert fl.voxel_irct(neg, 0.2)["label"].tolist() == [3]
        assert fl.voxel_irct(onlyneg, 0.2)["label"].tolist() == [-7]
        assert len(fl.voxel_irct(huge, 0.2)) == 51
    finally:
        ctx.close()


def test_point_to_point_edge_cases_equal_the_checker():
    rng = np.random.default_rng(7)
    p = bev_amd.params_for_sensor("HDL_32E")
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=1000)
    try:
        a = rng.uniform(-10, 10, (4000, 3)).astype(F32)
        c, s = np.cos(0.05), np.sin(0.05)
        R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], F32)
        b = (a @ R.T + np.array([0.3, -0.2, 0.05], F32)).astype(F32)
        bad = a.copy()
        bad[::9, 1] = np.nan
        bad[1::13, 2] = -np.inf
        line = np.c_[np.linspace(0, 5, 200), np.zeros(200), np.zeros(200)].astype(F32)
        plane = np.c_[rng.uniform(-5, 5, (500, 2)), np.zeros(500)].astype(F32)
        g = np.stack(np.meshgrid(np.arange(-6, 7), np.arange(-6, 7)), -1).reshape(-1, 2).astype(F32)
        grid = np.c_[g, np.zeros(len(g), F32)]
        ties = np.c_[g + F32(0.5), np.zeros(len(g), F32)]
        guess = np.eye(4, dtype=F32)
        guess[0, 3] = 0.1
        negz = np.eye(4, dtype=F32)
        negz[0, 1] = negz[2, 3] = -0.0  # an identity with -0: still the identity (value comparison)
        far = b + F32(50.0)
        whole = fl.params(**fl.WHOLE)
        cases = [
            ("moved", a, b, None, None), ("moved whole", a, b, None, whole), ("guess", a, b, guess, None),
            ("one iteration", a, b, None, fl.params(max_iterations=1)), ("non-finite", bad, b, None, None),
            ("non-finite target", a, bad, None, whole), ("collinear", line, line + F32(0.1), None, None),
            ("planar", plane, plane + F32(0.2), None, whole), ("ties", ties, grid, None, None),
            ("identity -0", a, b, negz, None), ("too far", a, far, None, None), ("two points", a[:2], b[:2], None, None),
            ("empty source", a[:0], b, None, None), ("empty target", a, b[:0], None, None),
        ]
        for name, src, tgt, gs, prm in cases:
            got = ctx.icp_point_to_point(src, tgt, gs, prm)
            exp = fl.run(src, tgt, gs, prm)
            assert _same(got, exp), f"{name}: {got} != {exp}"
        r = fl.run(a, b)
        assert r["converged"] == 1 and r["fitness"] < 1e-6
        assert fl.run(a, far)["state"] == bev_amd.ICP_NO_CORRESPONDENCES
        assert fl.run(a, b, None, fl.params(max_iterations=1))["state"] == bev_amd.ICP_ITERATIONS
    finally:
        ctx.close()


def _chain(F0=100, seed=21):
    """F0 HDL_64E sweeps and a moved copy of each (seeded yaw and translation by bev_transform_cloud), through the BEV
    path on the device; the matches: (i, F0 + i) with the yaw as angle guess, and (i, i + 1)."""
    import torch

    p = bev_amd.params_for_sensor("HDL_64E")
    rng = np.random.default_rng(seed)
    yaw = rng.uniform(-20, 20, F0).astype(F32)
    tr = rng.uniform(-1.5, 1.5, (F0, 2)).astype(F32)
    with ThreadPoolExecutor(THREADS) as ex:
        base = list(ex.map(lambda i: synth.sweep(p, 500 + i, keep=0.98, n_dup=2000), range(F0)))
    n_max = max(len(f) for f in base)
    ctx = bev_amd.BevContext(p, device=0, max_batch=100, max_points=n_max)
    moved = [ctx.transform_cloud(base[i], bev_amd.yaw_translate_matrix(float(tr[i, 0]), float(tr[i, 1]), 0.0,
                                                                       float(yaw[i]))) for i in range(F0)]
    frames = base + moved
    F = len(frames)
    offs = np.zeros(F + 1, np.uint64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(np.concatenate(frames).view(np.uint8).reshape(-1)).to(dev)
    S = p.slots
    d_ord = torch.empty(F * S * 32, dtype=torch.uint8, device=dev)
    d_multi = torch.empty(F * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    d_single = torch.empty(F * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    stride = bev_amd.regfront_max_out(S)
    d_pn = torch.zeros(F * stride * 12, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(F, dtype=torch.int32, device=dev)
    m = np.zeros(2 * F0, bev_amd.MATCH_DTYPE)
    m["query_idx"] = np.r_[np.arange(F0), np.arange(F0)]
    m["match_idx"] = np.r_[F0 + np.arange(F0), (np.arange(F0) + 1) % F0]
    m["angle_guess"] = np.r_[yaw + rng.uniform(-2, 2, F0).astype(F32), rng.uniform(-3, 3, F0).astype(F32)]
    torch.cuda.synchronize()
    return dict(p=p, F=F, S=S, ctx=ctx, d_in=d_in, offs=offs, d_ord=d_ord, d_multi=d_multi, d_single=d_single, d_pn=d_pn,
                d_cnt=d_cnt, stride=stride, torch=torch, dev=dev, m=m)


def _bev(e):
    e["ctx"].process_device(e["F"], e["d_in"].data_ptr(), e["offs"], e["d_ord"].data_ptr(), e["d_multi"].data_ptr(),
                            e["d_single"].data_ptr())


def test_batched_both_tools_equal_the_checker():
    e = _chain()
    torch, ctx, F, S, m = e["torch"], e["ctx"], e["F"], e["S"], e["m"]
    n = len(m)
    R = bev_amd.ICP_RESULT_DTYPE.itemsize
    try:
        _bev(e)
        ctx.registration_front_device(F, e["d_ord"].data_ptr(), None, e["d_pn"].data_ptr(), e["stride"],
                                      e["d_cnt"].data_ptr())
        d_coarse = torch.zeros(n * 2 * R, dtype=torch.uint8, device=e["dev"])
        d_best = torch.full((n,), -7, dtype=torch.int32, device=e["dev"])
        ctx.coarse_registration_device(F, e["d_pn"].data_ptr(), e["stride"], e["d_cnt"].data_ptr(), m,
                                       d_coarse.data_ptr(), d_best.data_ptr())
        d_top = torch.zeros(n * R, dtype=torch.uint8, device=e["dev"])
        d_whole = torch.zeros(n * R, dtype=torch.uint8, device=e["dev"])
        # straight behind the coarse entry, no host round trip: guesses from its device output
        ctx.fine_registration_device(F, e["d_ord"].data_ptr(), None, m, d_top.data_ptr(), d_coarse.data_ptr(),
                                     d_best.data_ptr())
        ctx.fine_registration_device(F, e["d_ord"].data_ptr(), None, m, d_whole.data_ptr(),
                                     params=bev_amd.icp_whole_defaults())
        ctx.synchronize()
        coarse = d_coarse.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE).reshape(n, 2)
        best = d_best.cpu().numpy()
        top = d_top.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE)
        whole = d_whole.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE)

        # the coarse results on the same context are the coarse checker's
        cnt = e["d_cnt"].cpu().numpy()
        pn = e["d_pn"].cpu().numpy().reshape(F, e["stride"], 12)
        exp_c, exp_b = il.coarse([pn[f, : cnt[f]] for f in range(F)], m, threads=THREADS)
        assert _same(coarse, exp_c) and np.array_equal(best, exp_b)

        ordered = e["d_ord"].cpu().numpy().view(POINT_DTYPE).reshape(F, S)
        guesses = [coarse[k, best[k]]["T"].reshape(4, 4) for k in range(n)]
        exp_top = fl.fine(ordered, m, guesses, fl.params(**fl.FINE), threads=THREADS)
        exp_whole = fl.fine(ordered, m, None, fl.params(**fl.WHOLE), threads=THREADS)
        for name, got, exp in (("top-part", top, exp_top), ("whole", whole, exp_whole)):
            bad = [k for k in range(n) if not _same(got[k], exp[k])]
            assert not bad, f"{name}: {len(bad)} of {n} differ, first {bad[0]}: {got[bad[0]]} != {exp[bad[0]]}"
        # the moved copies register: the fine transform is the motion applied before the BEV path
        F0 = n // 2
        ok = (whole["fitness"][:F0] <= 1.5).mean()
        assert ok > 0.9, ok
        assert np.bincount(whole["state"], minlength=6)[[bev_amd.ICP_TRANSFORM, bev_amd.ICP_REL_MSE]].sum() > 0

        # again between two unsynchronised BEV calls, right behind the front end and the coarse entry: the same bytes
        d_top2 = torch.zeros_like(d_top)
        d_coarse2 = torch.zeros_like(d_coarse)
        d_best2 = torch.full_like(d_best, -7)
        e["d_ord"].zero_()
        torch.cuda.synchronize()
        _bev(e)
        ctx.registration_front_device(F, e["d_ord"].data_ptr(), None, e["d_pn"].data_ptr(), e["stride"],
                                      e["d_cnt"].data_ptr())
        ctx.coarse_registration_device(F, e["d_pn"].data_ptr(), e["stride"], e["d_cnt"].data_ptr(), m,
                                       d_coarse2.data_ptr(), d_best2.data_ptr())
        ctx.fine_registration_device(F, e["d_ord"].data_ptr(), None, m, d_top2.data_ptr(), d_coarse2.data_ptr(),
                                     d_best2.data_ptr())
        _bev(e)
        ctx.synchronize()
        assert _same(d_top2.cpu().numpy(), d_top.cpu().numpy())
        assert _same(d_coarse2.cpu().numpy(), d_coarse.cpu().numpy())

        # the host convenience, packed clouds with offsets
        sub = [(i, (i + 1) % 8, 0.5) for i in range(8)]
        clouds = [ordered[f] for f in range(8)]
        got = ctx.fine_registration(clouds, sub, params=bev_amd.icp_whole_defaults())
        assert _same(got, fl.fine(clouds, sub, None, fl.params(**fl.WHOLE), threads=THREADS))
    finally:
        ctx.close()


def test_invalid_arguments_launch_nothing():
    p = bev_amd.params_for_sensor("HDL_32E")
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=1000)
    try:
        lib, h = ctx.lib, ctx._h
        m = np.zeros(1, bev_amd.MATCH_DTYPE)
        m["match_idx"] = 5
        prm = bev_amd.icp_fine_defaults()
        import ctypes as C

        assert lib.bev_fine_registration_device_resident(h, 2, C.c_void_p(16), None, 0.2, 1, m.ctypes.data, None, None,
                                                         C.byref(prm), C.c_void_p(16)) == -1
        m["match_idx"] = 1
        assert lib.bev_fine_registration_device_resident(h, 2, C.c_void_p(16), None, 0.0, 1, m.ctypes.data, None, None,
                                                         C.byref(prm), C.c_void_p(16)) == -1
        assert lib.bev_fine_registration_device_resident(h, 2, C.c_void_p(16), None, 0.2, 1, m.ctypes.data,
                                                         C.c_void_p(16), None, C.byref(prm), C.c_void_p(16)) == -1
        bad = bev_amd.icp_fine_defaults()
        bad.max_iterations = 0
        assert lib.bev_icp_point_to_point(h, None, 0, None, 0, None, C.byref(bad), C.c_void_p(16)) == -1
        out = np.zeros(1, POINT_DTYPE)
        n = C.c_uint32(0)
        assert lib.bev_voxel_grid_irct(h, out.ctypes.data, 1, float("nan"), out.ctypes.data, C.byref(n)) == -1
        assert lib.bev_fine_registration_device_resident(h, 0, None, None, 0.2, 0, None, None, None, None, None) == 0
    finally:
        ctx.close()
