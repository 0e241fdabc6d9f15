"""GPU: the coarse point-to-plane ICP (bev_icp.h) byte for byte against the sequential checker tests/icp/icp_oracle.c —
per problem on edge cases, and the batched device-resident entry over the registration front end's output of 1000
HDL_64E frames, also between unsynchronised BEV calls."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bev_amd
import icp_lib as il
import regfront_lib as rl
from bev_amd import synth

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 4)
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _checker():
    il.build()
    rl.build()


def _pn(xyz, nrm=None):
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    out = np.zeros((len(xyz), 12), F32)
    out[:, :3] = xyz
    if nrm is not None:
        out[:, 4:7] = np.asarray(nrm, F32).reshape(-1, 3)
    return out


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _cloud(rng, n, spread=30.0):
    xy = rng.uniform(-spread, spread, (n, 2)).astype(F32)
    ang = rng.uniform(0, 2 * np.pi, n)
    return _pn(np.c_[xy, np.zeros(n, F32)], np.c_[np.cos(ang), np.sin(ang), np.zeros(n)])


def test_per_problem_edge_cases_equal_the_checker():
    rng = np.random.default_rng(11)
    p = bev_amd.params_for_sensor("HDL_32E")
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=1000)
    try:
        a = _cloud(rng, 3000)
        b = a.copy()
        b[:, :2] += F32(0.4)
        nan_n = b.copy()
        nan_n[::3, 4:7] = np.nan  # |N| = 1 normals
        bad = a.copy()
        bad[::7, rng.integers(0, 3)] = np.nan
        bad[1::11, 0] = np.inf
        g = np.stack(np.meshgrid(np.arange(-8, 9), np.arange(-8, 9)), -1).reshape(-1, 2).astype(F32)
        grid = _pn(np.c_[g, np.zeros(len(g), F32)], np.tile([[1.0, 0, 0], [0, 1.0, 0]], (len(g) // 2 + 1, 1))[: len(g)])
        ties = _pn(np.c_[g + F32(0.5), np.zeros(len(g), F32)])  # every query equidistant from 4 grid points
        guess = il.tool_guess(37.5, 1)
        guess[:3, 3] = [1.5, -2.0, 0.25]
        cases = [
            ("empty target", a, a[:0], None),
            ("empty source", a[:0], a, None),
            ("single target point", a, a[:1], None),
            ("single source point", a[:1], a, None),
            ("two correspondences", a[:2], a, None),
            ("NaN target normals", a, nan_n, None),
            ("non-finite points", bad, np.concatenate([bad, a[:50]]), None),
            ("equal-distance ties", ties, grid, None),
            ("non-identity guess", b, a, guess),
            ("3-D clouds", _pn(rng.uniform(-20, 20, (2000, 3)), rng.normal(size=(2000, 3))),
             _pn(rng.uniform(-20, 20, (2500, 3)), rng.normal(size=(2500, 3))), None),
        ]
        for name, s_, t_, g_ in cases:
            got = ctx.icp_point_to_plane(s_, t_, g_)
            exp = il.run(s_, t_, g_)
            assert _same(got, exp), f"{name}: {got} != {exp}"
        prm = bev_amd.icp_params(max_correspondence_distance=0.7, max_iterations=25, transformation_epsilon=1e-9,
                                 euclidean_fitness_epsilon=1e-4)
        assert _same(ctx.icp_point_to_plane(b, a, None, prm), il.run(b, a, None, prm))
    finally:
        ctx.close()


def _front_end(F=1000):
    p = bev_amd.params_for_sensor("HDL_64E")
    import torch

    with ThreadPoolExecutor(THREADS) as ex:
        frames = list(ex.map(lambda i: synth.sweep(p, 300 + i, keep=0.98, n_dup=5000), range(F)))
    offs = np.zeros(F + 1, np.uint64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(np.concatenate(frames).view(np.uint8).reshape(-1)).to(dev)
    n_max = max(len(f) for f in frames)
    S = p.slots
    d_ord = torch.empty(F * S * 32, dtype=torch.uint8, device=dev)
    d_multi = torch.empty(F * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    d_single = torch.empty(F * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    stride = bev_amd.regfront_max_out(S)
    d_pn = torch.zeros(F * stride * 12, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(F, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx = bev_amd.BevContext(p, device=0, max_batch=500, max_points=n_max)
    return dict(p=p, F=F, ctx=ctx, d_in=d_in, offs=offs, d_ord=d_ord, d_multi=d_multi, d_single=d_single, d_pn=d_pn,
                d_cnt=d_cnt, stride=stride, torch=torch, dev=dev)


def _matches(F, seed=5):
    rng = np.random.default_rng(seed)
    m = np.zeros(2 * F, bev_amd.MATCH_DTYPE)
    m["query_idx"] = np.r_[np.arange(F), np.arange(F)]
    m["match_idx"] = np.r_[(np.arange(F) + 1) % F, rng.integers(0, F, F)]
    m["angle_guess"] = rng.uniform(-180, 180, 2 * F).astype(F32)
    m["angle_guess"][: F // 2] = rng.uniform(-3, 3, F // 2)  # near the truth (consecutive frames): proper registrations
    return m


def test_batched_1000_frames_every_result_equals_the_checker():
    e = _front_end()
    torch, ctx, F = e["torch"], e["ctx"], e["F"]
    try:
        ctx.process_device(F, e["d_in"].data_ptr(), e["offs"], e["d_ord"].data_ptr(), e["d_multi"].data_ptr(),
                           e["d_single"].data_ptr())
        ctx.registration_front_device(F, e["d_ord"].data_ptr(), None, e["d_pn"].data_ptr(), e["stride"],
                                      e["d_cnt"].data_ptr())
        m = _matches(F)
        n = len(m)
        d_res = torch.zeros(n * 2 * bev_amd.ICP_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=e["dev"])
        d_best = torch.full((n,), -7, dtype=torch.int32, device=e["dev"])
        ctx.coarse_registration_device(F, e["d_pn"].data_ptr(), e["stride"], e["d_cnt"].data_ptr(), m,
                                       d_res.data_ptr(), d_best.data_ptr())
        ctx.synchronize()
        got = d_res.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE).reshape(n, 2)
        best = d_best.cpu().numpy()
        cnt = e["d_cnt"].cpu().numpy()
        pn = e["d_pn"].cpu().numpy().reshape(F, e["stride"], 12)
        clouds = [pn[f, : cnt[f]] for f in range(F)]
        exp, exp_best = il.coarse(clouds, m, threads=THREADS)
        bad = [k for k in range(n) if not _same(got[k], exp[k])]
        assert not bad, f"{len(bad)} of {n} matches differ, first {bad[0]}: {got[bad[0]]} != {exp[bad[0]]}"
        assert np.array_equal(best, exp_best)
        states = np.bincount(got["state"].reshape(-1), minlength=6)
        assert states[bev_amd.ICP_ITERATIONS] > 0 and (best == 0).any() and (best == 1).any()

        # the same call between two unsynchronised BEV calls, right behind the front end: the same bytes
        d_res2 = torch.zeros_like(d_res)
        d_best2 = torch.full_like(d_best, -7)
        e["d_pn"].zero_()
        torch.cuda.synchronize()
        ctx.process_device(F, e["d_in"].data_ptr(), e["offs"], e["d_ord"].data_ptr(), e["d_multi"].data_ptr(),
                           e["d_single"].data_ptr())
        ctx.registration_front_device(F, e["d_ord"].data_ptr(), None, e["d_pn"].data_ptr(), e["stride"],
                                      e["d_cnt"].data_ptr())
        ctx.coarse_registration_device(F, e["d_pn"].data_ptr(), e["stride"], e["d_cnt"].data_ptr(), m,
                                       d_res2.data_ptr(), d_best2.data_ptr())
        ctx.process_device(F, e["d_in"].data_ptr(), e["offs"], e["d_ord"].data_ptr(), e["d_multi"].data_ptr(),
                           e["d_single"].data_ptr())
        ctx.synchronize()
        assert _same(d_res2.cpu().numpy(), d_res.cpu().numpy())
        assert _same(d_best2.cpu().numpy(), best)

        # the host convenience on the same clouds
        r3, b3 = ctx.coarse_registration(clouds[:40], [(i, (i + 1) % 40, float(m["angle_guess"][i])) for i in range(40)])
        e3, eb3 = il.coarse(clouds[:40], [(i, (i + 1) % 40, float(m["angle_guess"][i])) for i in range(40)],
                            threads=THREADS)
        assert _same(r3, e3) and np.array_equal(b3, eb3)
    finally:
        ctx.close()


def test_invalid_arguments_launch_nothing():
    import torch

    p = bev_amd.params_for_sensor("HDL_32E")
    ctx = bev_amd.BevContext(p, device=0, max_batch=2, max_points=1000)
    try:
        dev = torch.device("cuda:0")
        pn = torch.zeros(4 * 10 * 12, dtype=torch.float32, device=dev)
        cnt = torch.full((4,), 10, dtype=torch.int32, device=dev)
        res = torch.zeros(2 * bev_amd.ICP_RESULT_DTYPE.itemsize * 2, dtype=torch.uint8, device=dev)
        sentinel = torch.full((2,), -7, dtype=torch.int32, device=dev)
        ok = np.array([(0, 1, 0.0), (3, 2, 5.0)], bev_amd.MATCH_DTYPE)
        bad_sets = [
            (np.array([(0, 4, 0.0)], bev_amd.MATCH_DTYPE), None),
            (np.array([(-1, 0, 0.0)], bev_amd.MATCH_DTYPE), None),
            (ok, bev_amd.icp_params(max_iterations=0)),
            (ok, bev_amd.icp_params(max_iterations=1001)),
            (ok, bev_amd.icp_params(max_correspondence_distance=0.0)),
            (ok, bev_amd.icp_params(max_correspondence_distance=float("nan"))),
            (ok, bev_amd.icp_params(max_correspondence_distance=float("inf"))),
        ]
        for mm, prm in bad_sets:
            with pytest.raises(bev_amd.BevError, match="status -1"):
                ctx.coarse_registration_device(4, pn.data_ptr(), 10, cnt.data_ptr(), mm, res.data_ptr(),
                                               sentinel.data_ptr(), prm)
        with pytest.raises(bev_amd.BevError, match="status -1"):
            ctx.icp_point_to_plane(np.zeros((3, 12), F32), np.zeros((3, 12), F32), None,
                                   bev_amd.icp_params(max_iterations=0))
        ctx.synchronize()
        assert not res.any() and (sentinel == -7).all()
        d = bev_amd.icp_coarse_defaults()
        assert (d.max_correspondence_distance, d.max_iterations, d.transformation_epsilon) == (10.0, 10, 0.0)
        assert d.euclidean_fitness_epsilon == -np.finfo(np.float64).max
    finally:
        ctx.close()
