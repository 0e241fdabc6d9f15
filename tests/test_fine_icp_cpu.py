"""CPU: the fine-stage checker (tests/fineicp/fine_icp_oracle.c) against independent code — a numpy
restatement of VoxelGrid<PointXYZIRCT>, numpy.linalg.svd, a float64 Umeyama, brute-force nearest neighbours, known rigid
motions, crafted convergence states and the report maths — plus the fine-stage C ABI without a device."""
import ctypes as C
import math

import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
from bev_amd import POINT_DTYPE

F32 = np.float32


def _pts(xyz, intensity=None, label=None):
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    out = np.zeros(len(xyz), POINT_DTYPE)
    out["x"], out["y"], out["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if intensity is not None:
        out["intensity"] = intensity
    if label is not None:
        out["label"] = label
    return out


def _np_voxel(cloud, leaf):
    """VoxelGrid<PointXYZIRCT> restated in numpy / Python: float32 sums in input order, the label vote of a
    std::map<uint32_t, size_t>."""
    xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(F32)
    fin = np.isfinite(xyz).all(1)
    if not fin.any():
        return np.zeros(0, POINT_DTYPE)
    mn, mx = xyz[fin].min(0), xyz[fin].max(0)
    inv = F32(1.0) / F32(leaf)
    minb = np.floor(mn * inv).astype(np.int64)
    div = np.floor(mx * inv).astype(np.int64) - minb + 1
    ijk = (np.floor(xyz[fin] * inv) - minb.astype(F32)).astype(np.int64)
    idx = (ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]) % (1 << 32)
    order = np.flatnonzero(fin)
    vox = {}
    for k, i in zip(idx.tolist(), order.tolist()):
        vox.setdefault(k, []).append(i)
    out = np.zeros(len(vox), POINT_DTYPE)
    for o, k in enumerate(sorted(vox)):
        s = [F32(0)] * 4
        for i in vox[k]:
            for d, f in enumerate(("x", "y", "z", "intensity")):
                s[d] = F32(s[d] + cloud[f][i])
        n = F32(len(vox[k]))
        for d, f in enumerate(("x", "y", "z", "intensity")):
            out[f][o] = F32(s[d] / n)
        counts = {}
        for i in vox[k]:
            u = int(cloud["label"][i]) & 0xFFFFFFFF
            counts[u] = counts.get(u, 0) + 1
        best, lab = 0, 0
        for u in sorted(counts):
            if counts[u] > best:
                best, lab = counts[u], u
        out["label"][o] = np.int16(np.uint32(lab).astype(np.int64) - (1 << 32) if lab >= 1 << 31 else lab)
    return out


def test_voxel_irct_equals_a_numpy_restatement():
    rng = np.random.default_rng(1)
    n = 3000
    cloud = _pts(rng.uniform(-3, 3, (n, 3)), rng.uniform(0, 10, n).astype(F32), rng.integers(-4, 5, n))
    cloud["row"], cloud["col"], cloud["t"] = 3, 4, 5
    cloud["x"][::37] = np.nan
    got = fl.voxel_irct(cloud, 0.5)
    exp = _np_voxel(cloud, 0.5)
    assert got.tobytes() == exp.tobytes()
    assert (got["row"] == 0).all() and (got["t"] == 0).all() and (got["_pad0"] == 0).all()
    # ties: the smallest as uint32, so non-negative labels come before negative ones
    tie = _pts(np.zeros((6, 3)), None, [-1, -1, 2, 2, -3, -3])
    assert fl.voxel_irct(tie, 0.2)["label"].tolist() == [2]
    assert fl.voxel_irct(_pts(np.zeros((4, 3)), None, [-1, -1, -3, -3]), 0.2)["label"].tolist() == [-3]
    # empty slots of an ordered cloud (all-zero records) are one voxel at the origin
    ordered = np.zeros(100, POINT_DTYPE)
    v = fl.voxel_irct(ordered, 0.2)
    assert len(v) == 1 and v["x"][0] == 0 and v["label"][0] == 0
    # the "leaf size is too small" branch returns the input unchanged
    huge = _pts([[0, 0, 0], [1e6, 1e6, 1e6]], [1, 2], [1, 2])
    assert fl.voxel_irct(huge, 0.2).tobytes() == huge.tobytes()


def _check_svd(a):
    u, s, v, sweeps = fl.svd3(a)
    a = np.asarray(a, np.float64)
    assert sweeps < 64
    assert np.all(s >= 0) and np.all(np.diff(s) <= 0)
    assert np.allclose(u.T.astype(np.float64) @ u, np.eye(3), atol=1e-5)
    assert np.allclose(v.T.astype(np.float64) @ v, np.eye(3), atol=1e-5)
    scale = max(np.abs(a).max(), 1e-30)
    assert np.allclose(u.astype(np.float64) @ np.diag(s) @ v.T.astype(np.float64), a, atol=2e-5 * scale)
    assert np.allclose(s, np.linalg.svd(a, compute_uv=False), atol=2e-5 * scale)
    return u, s, v


def test_svd3_against_numpy():
    rng = np.random.default_rng(2)
    for _ in range(200):
        _check_svd(rng.normal(size=(3, 3)).astype(F32))
    x, y = rng.normal(size=3), rng.normal(size=3)
    _, s, _ = _check_svd(np.outer(x, y).astype(F32))  # rank 1
    assert s[1] < 1e-5 * s[0]
    b = rng.normal(size=(3, 2))
    _, s, _ = _check_svd((b @ rng.normal(size=(2, 3))).astype(F32))  # rank 2
    assert s[2] < 1e-5 * s[0]
    _check_svd(np.zeros((3, 3), F32))
    _check_svd(np.diag([1.0, -2.0, 3.0]).astype(F32))
    # a reflection: the rotation flips the last singular direction, so det(R) = +1
    refl = np.diag([1.0, 1.0, -1.0]).astype(F32)
    R = fl.rotation(refl)
    assert abs(np.linalg.det(R.astype(np.float64)) - 1.0) < 1e-5
    assert np.isnan(fl.rotation(np.full((3, 3), np.inf, F32))).all()


def _np_umeyama(src, dst):
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    ms, md = src.mean(0), dst.mean(0)
    sigma = (dst - md).T @ (src - ms) / len(src)
    u, _, vt = np.linalg.svd(sigma)
    S = np.eye(3)
    if np.linalg.det(u) * np.linalg.det(vt) < 0:
        S[2, 2] = -1
    R = u @ S @ vt
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, md - R @ ms
    return T


def test_umeyama_step_against_float64():
    rng = np.random.default_rng(3)
    for k in range(20):
        src = rng.uniform(-20, 20, (500, 3)).astype(F32)
        th = rng.uniform(-np.pi, np.pi)
        R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
        dst = (src @ R.T + rng.uniform(-5, 5, 3) + rng.normal(0, 0.05, (500, 3))).astype(F32)
        assert np.allclose(fl.umeyama(src, dst), _np_umeyama(src, dst), atol=2e-4)


def test_nn_against_brute_force():
    rng = np.random.default_rng(4)
    tgt = _pts(np.round(rng.uniform(-5, 5, (800, 3)), 1))  # a lattice: many exact ties
    tgt["x"][::50] = np.nan
    q = np.round(rng.uniform(-7, 7, (300, 3)), 1).astype(F32)
    idx, dist = fl.nn(tgt, q)
    t = np.stack([tgt["x"], tgt["y"], tgt["z"]], 1)
    for k in range(len(q)):
        d = (q[k] - t).astype(F32)
        dd = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F32)
        dd[~np.isfinite(t).all(1)] = np.inf
        j = int(np.flatnonzero(dd == dd.min())[0])
        assert idx[k] == j and dist[k] == dd[j]


@pytest.mark.parametrize("yaw,tx,ty", [(0.0, 0.3, -0.2), (4.0, -0.5, 0.4), (-7.0, 0.8, 0.1), (10.0, 0.0, -0.7)])
def test_icp_recovers_a_known_rigid_motion(yaw, tx, ty):
    """target = R source + t: the checker's loop, not only its pieces, finds the motion (the GPU is compared to it byte
    for byte, so this guards against a bug both share)."""
    rng = np.random.default_rng(int(yaw * 10) & 0xFFFF)
    # a structured scene: ground, walls, pillars (well-conditioned for point-to-point ICP)
    g = rng.uniform(-15, 15, (3000, 2))
    ground = np.c_[g, rng.normal(0, 0.02, 3000)]
    w1 = np.c_[rng.uniform(-15, 15, 800), np.full(800, 8.0), rng.uniform(0, 3, 800)]
    w2 = np.c_[np.full(800, -6.0), rng.uniform(-15, 15, 800), rng.uniform(0, 3, 800)]
    p = np.c_[rng.normal(3, 0.3, 500), rng.normal(-4, 0.3, 500), rng.uniform(0, 4, 500)]
    src = np.r_[ground, w1, w2, p].astype(F32)
    th = math.radians(yaw)
    R = np.array([[math.cos(th), -math.sin(th), 0], [math.sin(th), math.cos(th), 0], [0, 0, 1]])
    tgt = (src.astype(np.float64) @ R.T + [tx, ty, 0.05]).astype(F32)
    guess = fl.tool_guess(F32(yaw + 1.5))  # a yaw guess 1.5 degrees off, no translation
    r = fl.run(src, tgt, guess, fl.params(**fl.WHOLE))
    T = np.asarray(r["T"], np.float64).reshape(4, 4)
    assert r["converged"] == 1
    assert np.abs(T[:3, 3] - [tx, ty, 0.05]).max() < 1e-3
    assert abs(math.atan2(T[1, 0], T[0, 0]) - th) < 1e-4
    assert r["fitness"] < 1e-6


def test_states_on_crafted_inputs():
    rng = np.random.default_rng(5)
    a = rng.uniform(-10, 10, (2000, 3)).astype(F32)
    b = (a + F32(0.2)).astype(F32)
    assert fl.run(a, b + F32(100))["state"] == bev_amd.ICP_NO_CORRESPONDENCES
    assert fl.run(a[:2], b[:2])["state"] == bev_amd.ICP_NO_CORRESPONDENCES
    assert fl.run(a, b, None, fl.params(max_iterations=1))["state"] == bev_amd.ICP_ITERATIONS
    assert fl.run(a, a)["state"] == bev_amd.ICP_TRANSFORM  # the first increment is the identity
    r = fl.run(a, (a + rng.normal(0, 0.05, a.shape)).astype(F32), None,
               fl.params(euclidean_fitness_epsilon=0.5, transformation_epsilon=0.0))
    assert r["state"] == bev_amd.ICP_REL_MSE
    nan = a.copy()
    nan[:, 0] = np.nan
    r = fl.run(nan, b)
    assert r["state"] == bev_amd.ICP_NO_CORRESPONDENCES and r["fitness"] == np.finfo(np.float64).max


def test_report_maths_against_numpy():
    rng = np.random.default_rng(6)
    for _ in range(100):
        def T(yaw, tx, ty):
            m = np.eye(4, dtype=F32)
            c, s = np.cos(yaw), np.sin(yaw)
            m[:2, :2] = [[c, -s], [s, c]]
            m[0, 3], m[1, 3] = tx, ty
            return m
        a, b = rng.uniform(-np.pi, np.pi, 2)
        Tf, Tc = T(a, *rng.uniform(-3, 3, 2)), T(b, *rng.uniform(-3, 3, 2))
        xy, yaw = fl.report(Tf, Tc)
        assert abs(xy - np.hypot(Tf[0, 3] - Tc[0, 3], Tf[1, 3] - Tc[1, 3])) < 1e-5
        rel = np.linalg.inv(Tf[:3, :3].astype(np.float64)) @ Tc[:3, :3]
        exp = math.degrees(math.atan2(rel[1, 0], rel[0, 0]))
        assert abs(((yaw - exp) + 180) % 360 - 180) < 1e-3 and -180 <= yaw <= 180
        assert np.allclose(fl.inverse3(Tf[:3, :3]), np.linalg.inv(Tf[:3, :3].astype(np.float64)), atol=1e-5)
    # rotationMatrixToEulerAngles: the singular branch sets z = 0
    e = fl.euler(np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], F32))
    assert e[2] == 0.0 and abs(e[1] - np.pi / 2) < 1e-6
    assert fl.report_line(np.eye(4), np.eye(4)) == "0 0\n"


def test_defaults_and_exported_symbols():
    f, w = bev_amd.icp_fine_defaults(), bev_amd.icp_whole_defaults()
    assert (f.max_correspondence_distance, f.transformation_epsilon, f.euclidean_fitness_epsilon, f.max_iterations) == \
        (1.0, 1e-6, 0.01, 100)
    assert (w.max_correspondence_distance, w.transformation_epsilon, w.euclidean_fitness_epsilon, w.max_iterations) == \
        (4.0, 1e-6, 0.001, 200)
    lib = bev_amd.load_lib()
    for s in ("bev_voxel_grid_irct", "bev_icp_fine_defaults", "bev_icp_whole_defaults", "bev_icp_point_to_point",
              "bev_fine_registration_device_resident"):
        assert s in bev_amd.ABI_SYMBOLS and hasattr(lib, s)


def test_null_context_and_invalid_arguments_without_a_device():
    lib = bev_amd.load_lib()
    prm = bev_amd.icp_fine_defaults()
    res = np.zeros(1, bev_amd.ICP_RESULT_DTYPE)
    out = np.zeros(4, POINT_DTYPE)
    n = C.c_uint32(0)
    assert lib.bev_voxel_grid_irct(None, out.ctypes.data, 1, 0.2, out.ctypes.data, C.byref(n)) == -1
    assert lib.bev_icp_point_to_point(None, None, 0, None, 0, None, C.byref(prm), res.ctypes.data) == -1
    assert lib.bev_fine_registration_device_resident(None, 0, None, None, 0.2, 0, None, None, None, None, None) == -1
    bad = bev_amd.icp_fine_defaults()
    bad.max_correspondence_distance = float("nan")
    assert lib.bev_icp_point_to_point(None, None, 0, None, 0, None, C.byref(bad), res.ctypes.data) == -1
