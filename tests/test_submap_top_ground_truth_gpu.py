"""GPU: the coarse call against the thinned top part over the union (bev_submap_top_part_coarse_registration_device_resident;
DESIGN.md §6r) on the small seeded world of ground_truth_cases.py, against a plain float64 point-to-plane ICP in the manner of
§6o: per match, results[2m] at k = 1, 2, 3, 8 iterations equals the reference's iterate k from the yaw guess, the reference
being ref64_registration's loop (its nearest search, its distance rule, its composition) over the checker's target
(submap_top_cases.target: positions and recomputed normals) and the front end's rows of the query.

The bound is ground_truth_cases' own: FACTOR (8) times the largest distance, over the compared iterations, between that plain
code run in float32 and in float64, refused above CAP (1e-4).

One step is restated here: ref64_registration.plane_fit solves its 6 x 6 normal equations with numpy.linalg.solve, and on a
FLATTENED cloud (z = 0 and nz = 0 throughout) the columns of roll, pitch and z are exactly zero, so that call raises "Singular
matrix" before it returns anything.  _plane_fit below is that function with the one line replaced by the minimum-norm solution
(numpy.linalg.lstsq), which leaves the unobservable unknowns at 0, the rule the coarse stage documents for a non-positive pivot
(DESIGN.md §6c).  Everything else is the module's."""
import numpy as np
import pytest

import bev_amd
import ground_truth_cases as gt
import icp_lib
import ref64_registration as ref
import reg_cases as rc
import regfront_lib as rf
import submap_reg_cases as sc
import submap_top_cases as tc
from bev_amd import ICP_RESULT_DTYPE
from submap_reg_gpu_lib import R, _ctx, _dev, _offsets

pytestmark = pytest.mark.gpu
LEAF = 0.5
F32, F64 = np.float32, np.float64


def _plane_fit(s, t, n, dtype):
    """ref64_registration.plane_fit with the minimum-norm solution of its normal equations"""
    s, t, n = (np.asarray(a, dtype) for a in (s, t, n))
    A = np.concatenate([np.cross(s, n), n], axis=1)
    b = (n * (t - s)).sum(axis=1)
    x = np.linalg.lstsq(A.T @ A, A.T @ b, rcond=None)[0].astype(dtype)
    al, be, ga = x[0], x[1], x[2]
    rx = np.array([[1, 0, 0], [0, np.cos(al), -np.sin(al)], [0, np.sin(al), np.cos(al)]], dtype)
    ry = np.array([[np.cos(be), 0, np.sin(be)], [0, 1, 0], [-np.sin(be), 0, np.cos(be)]], dtype)
    rz = np.array([[np.cos(ga), -np.sin(ga), 0], [np.sin(ga), np.cos(ga), 0], [0, 0, 1]], dtype)
    T = np.eye(4, dtype=dtype)
    T[:3, :3] = rz @ ry @ rx
    T[:3, 3] = x[3:]
    return T


def _reference(src, target, angle, dtype, trace=None):
    tgt, nrm = np.asarray(target[:, :3], dtype), np.asarray(target[:, 4:7], dtype)
    return ref._loop(src[:, :3], tgt, ref.yaw_guess(angle, 0, dtype), gt.COARSE_D, max(gt.K),
                     lambda c, i: _plane_fit(c, tgt[i], nrm[i], dtype), dtype, trace)


def test_the_call_equals_the_float64_reference_iterates_on_the_checkers_target():
    import torch

    icp_lib.build()
    rf.build()
    S = gt.setup()
    clouds = S["clouds"]
    moffs, eframe, epose = gt.map_arrays(S)
    maps = sc.Maps()
    for g in range(len(moffs) - 1):
        maps.add([(int(eframe[e]), epose[e]) for e in range(int(moffs[g]), int(moffs[g + 1]))])
    m = gt.match_array(S)
    targets = tc.all_targets(clouds, maps, LEAF)
    assert all(len(t) > 100 and np.isfinite(t).all() for t in targets)     # the reference reads every normal
    pn = tc.queries(clouds)
    its, tols = [], []
    for q, g, a in S["matches"]:
        trace = []
        a64, a32 = _reference(pn[q], targets[g], a, F64, trace), _reference(pn[q], targets[g], a, F32)
        its.append((a64, trace))
        tols.append(gt.FACTOR * max(float(np.abs(a64[i - 1] - a32[i - 1].astype(F64)).max()) for i in gt.K))
        assert tols[-1] <= gt.CAP, (q, g, tols[-1])
    stride = max(len(p) for p in pn)
    dev = torch.device("cuda:0")
    ctx = _ctx(max_points=4096)
    try:
        d_clouds, d_pn = _dev(rc.packed(clouds)), _dev(rc.strided(pn, stride))
        d_cnt = _dev(np.array([len(p) for p in pn], np.uint32))
        for k in gt.K:
            d_res = torch.zeros(len(m) * 2 * R, dtype=torch.uint8, device=dev)
            d_best = torch.zeros(len(m) * 4, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            ctx.submap_top_part_coarse_registration_device(len(clouds), d_clouds.data_ptr(), _offsets(clouds), d_pn.data_ptr(), stride,
                                                           d_cnt.data_ptr(), moffs, eframe, epose, m, d_res.data_ptr(),
                                                           d_best.data_ptr(), LEAF, params=bev_amd.icp_params(max_iterations=k))
            ctx.synchronize()
            res = d_res.cpu().numpy().view(ICP_RESULT_DTYPE).reshape(-1, 2)
            for j in range(len(m)):
                rec, (it, trace) = res[j, 0], its[j]
                name = f"match {j}, k = {k}"
                state, n_it = int(rec["state"]), int(rec["iterations"])
                assert int(rec["converged"]) == 1, f"{name}: converged {rec['converged']}, state {state}"
                if state == bev_amd.ICP_ITERATIONS:
                    assert n_it == k, f"{name}: state ITERATIONS after {n_it} iterations, expected {k}"
                else:   # the one other end §6o admits: the absolute MSE test, where the reference's MSE has come to rest too
                    assert state == bev_amd.ICP_ABS_MSE and 2 <= n_it < k, f"{name}: state {state} after {n_it} iterations"
                    mse = [float(d2[keep].mean()) for _, _, d2, keep in trace]
                    assert abs(mse[n_it - 1] - mse[n_it - 2]) < 1e-11, f"{name}: {mse[n_it - 2]} -> {mse[n_it - 1]}"
                d = gt.dist(rec["T"], it[n_it - 1])
                print(f"{name}: {d:.1e}, tol {tols[j]:.1e}")
                assert d <= tols[j], f"{name}: {d:.3e} from the reference, tol {tols[j]:.3e}"
    finally:
        ctx.close()
