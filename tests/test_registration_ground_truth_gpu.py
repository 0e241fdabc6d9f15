"""GPU: the scan-to-map and pair registration calls against ground truth and a plain float64 ICP.  Every
comparison is with ref64_registration.py's iterates or with T_true = P_map^-1 P_q of ground_truth_cases.py, within the
tolerance that the reference alone sets (8 times float32 against float64 of the same plain code; the CPU file asserts the
conditions on the inputs) - never with a checker:

  1. the coarse call against maps: results[2m] at k = 1, 2, 3, 8 iterations equals the reference's iterate from the yaw guess;
     at the defaults it equals T_true and guess 0 is the better one;
  2. the fine calls (bev_submap_registration_device_resident, bev_submap_voxel_registration_device_resident at map_leaf 0 and
     0.2) at the same k: D 1 from a made-up coarse table whose chosen record is T_true perturbed, D 4 from the yaw guess; the
     tools' own settings against T_true; at map_leaf 0.2 the thinned cloud as a set equals the distinct visible world points;
  3. coarse and fine chained without a synchronisation: T_true;
  4. the pair calls on map C's frames against the same reference;
  5. the batch forms against T_true.

What the device measured on an MI355X is in DESIGN.md §6o."""
import numpy as np
import pytest

import bev_amd
import ground_truth_cases as gt
import ref64_registration as ref
import reg_cases as rc
from bev_amd import ICP_RESULT_DTYPE, MATCH_DTYPE
from submap_reg_gpu_lib import F32, R, _ctx, _dev, _fine_call, _offsets, _results

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    return gt.precompute()


def _near(name, T, want, tol):
    d = gt.dist(T, want)
    print(f"{name}: {d:.1e}, tol {tol:.1e}")
    assert d <= tol, f"{name}: {d:.3e} from the reference, tol {tol:.3e}:\n{np.asarray(T).reshape(4, 4)}\n!=\n{want}"


def _coarse_upload(S):
    stride = max(len(r) for r in S["rows"])
    return _dev(rc.strided(S["rows"], stride)), _dev(np.array([len(r) for r in S["rows"]], np.uint32)), stride


def _coarse_outputs(n):
    import torch

    dev = torch.device("cuda:0")
    return torch.zeros(n * 2 * R, dtype=torch.uint8, device=dev), torch.zeros(n * 4, dtype=torch.uint8, device=dev)


def _read_coarse(d_res, d_best, n):
    return d_res.cpu().numpy().view(ICP_RESULT_DTYPE).reshape(-1, 2)[:n], d_best.cpu().numpy().view(np.int32)[:n]


# ---- 1. coarse against maps -----------------------------------------------------------------------------------------------------------
def test_the_coarse_call_equals_the_reference_iterates_and_the_truth(S):
    import torch

    m, maps = gt.match_array(S), gt.map_arrays(S)
    ctx = _ctx(max_points=4096)
    try:
        d_pn, d_cnt, stride = _coarse_upload(S)

        def call(prm):
            d_res, d_best = _coarse_outputs(len(m))
            torch.cuda.synchronize()
            ctx.submap_coarse_registration_device(len(S["rows"]), d_pn.data_ptr(), stride, d_cnt.data_ptr(), *maps, m, d_res.data_ptr(),
                                                  d_best.data_ptr(), prm)
            ctx.synchronize()
            return _read_coarse(d_res, d_best, len(m))

        for k in gt.K:
            res, _ = call(bev_amd.icp_params(max_iterations=k))
            for j in range(len(m)):
                name = f"coarse, match {j}, k = {k}"
                _near(name, res[j, 0]["T"], gt.compared_iterate(name, res[j, 0], j, "coarse", k), gt.tol(j, "coarse"))
        res, best = call(None)
        for j in range(len(m)):
            _near(f"coarse defaults, match {j}, from T_true", res[j, 0]["T"], S["truth"][j], gt.tol(j, "coarse"))
            assert res[j, 0]["converged"] == 1 and best[j] == 0 and res[j, 1]["fitness"] >= 10 * res[j, 0]["fitness"], (j, res[j], best[j])
    finally:
        ctx.close()


# ---- 2. fine against maps -------------------------------------------------------------------------------------------------------------
def _cloud_as_a_set(ctx, S, d_clouds, maps, map_leaf):
    """the thinned targets of the three maps against the distinct world points their entries see, in the map frame"""
    import torch

    stride = max(sum(len(S["clouds"][f]) for f in frames) for _, frames in S["maps"])
    dev = torch.device("cuda:0")
    d_out = torch.zeros(len(S["maps"]) * stride * 16, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(len(S["maps"]), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.submap_voxel_cloud_device(len(S["clouds"]), d_clouds.data_ptr(), _offsets(S["clouds"]), *maps, map_leaf, stride,
                                  d_out.data_ptr(), d_cnt.data_ptr())
    ctx.synchronize()
    out, cnt = d_out.cpu().numpy().view(F32).reshape(len(S["maps"]), stride, 4), d_cnt.cpu().numpy()
    for g in range(len(S["maps"])):
        ids, tx, _ = gt.ref_target(S, g)
        rows = out[g, : cnt[g], :3].astype(np.float64)
        idx, _ = ref.nearest(rows, tx)
        off = float(np.abs(rows - tx[idx]).max())
        bound = 16 * float(np.spacing(F32(np.abs(tx).max())))
        print(f"map {g}: {cnt[g]} rows for {len(ids)} distinct world points, the farthest row {off:.2e} from its point, bound {bound:.2e}")
        assert (out[g, : cnt[g], 3] == 0).all() and cnt[g] >= len(ids)
        assert off <= bound, f"map {g}: a row {off} from every visible world point"
        assert len(np.unique(idx)) == len(ids), f"map {g}: {len(ids) - len(np.unique(idx))} visible world points have no row"


@pytest.mark.parametrize("map_leaf", [None, 0.0, 0.2])
def test_the_fine_calls_equal_the_reference_iterates_and_the_truth(S, map_leaf):
    m, maps = gt.match_array(S), gt.checker_maps(S)
    coarse, best = gt.coarse_table(S)
    ctx = _ctx(max_points=4096)
    try:
        d_clouds = _dev(rc.packed(S["clouds"]))
        for setting, D, table in (("fine", gt.FINE_D, (coarse, best)), ("whole", gt.WHOLE_D, (None, None))):
            for k in gt.K:
                res = _fine_call(ctx, S["clouds"], maps, m, gt.fixed_params(D, k), map_leaf, d_clouds, *table)
                for j in range(len(m)):
                    name = f"{setting}, map_leaf {map_leaf}, match {j}, k = {k}"
                    _near(name, res[j]["T"], gt.compared_iterate(name, res[j], j, setting, k), gt.tol(j, setting))
        for setting, prm, table in (("fine", bev_amd.icp_fine_defaults(), (coarse, best)), ("whole", bev_amd.icp_whole_defaults(), (None, None))):
            res = _fine_call(ctx, S["clouds"], maps, m, prm, map_leaf, d_clouds, *table)
            for j in range(len(m)):
                _near(f"{setting} settings, map_leaf {map_leaf}, match {j}, from T_true", res[j]["T"], S["truth"][j], gt.tol(j, setting))
                assert res[j]["converged"] == 1, res[j]
        if map_leaf:
            _cloud_as_a_set(ctx, S, d_clouds, gt.map_arrays(S), map_leaf)
    finally:
        ctx.close()


# ---- 3. the chain ---------------------------------------------------------------------------------------------------------------------
def test_coarse_and_fine_chained_without_a_synchronisation_give_the_truth(S):
    import torch

    m, maps = gt.match_array(S), gt.map_arrays(S)
    ctx = _ctx(max_points=4096)
    try:
        d_pn, d_cnt, stride = _coarse_upload(S)
        d_clouds = _dev(rc.packed(S["clouds"]))
        d_res, d_best = _coarse_outputs(len(m))
        d_fine = torch.zeros(len(m) * R, dtype=torch.uint8, device=d_clouds.device)
        torch.cuda.synchronize()
        ctx.submap_coarse_registration_device(len(S["rows"]), d_pn.data_ptr(), stride, d_cnt.data_ptr(), *maps, m, d_res.data_ptr(),
                                              d_best.data_ptr())
        ctx.submap_voxel_registration_device(len(S["clouds"]), d_clouds.data_ptr(), _offsets(S["clouds"]), *maps, m, d_fine.data_ptr(),
                                             0.2, d_res.data_ptr(), d_best.data_ptr())
        ctx.synchronize()
        _, best = _read_coarse(d_res, d_best, len(m))
        fine = _results(d_fine)[: len(m)]
        for j in range(len(m)):
            _near(f"the chain, match {j}, from T_true", fine[j]["T"], S["truth"][j], gt.tol(j, "fine"))
            assert fine[j]["converged"] == 1 and best[j] == 0, (fine[j], best[j])
    finally:
        ctx.close()


# ---- 4. the pair calls on map C's frames ------------------------------------------------------------------------------------------------
def test_the_pair_calls_equal_the_reference_on_the_one_entry_map(S):
    import torch

    pairs = [j for j, (_, g, _) in enumerate(S["matches"]) if len(S["maps"][g][1]) == 1]
    assert len(pairs) == 2 and all(S["maps"][S["matches"][j][1]] == (3, [3]) for j in pairs)
    m = np.array([(S["matches"][j][0], 3, S["matches"][j][2]) for j in pairs], MATCH_DTYPE)
    coarse, best = gt.coarse_table(S)
    coarse, best = coarse[pairs], best[pairs]
    ctx = _ctx(max_points=4096)
    try:
        d_pn, d_cnt, stride = _coarse_upload(S)
        d_clouds = _dev(rc.packed(S["clouds"]))
        offs = _offsets(S["clouds"])

        def coarse_call(prm):
            d_res, d_best = _coarse_outputs(len(m))
            torch.cuda.synchronize()
            ctx.coarse_registration_device(len(S["rows"]), d_pn.data_ptr(), stride, d_cnt.data_ptr(), m, d_res.data_ptr(), d_best.data_ptr(), prm)
            ctx.synchronize()
            return _read_coarse(d_res, d_best, len(m))

        def fine_call(prm, table):
            d_res = torch.zeros(len(m) * R, dtype=torch.uint8, device=d_clouds.device)
            d_c, d_b = (_dev(table[0]), _dev(table[1])) if table[0] is not None else (None, None)
            torch.cuda.synchronize()
            ctx.fine_registration_device(len(S["clouds"]), d_clouds.data_ptr(), offs, m, d_res.data_ptr(),
                                         d_c.data_ptr() if d_c is not None else None, d_b.data_ptr() if d_b is not None else None, params=prm)
            ctx.synchronize()
            return _results(d_res)[: len(m)]

        for k in gt.K:
            res, _ = coarse_call(bev_amd.icp_params(max_iterations=k))
            for i, j in enumerate(pairs):
                q, theta = S["matches"][j][0], S["matches"][j][2]
                name = f"pair coarse, match {j}, k = {k}"
                _near(name, res[i, 0]["T"], gt.compared_iterate(name, res[i, 0], j, "coarse", k), gt.tol(j, "coarse"))
                one = ctx.icp_point_to_plane(S["rows"][q], S["rows"][3], ref.yaw_guess(theta, 0), bev_amd.icp_params(max_iterations=k))
                name = f"icp_point_to_plane, match {j}, k = {k}"
                _near(name, one["T"], gt.compared_iterate(name, one, j, "coarse", k), gt.tol(j, "coarse"))
            for setting, D, table in (("fine", gt.FINE_D, (coarse, best)), ("whole", gt.WHOLE_D, (None, None))):
                res = fine_call(gt.fixed_params(D, k), table)
                for i, j in enumerate(pairs):
                    q = S["matches"][j][0]
                    name = f"pair {setting}, match {j}, k = {k}"
                    _near(name, res[i]["T"], gt.compared_iterate(name, res[i], j, setting, k), gt.tol(j, setting))
                    one = ctx.icp_point_to_point(S["clouds"][q], S["clouds"][3], gt.start(S, j, setting), gt.fixed_params(D, k))
                    name = f"icp_point_to_point {setting}, match {j}, k = {k}"
                    _near(name, one["T"], gt.compared_iterate(name, one, j, setting, k), gt.tol(j, setting))
        res, bst = coarse_call(None)
        fine = fine_call(bev_amd.icp_fine_defaults(), (coarse, best))
        whole = fine_call(bev_amd.icp_whole_defaults(), (None, None))
        for i, j in enumerate(pairs):
            q, theta = S["matches"][j][0], S["matches"][j][2]
            _near(f"pair coarse defaults, match {j}, from T_true", res[i, 0]["T"], S["truth"][j], gt.tol(j, "coarse"))
            _near(f"pair fine settings, match {j}, from T_true", fine[i]["T"], S["truth"][j], gt.tol(j, "fine"))
            _near(f"pair whole settings, match {j}, from T_true", whole[i]["T"], S["truth"][j], gt.tol(j, "whole"))
            plane = ctx.icp_point_to_plane(S["rows"][q], S["rows"][3], ref.yaw_guess(theta, 0))
            point = ctx.icp_point_to_point(S["clouds"][q], S["clouds"][3], gt.perturbed(S, j))
            _near(f"icp_point_to_plane defaults, match {j}, from T_true", plane["T"], S["truth"][j], gt.tol(j, "coarse"))
            _near(f"icp_point_to_point defaults, match {j}, from T_true", point["T"], S["truth"][j], gt.tol(j, "fine"))
            assert bst[i] == 0 and all(r["converged"] == 1 for r in (res[i, 0], fine[i], whole[i], plane, point))
    finally:
        ctx.close()


# ---- 5. the batch forms -----------------------------------------------------------------------------------------------------------------
def test_the_batch_forms_give_the_truth(S):
    m, maps = gt.match_array(S), gt.map_arrays(S)
    ctx = _ctx(max_points=4096)
    try:
        plain = ctx.submap_registration_batch(S["clouds"], *maps, m, params=bev_amd.icp_whole_defaults())
        thinned = ctx.submap_voxel_registration_batch(S["clouds"], *maps, m, 0.2, params=bev_amd.icp_whole_defaults())
    finally:
        ctx.close()
    for j in range(len(m)):
        _near(f"submap_registration_batch, match {j}, from T_true", plain[j]["T"], S["truth"][j], gt.tol(j, "whole"))
        _near(f"submap_voxel_registration_batch, match {j}, from T_true", thinned[j]["T"], S["truth"][j], gt.tol(j, "whole"))
        assert plain[j]["converged"] == 1 and thinned[j]["converged"] == 1
