"""GPU: verification on the ground-truth world of ground_truth_cases.py.  The scan-to-map call under the
whole tool's settings returns a motion within 1e-4 of the truth and the next world point is 0.36 m away, so under its result
every query point has a map point within 0.1, 0.2 and 0.3 m; under a record that is nowhere near, next to none has.  Map C's pair
form behaves likewise."""
import numpy as np
import pytest

import bev_amd
import ground_truth_cases as gt
import reg_cases as rc
from bev_amd import ICP_RESULT_DTYPE, MATCH_DTYPE, VERIFY_RESULT_DTYPE, verify_params

pytestmark = pytest.mark.gpu
TH = (0.1, 0.2, 0.3)
R, V = ICP_RESULT_DTYPE.itemsize, VERIFY_RESULT_DTYPE.itemsize


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(torch.device("cuda:0"))


def _far_off(S, ks):
    res = np.zeros(len(ks), ICP_RESULT_DTYPE)
    for i, k in enumerate(ks):
        res["T"][i] = gt.far_off(S, k).reshape(16)
    return res


def _judge(name, ver, n_points):
    for k, v in enumerate(ver):
        share = v["query_within"][:3] / max(int(v["n_query"]), 1)
        print(f"{name}, match {k}: n_query {v['n_query']} n_target {v['n_target']} forward {share} reverse "
              f"{v['target_within'][:3] / max(int(v['n_target']), 1)}")
        assert v["n_query"] == n_points[k] > 1000


def test_verification_separates_the_truth_from_a_wrong_record():
    import torch

    S = gt.setup()
    m, maps = gt.match_array(S), gt.map_arrays(S)
    clouds = S["clouds"]
    offs = np.r_[0, np.cumsum([len(c) for c in clouds])].astype(np.uint64)
    prm = verify_params(TH)
    ctx = bev_amd.BevContext(bev_amd.params_for_sensor("HDL_64E"), device=0, max_batch=2, max_points=4096)
    try:
        dev = torch.device("cuda:0")
        d_clouds = _dev(rc.packed(clouds))
        d_res = torch.zeros(len(m) * R, dtype=torch.uint8, device=dev)
        d_ver, d_bad = (torch.zeros(len(m) * V, dtype=torch.uint8, device=dev) for _ in range(2))
        d_far = _dev(_far_off(S, range(len(m))))
        torch.cuda.synchronize()
        ctx.submap_voxel_registration_device(len(clouds), d_clouds.data_ptr(), offs, *maps, m, d_res.data_ptr(), 0.0,
                                             params=bev_amd.icp_whole_defaults())
        ctx.submap_verify_registration_device(len(clouds), d_clouds.data_ptr(), offs, *maps, m, d_res.data_ptr(), d_ver.data_ptr(), 0.0, prm)
        ctx.submap_verify_registration_device(len(clouds), d_clouds.data_ptr(), offs, *maps, m, d_far.data_ptr(), d_bad.data_ptr(), 0.0, prm)
        ctx.synchronize()
        res = d_res.cpu().numpy().view(ICP_RESULT_DTYPE)
        ver, bad = (d.cpu().numpy().view(VERIFY_RESULT_DTYPE) for d in (d_ver, d_bad))
        n_points = [len(clouds[int(q)]) for q in m["query_idx"]]
        _judge("maps, the call's result", ver, n_points)
        _judge("maps, far_off", bad, n_points)
        for k in range(len(m)):
            assert gt.dist(res[k]["T"], S["truth"][k]) <= 1e-4 and res[k]["converged"] == 1
            assert ver[k]["query_within"][:3].tolist() == [ver[k]["n_query"]] * 3
            assert bad[k]["query_within"][2] < 0.05 * bad[k]["n_query"]  # measured on the host in float64: at most 0.022
        # map C's pair form: the one-entry map's frame as the target frame
        pairs = [j for j, (_, g, _) in enumerate(S["matches"]) if len(S["maps"][g][1]) == 1]
        assert len(pairs) == 2
        pm = np.array([(S["matches"][j][0], 3, S["matches"][j][2]) for j in pairs], MATCH_DTYPE)
        d_pres = torch.zeros(len(pm) * R, dtype=torch.uint8, device=dev)
        d_pver, d_pbad = (torch.zeros(len(pm) * V, dtype=torch.uint8, device=dev) for _ in range(2))
        d_pfar = _dev(_far_off(S, pairs))
        torch.cuda.synchronize()
        ctx.fine_registration_device(len(clouds), d_clouds.data_ptr(), offs, pm, d_pres.data_ptr(), params=bev_amd.icp_whole_defaults())
        ctx.verify_registration_device(len(clouds), d_clouds.data_ptr(), offs, pm, d_pres.data_ptr(), d_pver.data_ptr(), prm)
        ctx.verify_registration_device(len(clouds), d_clouds.data_ptr(), offs, pm, d_pfar.data_ptr(), d_pbad.data_ptr(), prm)
        ctx.synchronize()
        pver, pbad = (d.cpu().numpy().view(VERIFY_RESULT_DTYPE) for d in (d_pver, d_pbad))
        n_points = [len(clouds[int(q)]) for q in pm["query_idx"]]
        _judge("pair, the call's result", pver, n_points)
        _judge("pair, far_off", pbad, n_points)
        for i, j in enumerate(pairs):
            assert pver[i].tobytes() == ver[j].tobytes()  # a one-entry map under the identity is its frame
            assert pver[i]["query_within"][:3].tolist() == [pver[i]["n_query"]] * 3
            assert pbad[i]["query_within"][2] < 0.05 * pbad[i]["n_query"]
    finally:
        ctx.close()
