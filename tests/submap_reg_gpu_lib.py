"""What the GPU tests of the scan-to-map entry points share (test_submap_registration_gpu.py,
test_submap_voxel_registration_gpu.py, test_submap_coarse_registration_gpu.py): byte-for-byte comparison,
uploads, a small context, and one synchronised call of the fine entries.  The cases and their expected values are in
submap_reg_cases.py, submap_vox_cases.py and submap_coarse_cases.py."""
import os

import numpy as np

import bev_amd
import reg_cases as rc
from bev_amd import ICP_RESULT_DTYPE

THREADS = min(16, os.cpu_count() or 4)
F32 = np.float32
R = ICP_RESULT_DTYPE.itemsize
OK, INVALID, TOO_LARGE = 0, -1, -6


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(name, got, exp):
    assert len(got) == len(exp), f"{name}: {len(got)} records, expected {len(exp)}"
    bad = [k for k in range(len(exp)) if not _same(got[k], exp[k])]
    assert not bad, f"{name}: {len(bad)} of {len(exp)} differ, first {bad[0]}: {got[bad[0]]} != {exp[bad[0]]}"


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(torch.device("cuda:0"))


def _results(d):
    return d.cpu().numpy().view(ICP_RESULT_DTYPE).reshape(-1)


def _ctx(sensor="HDL_32E", max_batch=2, max_points=1000):
    return bev_amd.BevContext(bev_amd.params_for_sensor(sensor), device=0, max_batch=max_batch, max_points=max_points)


def _offsets(clouds):
    offs = np.zeros(len(clouds) + 1, np.uint64)
    offs[1:] = np.cumsum([len(c) for c in clouds])
    return offs


def _fine_call(ctx, clouds, maps, m, prm, map_leaf, d_clouds=None, coarse=None, best=None, fill=0):
    """one device-resident call on packed clouds, synchronised: (n,) ICP_RESULT_DTYPE.  map_leaf None:
    bev_submap_registration_device_resident; a number: bev_submap_voxel_registration_device_resident"""
    import torch

    d_clouds = d_clouds if d_clouds is not None else _dev(rc.packed(clouds))
    d_res = torch.full((max(len(m), 1) * R,), fill, dtype=torch.uint8, device=d_clouds.device)
    d_coarse = _dev(coarse) if coarse is not None else None
    d_best = _dev(best) if best is not None else None
    tabs = (d_coarse.data_ptr() if d_coarse is not None else None, d_best.data_ptr() if d_best is not None else None)
    torch.cuda.synchronize()
    if map_leaf is None:
        ctx.submap_registration_device(len(clouds), d_clouds.data_ptr(), _offsets(clouds), *maps.arrays(), m, d_res.data_ptr(),
                                       *tabs, params=prm)
    else:
        ctx.submap_voxel_registration_device(len(clouds), d_clouds.data_ptr(), _offsets(clouds), *maps.arrays(), m,
                                             d_res.data_ptr(), map_leaf, *tabs, params=prm)
    ctx.synchronize()
    return _results(d_res)[: len(m)]
