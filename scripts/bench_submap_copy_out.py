"""The copy-out launch of the two scan-to-map cloud calls (K_SUBMAP_VOX_OUT, K_SUBMAP_PN_OUT), profiled over
batches of calls at leaf 0 (the concatenation goes out): the profiled ms per map of a launch, per batch.  One JSON line."""
import json
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "point-cloud-preprocessing-tools_amd"))
sys.path.insert(0, str(REPO / "tests"))


def main():
    import torch

    import bev_amd
    from bev_amd import synth

    p = bev_amd.params_for_sensor("HDL_64E")
    F, S, W, NM, BATCHES, CALLS = 48, p.slots, 3, 16, 5, 20
    dev = torch.device("cuda:0")
    with ThreadPoolExecutor(16) as ex:
        frames = list(ex.map(lambda i: synth.sweep(p, i, keep=0.98, n_dup=5000), range(F)))
    n_max = max(len(f) for f in frames)
    ctx = bev_amd.BevContext(p, device=0, max_batch=F, max_points=n_max)
    offs = np.zeros(F + 1, np.uint64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    d_in = torch.from_numpy(np.concatenate(frames).view(np.uint8).reshape(-1)).to(dev)
    d_ord = torch.empty(F * S * 32, dtype=torch.uint8, device=dev)
    d_multi = torch.empty(F * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    d_single = torch.empty(F * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.process_device(F, d_in.data_ptr(), offs, d_ord.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
    stride = bev_amd.regfront_max_out(S)
    d_pn = torch.empty(F * stride * 12, dtype=torch.float32, device=dev)
    d_cnt = torch.empty(F, dtype=torch.int32, device=dev)
    ctx.registration_front_device(F, d_ord.data_ptr(), None, d_pn.data_ptr(), stride, d_cnt.data_ptr())
    ctx.synchronize()
    rng = np.random.default_rng(7)
    map_offs = np.arange(NM + 1, dtype=np.uint64) * np.uint64(W)
    entry_frame = (np.arange(NM * W) % F).astype(np.int32)
    entry_pose = np.stack([bev_amd.yaw_translate_matrix(float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.3, 0.3)), 0.0,
                                                        float(rng.uniform(-1, 1))) for _ in range(NM * W)]).astype(np.float32)
    d_vout = torch.empty(NM * W * S * 16, dtype=torch.uint8, device=dev)
    d_pout = torch.empty(NM * W * stride * 12, dtype=torch.float32, device=dev)
    d_oc = torch.zeros(NM, dtype=torch.int32, device=dev)
    vox = lambda: ctx.submap_voxel_cloud_device(F, d_ord.data_ptr(), None, map_offs, entry_frame, entry_pose, 0.0, W * S,
                                                d_vout.data_ptr(), d_oc.data_ptr())
    pn = lambda: ctx.submap_pn_cloud_device(F, d_pn.data_ptr(), stride, d_cnt.data_ptr(), map_offs, entry_frame, entry_pose, 0.0,
                                            W * stride, d_pout.data_ptr(), d_oc.data_ptr())
    out = {}
    for name, call, kern in (("vox", vox, "k_submap_vox_out"), ("pn", pn, "k_submap_pn_out")):
        call()
        ctx.synchronize()
        rows = int(d_oc.cpu().numpy().astype(np.int64).sum())
        per = []
        for _ in range(BATCHES):
            ctx.profile_reset()
            ctx.profile_enable(True)
            for _ in range(CALLS):
                call()
            ctx.synchronize()
            st = [s for s in ctx.profile_get() if s["name"] == kern]
            ctx.profile_enable(False)
            per.append(st[0]["total_ms"] / st[0]["launches"] if st and st[0]["launches"] else None)
        out[name] = {"kernel": kern, "rows_copied_per_launch": rows, "ms_per_launch_by_batch": per}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
