"""The copy-out launch of the two scan-to-map cloud calls (K_SUBMAP_VOX_OUT, K_SUBMAP_PN_OUT), profiled over
batches of calls at leaf 0 (the concatenation goes out): the profiled ms per map of a launch, per batch.  One JSON line."""
import argparse

import numpy as np

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    bl.std_args(ap, out=None)
    args = ap.parse_args()
    import torch

    import bev_amd

    p = bev_amd.params_for_sensor("HDL_64E")
    F, S, W, NM, BATCHES, CALLS = 48, p.slots, 3, 16, 5, 20
    dev = torch.device("cuda:0")
    frames = bl.sweeps(p, F)
    ctx = bev_amd.BevContext(p, device=0, max_batch=F, max_points=max(len(f) for f in frames))
    offs, d_in = bl.upload(frames, dev)
    d_ord, d_multi, d_single = bl.bev_outputs(p, F, dev)
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
            st = bl.kernel_ms(ctx, lambda: [call() for _ in range(CALLS)], names=(kern,)).get(kern)
            per.append(st["ms_per_step"] / st["launches"] if st and st["launches"] else None)
        out[name] = {"kernel": kern, "rows_copied_per_launch": rows, "ms_per_launch_by_batch": per}
    ctx.close()
    bl.emit(out, args, machine=())


if __name__ == "__main__":
    main()
