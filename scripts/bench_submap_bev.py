"""The 24-layer and uint8 BEVs of submaps (bev_submap_bev_device_resident) on device-resident frames, against the posed call.

    python scripts/bench_submap_bev.py [--frames 1000] [--steps 20] [--warmup 5] [--windows 1,5,21] [--out FILE] [--label TEXT]

One JSON line, also written to --out (default profiles/submap_bev_bench.json).  The frames are benchlib's marked sweeps, the
workload its sliding windows, both outputs wanted, all in one call.
Yardstick: bev_posed_bev_device_resident with the same W poses for every frame (W at most 64) in the same process: it does as
many splats (a few more: its windows are not clipped at the ends) and expands W times as many images.  The two calls are timed
alternately, run by run (A, B, A, B), each run by benchlib.timed.  The kernels' times come from bev_profile_get over five more
steps of each call, alternated; the median step is reported, all five splat times beside it.
Beside them, profiled only: the yardstick's own work through the new call (F * W maps of one entry each), which separates
what sharing grids between frames costs from what the kernel and the plan cost.
One full-window map's images are compared with the oracle in every configuration: the numbers are of code that computes the
right thing."""
import argparse
import os
import sys

import numpy as np

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="1,5,21")
    bl.std_args(ap, frames=1000, steps=20, warmup=5, distinct=8, out="submap_bev_bench.json")
    args = ap.parse_args()
    import torch

    import bev_amd
    import oracle_lib as orc

    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured (there is no CPU path)")
    dev = torch.device("cuda:0")
    F = args.frames
    p = bev_amd.params_for_sensor("HDL_64E")
    sp = orc.sensor_from_params(p)
    S, M, L = p.slots, p.mat_size, p.n_layers
    result = {"metric": "submap_bev_maps_per_s", "frames": F, "steps": args.steps, "warmup": args.warmup, "runs": "A, B, A, B",
              "records_per_frame": S, "mat_size": M, "layers": L, "outputs": "multi and single",
              "posed_group_env": os.environ.get("BEV_POSED_GROUP"), "windows": {}}

    t = bl.tiled_marked_frames(p, args.distinct, F, dev)
    distinct, d_clouds, offs = t.clouds, t.d_clouds, t.offs
    ctx = bev_amd.BevContext(p, device=0, max_batch=8, max_points=S)
    for W in [int(w) for w in args.windows.split(",")]:
        h = W // 2
        rel = bl.relative_poses(W)
        windows, map_offs, entry_frame, entry_pose = bl.sliding_windows(F, W, rel)
        poses = np.ascontiguousarray(np.broadcast_to(np.stack([rel[d] for d in range(-h, h + 1)]), (F, W, 12)))
        d_multi = torch.empty(F * L * M * M, dtype=torch.uint8, device=dev)
        d_single = torch.empty(F * M * M, dtype=torch.uint8, device=dev)
        y_multi = torch.empty(F * W * L * M * M, dtype=torch.uint8, device=dev)
        y_single = torch.empty(F * W * M * M, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        a_step = lambda: ctx.submap_bev_device(F, d_clouds.data_ptr(), offs, map_offs, entry_frame, entry_pose, d_multi.data_ptr(),
                                               d_single.data_ptr())
        b_step = lambda: ctx.posed_bev_device(F, d_clouds.data_ptr(), offs, y_multi.data_ptr(), y_single.data_ptr(), poses=poses)
        runs = {"submap": [], "posed": []}
        for _ in range(2):
            for name, step in (("submap", a_step), ("posed", b_step)):
                fenced, unfenced = bl.timed(ctx, step, args.steps, args.warmup)
                runs[name].append({"fenced_median_ms": fenced * 1e3, "unfenced_mean_ms": unfenced * 1e3})
        # the kernels' times: five profiled steps of each call, alternated; the median step's figures are reported
        # (C: the yardstick's work through the new call — F * W maps of one entry, map f * W + k = frame f under pose k, into
        # the yardstick's buffers: the same grids as B, no grid shared between frames; what separates A from C is the sharing)
        c_offs = np.arange(F * W + 1, dtype=np.uint64)
        c_frame = np.repeat(np.arange(F, dtype=np.int32), W)
        c_pose = poses.reshape(F * W, 12)
        c_step = lambda: ctx.submap_bev_device(F, d_clouds.data_ptr(), offs, c_offs, c_frame, c_pose, y_multi.data_ptr(), y_single.data_ptr())
        pa, pb, pc = [], [], []
        for _ in range(5):
            pa.append(bl.kernel_ms(ctx, a_step, names=("k_submap_splat", "k_posed_expand")))
            pb.append(bl.kernel_ms(ctx, b_step, names=("k_posed_splat", "k_posed_expand")))
            pc.append(bl.kernel_ms(ctx, c_step, names=("k_submap_splat", "k_posed_expand")))
        ka = sorted(pa, key=lambda k: k["k_submap_splat"]["ms_per_step"])[2]
        kb = sorted(pb, key=lambda k: k["k_posed_splat"]["ms_per_step"])[2]
        ka["k_submap_splat"]["ms_of_5_steps"] = [k["k_submap_splat"]["ms_per_step"] for k in pa]
        kb["k_posed_splat"]["ms_of_5_steps"] = [k["k_posed_splat"]["ms_per_step"] for k in pb]

        # one map with a full window against the oracle, and the yardstick's image of the same key frame under the identity
        i = F // 2
        moved = np.concatenate([orc.transform_cloud(distinct[j % len(distinct)], rel[j - i]) for j in windows[i]])
        got_m = d_multi[i * L * M * M:(i + 1) * L * M * M].cpu().numpy()
        got_s = d_single[i * M * M:(i + 1) * M * M].cpu().numpy()
        assert got_m.tobytes() == orc.multi_bev(sp, moved, 1.0).tobytes(), W
        assert got_s.tobytes() == orc.single_bev(moved, 1.0).tobytes(), W
        own = orc.transform_cloud(distinct[i % len(distinct)], rel[0])
        g = i * W + h
        assert y_single[g * M * M:(g + 1) * M * M].cpu().numpy().tobytes() == orc.single_bev(own, 1.0).tobytes(), W

        entries, y_entries = int(map_offs[-1]), F * W
        best = {n: min(r["unfenced_mean_ms"] for r in runs[n]) for n in runs}
        w = {"half_window": h, "maps": F, "entries": entries, "point_poses": entries * S, "runs": runs,
             "launch_groups": ka.get("k_posed_expand", {}).get("launches"),
             "maps_per_s": F / (best["submap"] * 1e-3), "point_poses_per_s": entries * S / (best["submap"] * 1e-3),
             "kernels": ka,
             "posed_yardstick": {"grids": y_entries, "point_poses": y_entries * S, "kernels": kb,
                                 "launch_groups": kb.get("k_posed_expand", {}).get("launches"),
                                 "point_poses_per_s": y_entries * S / (best["posed"] * 1e-3)},
             "one_entry_per_map": {"maps": F * W, "k_submap_splat_ms_of_5_steps": [k["k_submap_splat"]["ms_per_step"] for k in pc],
                                   "launch_groups": pc[0]["k_posed_expand"]["launches"]},
             "submap_over_posed_unfenced_time": [a["unfenced_mean_ms"] / b["unfenced_mean_ms"] for a, b in zip(runs["submap"], runs["posed"])],
             "submap_over_posed_fenced_time": [a["fenced_median_ms"] / b["fenced_median_ms"] for a, b in zip(runs["submap"], runs["posed"])]}
        if "k_submap_splat" in ka and "k_posed_splat" in kb:
            w["splat_ns_per_kilo_point_pose"] = ka["k_submap_splat"]["ms_per_step"] * 1e6 / (entries * S / 1e3)
            w["posed_yardstick"]["splat_ns_per_kilo_point_pose"] = kb["k_posed_splat"]["ms_per_step"] * 1e6 / (y_entries * S / 1e3)
            w["submap_over_posed_splat_per_point_pose"] = w["splat_ns_per_kilo_point_pose"] / w["posed_yardstick"]["splat_ns_per_kilo_point_pose"]
        result["windows"][str(W)] = w
        del d_multi, d_single, y_multi, y_single
        torch.cuda.empty_cache()
    ctx.close()
    bl.emit(result, args)


if __name__ == "__main__":
    main()
