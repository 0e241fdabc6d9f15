"""The float max-height BEV of submaps (bev_submap_float_bev_device_resident) on device-resident frames, against the float call.

    python scripts/bench_submap_float_bev.py [--frames 1000] [--steps 20] [--warmup 5] [--windows 1,5,21] [--out FILE] [--label TEXT]

One JSON line, also written to --out (default profiles/submap_float_bev_bench.json).  The frames are benchlib's marked sweeps,
the workload its sliding windows, interval 1.0, label-0 points skipped, all in one call.
Yardstick: bev_float_bev_device_resident with the same W poses for every frame (W at most 64) in the same process: it does as
many point-poses (a few more: its windows are not clipped at the ends) and zeroes and fills W times as many grids.  The two
calls are timed alternately, run by run (A, B, A, B), each run by benchlib.timed.  The kernels' times come from
bev_profile_get over five more steps of each call, alternated; the median step is reported, all five times beside it.  Beside
them, profiled only: the yardstick's own work through the new call (F * W maps of one entry each), which separates what
sharing grids between frames costs from what the kernel and the plan cost.
One full-window map's grid is compared with the oracle in every configuration: the numbers are of code that computes the
right thing."""
import argparse
import sys

import numpy as np

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="1,5,21")
    bl.std_args(ap, frames=1000, steps=20, warmup=5, distinct=8, out="submap_float_bev_bench.json")
    args = ap.parse_args()
    import torch

    import bev_amd
    import oracle_lib as orc

    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured (there is no CPU path)")
    dev = torch.device("cuda:0")
    F = args.frames
    p = bev_amd.params_for_sensor("HDL_64E")
    S, M = p.slots, 201
    A, B = "k_submap_float_splat", "k_float_bev_batch"
    result = {"metric": "submap_float_bev_maps_per_s", "frames": F, "steps": args.steps, "warmup": args.warmup, "runs": "A, B, A, B",
              "records_per_frame": S, "interval": 1.0, "skip_label0": 1, "mat_size": M, "windows": {}}

    t = bl.tiled_marked_frames(p, args.distinct, F, dev)
    distinct, d_clouds, offs = t.clouds, t.d_clouds, t.offs
    ctx = bev_amd.BevContext(p, device=0, max_batch=8, max_points=S)
    assert int(ctx.lib.bev_float_bev_size(1.0)) == M
    for W in [int(w) for w in args.windows.split(",")]:
        h = W // 2
        rel = bl.relative_poses(W)
        windows, map_offs, entry_frame, entry_pose = bl.sliding_windows(F, W, rel)
        poses = np.ascontiguousarray(np.broadcast_to(np.stack([rel[d] for d in range(-h, h + 1)]), (F, W, 12)))
        d_out = torch.empty(F * M * M, dtype=torch.float32, device=dev)
        y_out = torch.empty(F * W * M * M, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        a_step = lambda: ctx.submap_float_bev_device(F, d_clouds.data_ptr(), offs, map_offs, entry_frame, entry_pose, d_out.data_ptr(),
                                                     1.0, True)
        b_step = lambda: ctx.float_bev_device(F, d_clouds.data_ptr(), offs, y_out.data_ptr(), 1.0, True, poses=poses)
        runs = {"submap": [], "float": []}
        for _ in range(2):
            for name, step in (("submap", a_step), ("float", b_step)):
                fenced, unfenced = bl.timed(ctx, step, args.steps, args.warmup)
                runs[name].append({"fenced_median_ms": fenced * 1e3, "unfenced_mean_ms": unfenced * 1e3})
        # the kernels' times: five profiled steps of each call, alternated; the median step's figures are reported
        # (C: the yardstick's work through the new call — F * W maps of one entry, map f * W + k = frame f under pose k, into
        # the yardstick's buffer: the same grids as B, no grid shared between frames; what separates A from C is the sharing)
        c_offs = np.arange(F * W + 1, dtype=np.uint64)
        c_frame = np.repeat(np.arange(F, dtype=np.int32), W)
        c_pose = poses.reshape(F * W, 12)
        c_step = lambda: ctx.submap_float_bev_device(F, d_clouds.data_ptr(), offs, c_offs, c_frame, c_pose, y_out.data_ptr(), 1.0, True)
        pa, pb, pc = [], [], []
        for _ in range(5):
            pa.append(bl.kernel_ms(ctx, a_step, names=(A,)))
            pb.append(bl.kernel_ms(ctx, b_step, names=(B,)))
            pc.append(bl.kernel_ms(ctx, c_step, names=(A,)))
        ka = sorted(pa, key=lambda k: k[A]["ms_per_step"])[2]
        kb = sorted(pb, key=lambda k: k[B]["ms_per_step"])[2]
        ka[A]["ms_of_5_steps"] = [k[A]["ms_per_step"] for k in pa]
        kb[B]["ms_of_5_steps"] = [k[B]["ms_per_step"] for k in pb]

        # one map with a full window against the oracle, and the yardstick's grid of the same key frame under the identity
        a_step()
        b_step()
        ctx.synchronize()
        i = F // 2
        moved = np.concatenate([orc.transform_cloud(distinct[j % len(distinct)], rel[j - i]) for j in windows[i]])
        assert d_out[i * M * M:(i + 1) * M * M].cpu().numpy().tobytes() == orc.float_bev(moved, 1.0, True).tobytes(), W
        own = orc.transform_cloud(distinct[i % len(distinct)], rel[0])
        g = i * W + h
        assert y_out[g * M * M:(g + 1) * M * M].cpu().numpy().tobytes() == orc.float_bev(own, 1.0, True).tobytes(), W

        entries, y_entries = int(map_offs[-1]), F * W
        best = {n: min(r["unfenced_mean_ms"] for r in runs[n]) for n in runs}
        w = {"half_window": h, "maps": F, "entries": entries, "point_poses": entries * S, "runs": runs,
             "maps_per_s": F / (best["submap"] * 1e-3), "point_poses_per_s": entries * S / (best["submap"] * 1e-3),
             "kernels": ka, "oracle_checked_map": i,
             "float_yardstick": {"grids": y_entries, "point_poses": y_entries * S, "kernels": kb,
                                 "frames_per_s": F / (best["float"] * 1e-3),
                                 "point_poses_per_s": y_entries * S / (best["float"] * 1e-3)},
             "one_entry_per_map": {"maps": F * W, "k_submap_float_splat_ms_of_5_steps": [k[A]["ms_per_step"] for k in pc]},
             "submap_over_float_unfenced_time": [a["unfenced_mean_ms"] / b["unfenced_mean_ms"] for a, b in zip(runs["submap"], runs["float"])],
             "submap_over_float_fenced_time": [a["fenced_median_ms"] / b["fenced_median_ms"] for a, b in zip(runs["submap"], runs["float"])]}
        w["splat_ns_per_kilo_point_pose"] = ka[A]["ms_per_step"] * 1e6 / (entries * S / 1e3)
        w["float_yardstick"]["splat_ns_per_kilo_point_pose"] = kb[B]["ms_per_step"] * 1e6 / (y_entries * S / 1e3)
        w["one_entry_per_map"]["splat_ns_per_kilo_point_pose"] = sorted(k[A]["ms_per_step"] for k in pc)[2] * 1e6 / (y_entries * S / 1e3)
        w["submap_over_float_splat_per_point_pose"] = w["splat_ns_per_kilo_point_pose"] / w["float_yardstick"]["splat_ns_per_kilo_point_pose"]
        result["windows"][str(W)] = w
        del d_out, y_out
        torch.cuda.empty_cache()
    ctx.close()
    bl.emit(result, args, machine=("device",))


if __name__ == "__main__":
    main()
