"""Float max-height BEV of a batch (bev_float_bev_device_resident) on device-resident frames.

    python scripts/bench_manip.py [--frames 1000] [--steps 20] [--warmup 5] [--copybw PATH] [--per-cloud]

One JSON line.  The frames are benchlib's marked sweeps, interval 1.0, label 0 skipped.  Per n_poses of 0, 1 and 8: frames/s of
one call over all frames by benchlib.timed, k_float_bev_batch's time from bev_profile_get over one more step, and the
algorithmic bytes (32 n read + 4 M * M per grid zeroed and touched) over that time.  --copybw: the built
scripts/microbench/copybw.hip (benchlib.copy_rate).  --per-cloud: the loop of bev_float_bev over the same frames in host
memory, for context."""
import argparse
import time

import numpy as np

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copybw", default=None, help="the built scripts/microbench/copybw.hip")
    ap.add_argument("--per-cloud", action="store_true", help="also time the loop of bev_float_bev over the frames")
    bl.std_args(ap, frames=1000, steps=20, warmup=5, distinct=8, out=None)
    args = ap.parse_args()
    import torch

    import bev_amd
    import oracle_lib as orc

    dev = torch.device("cuda:0")
    F, interval = args.frames, 1.0
    p = bev_amd.params_for_sensor("HDL_64E")
    S = p.slots
    result = {"metric": "float_bev_frames_per_s", "frames": F, "steps": args.steps, "warmup": args.warmup,
              "records_per_frame": S, "interval": interval, "skip_label0": True, "n_poses": {}}
    copy_tbs = bl.copy_rate(args.copybw, result)

    t = bl.tiled_marked_frames(p, args.distinct, F, dev)
    distinct, d_clouds, offs = t.clouds, t.d_clouds, t.offs
    ctx = bev_amd.BevContext(p, device=0, max_batch=8, max_points=S)
    M = int(ctx.lib.bev_float_bev_size(interval))
    rng = np.random.default_rng(1)
    for n_poses in (0, 1, 8):
        G = max(1, n_poses)
        poses = bl.frame_poses(rng, F, n_poses)
        d_out = torch.empty(F * G * M * M, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        step = lambda: ctx.float_bev_device(F, d_clouds.data_ptr(), offs, d_out.data_ptr(), interval, True, poses=poses)
        fenced, unfenced = bl.timed(ctx, step, args.steps, args.warmup)
        kernel_ms = sum(k["ms_per_step"] for k in bl.kernel_ms(ctx, step, names=("k_float_bev_batch",)).values())
        # one frame's grids against the oracle: the numbers are of a kernel that computes the right thing
        got = d_out[(F - 1) * G * M * M:].cpu().numpy().reshape(G, M, M)
        cloud = distinct[(F - 1) % len(distinct)]
        for k in range(G):
            want = orc.float_bev(orc.transform_cloud(cloud, poses[F - 1, k]) if n_poses else cloud, interval, True)
            assert got[k].tobytes() == want.tobytes(), (n_poses, k)
        bytes_frame = 32.0 * S + 4.0 * M * M * G
        w = {"fenced_median_ms": fenced * 1e3, "fenced_frames_per_s": F / fenced,
             "unfenced_mean_ms": unfenced * 1e3, "unfenced_frames_per_s": F / unfenced,
             "kernel_ms_per_step": kernel_ms, "algorithmic_bytes_per_frame": bytes_frame,
             "achieved_GBps_over_kernel_time": bytes_frame * F / (kernel_ms * 1e-3) / 1e9 if kernel_ms else None}
        if copy_tbs and kernel_ms:
            w["fraction_of_copy_rate"] = w["achieved_GBps_over_kernel_time"] / (copy_tbs * 1e3)
        result["n_poses"][str(n_poses)] = w
        del d_out
        torch.cuda.empty_cache()

    if args.per_cloud:
        host = [distinct[f % len(distinct)] for f in range(F)]
        ctx.float_bev(host[0], interval, True)
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            for c in host:
                ctx.float_bev(c, interval, True)
            times.append(time.perf_counter() - t0)
        result["per_cloud_bev_float_bev_loop"] = {"passes_ms": [x * 1e3 for x in times], "frames_per_s": F / min(times)}
    ctx.close()
    bl.emit(result, args)


if __name__ == "__main__":
    main()
