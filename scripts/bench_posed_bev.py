"""The 24-layer and uint8 BEVs of a batch under per-frame poses (bev_posed_bev_device_resident) on device-resident frames.

    python scripts/bench_posed_bev.py [--frames 1000] [--steps 20] [--warmup 5] [--no-yardsticks] [--label TEXT]

One JSON line.  The frames are benchlib's marked sweeps, both outputs wanted.  Per n_poses of 0, 1 and 8: grids/s of one call
over all frames by benchlib.timed, and the times of k_posed_splat and k_posed_expand from bev_profile_get over one more step.
One frame's images are compared with the oracle in every configuration: the numbers are of code that computes the right thing.
Two yardsticks in the same call (skipped with --no-yardsticks):
  (a) the per-cloud route: bev_transform_cloud + bev_multi_bev + bev_single_bev per frame over the same frames in host
      memory, one pose per frame;
  (b) bev_float_bev_device_resident at the same pose counts (one atomic per point where this has two, and no expand pass)."""
import argparse
import os
import sys
import time

import numpy as np

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-yardsticks", action="store_true", help="only the batch call (the A/B of two builds)")
    bl.std_args(ap, frames=1000, steps=20, warmup=5, distinct=8, out=None)
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
    result = {"metric": "posed_bev_grids_per_s", "frames": F, "steps": args.steps, "warmup": args.warmup,
              "records_per_frame": S, "mat_size": M, "layers": L, "outputs": "multi and single",
              "posed_group_env": os.environ.get("BEV_POSED_GROUP"), "n_poses": {}}

    t = bl.tiled_marked_frames(p, args.distinct, F, dev)
    distinct, d_clouds, offs = t.clouds, t.d_clouds, t.offs
    ctx = bev_amd.BevContext(p, device=0, max_batch=8, max_points=S)
    Mf = int(ctx.lib.bev_float_bev_size(1.0))
    rng = np.random.default_rng(1)
    for n_poses in (0, 1, 8):
        G = max(1, n_poses)
        poses = bl.frame_poses(rng, F, n_poses)
        d_multi = torch.empty(F * G * L * M * M, dtype=torch.uint8, device=dev)
        d_single = torch.empty(F * G * M * M, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        step = lambda: ctx.posed_bev_device(F, d_clouds.data_ptr(), offs, d_multi.data_ptr(), d_single.data_ptr(), poses=poses)
        fenced, unfenced = bl.timed(ctx, step, args.steps, args.warmup)
        kernels = bl.kernel_ms(ctx, step, names=("k_posed_splat", "k_posed_expand"))
        got_m = d_multi[(F - 1) * G * L * M * M:].cpu().numpy().reshape(G, L, M, M)
        got_s = d_single[(F - 1) * G * M * M:].cpu().numpy().reshape(G, M, M)
        cloud = distinct[(F - 1) % len(distinct)]
        for k in range(G):
            moved = orc.transform_cloud(cloud, poses[F - 1, k]) if n_poses else cloud
            assert got_m[k].tobytes() == orc.multi_bev(sp, moved, 1.0).tobytes(), (n_poses, k)
            assert got_s[k].tobytes() == orc.single_bev(moved, 1.0).tobytes(), (n_poses, k)
        grids = F * G
        w = {"grids": grids, "fenced_median_ms": fenced * 1e3, "fenced_grids_per_s": grids / fenced,
             "unfenced_mean_ms": unfenced * 1e3, "unfenced_grids_per_s": grids / unfenced, "kernels": kernels,
             # what the algorithm has to move per grid: the frame's records once per frame, the planes zeroed, read and the
             # images written (atomics not counted: two words per point that is on the grid)
             "algorithmic_bytes_per_grid": 32.0 * S / G + 2 * 8.0 * M * M + (L + 1.0) * M * M}
        if "k_posed_splat" in kernels:
            w["splat_us_per_grid"] = kernels["k_posed_splat"]["ms_per_step"] * 1e3 / grids
        if "k_posed_expand" in kernels:
            w["expand_us_per_grid"] = kernels["k_posed_expand"]["ms_per_step"] * 1e3 / grids
            w["expand_written_GBps"] = (L + 1.0) * M * M * grids / (kernels["k_posed_expand"]["ms_per_step"] * 1e-3) / 1e9
        del d_multi, d_single
        torch.cuda.empty_cache()

        if not args.no_yardsticks:   # (b) the float grid of the same frames and poses
            d_out = torch.empty(F * G * Mf * Mf, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            fstep = lambda: ctx.float_bev_device(F, d_clouds.data_ptr(), offs, d_out.data_ptr(), 1.0, True, poses=poses)
            ff, fu = bl.timed(ctx, fstep, args.steps, args.warmup)
            fk = bl.kernel_ms(ctx, fstep, names=("k_float_bev_batch",))
            w["float_bev_yardstick"] = {"fenced_median_ms": ff * 1e3, "fenced_grids_per_s": grids / ff, "unfenced_mean_ms": fu * 1e3,
                                        "unfenced_grids_per_s": grids / fu, "kernels": fk}
            if "k_float_bev_batch" in fk and "k_posed_splat" in kernels:
                w["float_bev_yardstick"]["kernel_us_per_grid"] = fk["k_float_bev_batch"]["ms_per_step"] * 1e3 / grids
                w["splat_over_float_kernel"] = kernels["k_posed_splat"]["ms_per_step"] / fk["k_float_bev_batch"]["ms_per_step"]
            w["posed_over_float_unfenced_time"] = unfenced / fu
            del d_out
            torch.cuda.empty_cache()
        result["n_poses"][str(n_poses)] = w

    if not args.no_yardsticks:   # (a) the per-cloud route, one pose per frame, host memory
        host = [distinct[f % len(distinct)] for f in range(F)]
        pose1 = [bev_amd.yaw_translate_matrix(rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-0.5, 0.5), rng.uniform(-180, 180))
                 for _ in range(F)]
        ctx.single_bev(ctx.transform_cloud(host[0], pose1[0]))
        ctx.multi_bev(host[0])
        times = []
        for _ in range(2):
            t0 = time.perf_counter()
            for c, m in zip(host, pose1):
                moved = ctx.transform_cloud(c, m)
                ctx.multi_bev(moved)
                ctx.single_bev(moved)
            times.append(time.perf_counter() - t0)
        per_cloud = F / min(times)
        one = result["n_poses"]["1"]
        result["per_cloud_transform_multi_single_loop"] = {"passes_ms": [x * 1e3 for x in times], "grids_per_s": per_cloud}
        result["batch_over_per_cloud_at_1_pose"] = one["unfenced_grids_per_s"] / per_cloud
        result["batch_over_per_cloud_at_8_poses"] = result["n_poses"]["8"]["unfenced_grids_per_s"] / per_cloud
        assert one["unfenced_grids_per_s"] > per_cloud, "the batch call is not faster than the per-cloud route"
    ctx.close()
    bl.emit(result, args)


if __name__ == "__main__":
    main()
