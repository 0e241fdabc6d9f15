"""Batched projection of raw sweeps (bev_project_device_resident) on device-resident frames.

    python scripts/bench_project.py [--frames 1000] [--steps 20] [--warmup 5] [--copybw PATH]

One JSON line.  Per workload — MulRan sweeps of 65,536 returns, KITTI sweeps of about 120 k (projection_data.kitti_returns),
Oxford sweeps of about 35 k, and Oxford frames of 2 M returns — frames/s of one call over all frames by benchlib.timed, the
per-kernel times of bev_profile_get over one more step, and the algorithmic bytes per frame (16 n read + 32 n_out written)
over the kernel time.  --copybw: the built scripts/microbench/copybw.hip (benchlib.copy_rate): the yardstick of the two map
kernels.  Then MulRan end to end, three interleaved passes: project_device + process_device against process_device alone on
records projected beforehand."""
import argparse

import numpy as np

import benchlib as bl


def _tiled(torch, distinct, frames, dev):
    """`frames` frames on the device, the distinct host frames in turn; returns (tensor, offsets)"""
    sizes = [distinct[f % len(distinct)].size // 4 for f in range(frames)]
    offs = np.zeros(frames + 1, np.uint64)
    offs[1:] = np.cumsum(sizes)
    d = torch.empty(int(offs[-1]) * 4 + 4, dtype=torch.float32, device=dev)
    up = [torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(dev) for x in distinct]
    for f in range(frames):
        d[int(offs[f]) * 4:int(offs[f + 1]) * 4] = up[f % len(up)]
    return d, offs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big-frames", type=int, default=100, help="frames of the 2 M-return run")
    ap.add_argument("--copybw", default=None, help="the built scripts/microbench/copybw.hip")
    bl.std_args(ap, frames=1000, steps=20, warmup=5, sub_batch=500, out=None)
    args = ap.parse_args()
    import torch

    import bev_amd
    from projection_data import kitti_returns, raw_returns

    dev = torch.device("cuda:0")
    F = args.frames
    result = {"metric": "project_frames_per_s", "frames": F, "steps": args.steps, "warmup": args.warmup, "workloads": {}}

    copy_tbs = bl.copy_rate(args.copybw, result)
    pool = [raw_returns(70000, s, nonfinite=False) for s in range(8)]
    big = np.concatenate([np.roll(pool[i % 8], 11 * i, axis=0) for i in range(29)])[:2_000_000]
    workloads = [
        ("mulran_65536", 0, "OS1_64", [x[:65536] for x in pool], F),
        ("kitti_120k", 2, "HDL_64E", [kitti_returns(s, "sweep") for s in range(12)], F),
        ("oxford_35k", 1, "HDL_32E", [np.ascontiguousarray(x[:35000 - 300 * i].T) for i, x in enumerate(pool)], F),
        ("oxford_2M", 1, "HDL_32E", [np.ascontiguousarray(big.T), np.ascontiguousarray(big[::-1].T)], args.big_frames),
    ]
    for name, kind, sensor, distinct, nf in workloads:
        p = bev_amd.params_for_sensor(sensor)
        d_in, offs = _tiled(torch, distinct, nf, dev)
        n_out = bev_amd.project_batch_out_points(kind, nf, offs)
        d_out = torch.empty(n_out * 32, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx = bev_amd.BevContext(p, device=0, max_batch=8, max_points=max(p.slots, int(np.diff(offs).max())))
        step = lambda: ctx.project_device(kind, nf, d_in.data_ptr(), offs, d_out.data_ptr())
        fenced, unfenced = bl.timed(ctx, step, args.steps, args.warmup)
        kernels = bl.kernel_ms(ctx, step, ("k_project", "k_kitti"))
        ctx.close()
        bytes_frame = (16.0 * int(offs[-1]) + 32.0 * n_out) / nf
        kernel_ms = sum(kernels.values())
        w = {"kind": kind, "sensor": sensor, "frames": nf, "returns_per_frame_mean": float(offs[-1]) / nf,
             "fenced_median_ms": fenced * 1e3, "fenced_frames_per_s": nf / fenced,
             "unfenced_mean_ms": unfenced * 1e3, "unfenced_frames_per_s": nf / unfenced,
             "kernels_ms_per_step": kernels, "algorithmic_bytes_per_frame": bytes_frame,
             "achieved_GBps_over_kernel_time": bytes_frame * nf / (kernel_ms * 1e-3) / 1e9 if kernel_ms else None}
        if copy_tbs and kind != 2 and kernel_ms:
            w["fraction_of_copy_rate"] = w["achieved_GBps_over_kernel_time"] / (copy_tbs * 1e3)
        result["workloads"][name] = w
        del d_in, d_out
        torch.cuda.empty_cache()

    # MulRan end to end: raw returns -> records -> BEV, against the BEV path alone on records made beforehand
    p = bev_amd.params_for_sensor("OS1_64")
    d_in, offs = _tiled(torch, [x[:65536] for x in pool], F, dev)
    d_rec = torch.empty(int(offs[-1]) * 32, dtype=torch.uint8, device=dev)
    d_ord, d_multi, d_single = bl.bev_outputs(p, F, dev)
    torch.cuda.synchronize()
    ctx = bev_amd.BevContext(p, device=0, max_batch=args.sub_batch, max_points=65536)
    process = lambda: ctx.process_device(F, d_rec.data_ptr(), offs, d_ord.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())

    def both():
        ctx.project_device(0, F, d_in.data_ptr(), offs, d_rec.data_ptr())
        process()

    both()
    ctx.synchronize()
    passes = []
    for _ in range(3):
        a = bl.timed(ctx, both, args.steps, args.warmup)
        b = bl.timed(ctx, process, args.steps, args.warmup)
        passes.append({"project_and_process_unfenced_frames_per_s": F / a[1], "process_alone_unfenced_frames_per_s": F / b[1],
                       "project_and_process_fenced_frames_per_s": F / a[0], "process_alone_fenced_frames_per_s": F / b[0]})
    modes = sorted(set(int(m) for m in ctx.frame_info(0, min(8, F % args.sub_batch or args.sub_batch))[:, 1]))
    ctx.close()
    result["mulran_end_to_end"] = {"passes": passes, "frame_modes_of_the_last_sub_batch": modes}
    bl.emit(result, args)


if __name__ == "__main__":
    main()
