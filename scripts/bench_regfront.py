"""Registration front end (top-part flatten -> voxel grid -> 2-D normals) on device-resident HDL_64E frames.

    python scripts/bench_regfront.py [--frames 1000] [--steps 20] [--warmup 5]

The frames are benchlib's sweeps (no moved copies), run once through bev_process_device_resident; the chain then reads that
d_ordered output.  The context is created after the buffers.  One JSON line: frames/s of the chain by benchlib.timed, the
per-kernel times of bev_profile_get over one more step, and the sequential C checker's frames/s on one core (context only)."""
import argparse
import time

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-frames", type=int, default=5, help="frames the C checker is timed on")
    bl.std_args(ap, frames=1000, sub_batch=500, steps=20, warmup=5, out=None)
    args = ap.parse_args()
    import torch

    import bev_amd
    import regfront_lib as rl

    rl.build()
    p = bev_amd.params_for_sensor("HDL_64E")
    F, S = args.frames, p.slots
    dev = torch.device("cuda:0")
    frames = bl.sweeps(p, F)
    offs, d_in = bl.upload(frames, dev)
    n_max = max(len(f) for f in frames)
    del frames
    d_ord, d_multi, d_single = bl.bev_outputs(p, F, dev)
    stride = bev_amd.regfront_max_out(S)
    d_out = torch.empty(F * stride * 12, dtype=torch.float32, device=dev)
    d_cnt = torch.empty(F, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx = bev_amd.BevContext(p, device=0, max_batch=args.sub_batch, max_points=n_max)
    ctx.process_device(F, d_in.data_ptr(), offs, d_ord.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
    ctx.synchronize()

    step = lambda: ctx.registration_front_device(F, d_ord.data_ptr(), None, d_out.data_ptr(), stride, d_cnt.data_ptr())
    fenced, unfenced = bl.timed(ctx, step, args.steps, args.warmup)
    kernels = bl.kernel_ms(ctx, step, "k_rf_")
    cnt = d_cnt.cpu().numpy()

    ordered = d_ord[: args.cpu_frames * S * 32].cpu().numpy().view(bev_amd.POINT_DTYPE).reshape(args.cpu_frames, S)
    t = time.perf_counter()
    for i in range(args.cpu_frames):
        rl.chain(ordered[i])
    cpu_s = (time.perf_counter() - t) / args.cpu_frames
    ctx.close()
    bl.emit({
        "metric": "regfront_frames_per_s", "sensor": "HDL_64E", "frames": F, "sub_batch": args.sub_batch,
        "steps": args.steps, "warmup": args.warmup,
        "fenced_median_ms": fenced * 1e3, "fenced_frames_per_s": F / fenced,
        "unfenced_mean_ms": unfenced * 1e3, "unfenced_frames_per_s": F / unfenced,
        "records_per_frame_mean": float(cnt.mean()), "records_per_frame_max": int(cnt.max()),
        "kernels_ms_per_step": kernels,
        "checker_single_core_frames_per_s": 1.0 / cpu_s,
    }, args)


if __name__ == "__main__":
    main()
