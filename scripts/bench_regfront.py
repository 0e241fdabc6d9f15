"""Registration front end (top-part flatten -> voxel grid -> 2-D normals) on device-resident HDL_64E frames.

    python scripts/bench_regfront.py [--frames 1000] [--steps 20] [--warmup 5]

The frames are bench.py's default workload (synthetic HDL_64E sweeps, 98 % of the slots, 5,000 duplicates), run once
through bev_process_device_resident; the chain then reads that d_ordered output.  One JSON line: frames/s of the chain
as the median of fenced steps (launch, bev_synchronize) and as the mean of unfenced steps (back to back, one
synchronisation at the end), the per-kernel times of bev_profile_get over one more step, and the sequential C checker's
frames/s on one core (context only)."""
import argparse
import json
import os
import socket
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "point-cloud-preprocessing-tools_amd"))
sys.path.insert(0, str(REPO / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--sub-batch", type=int, default=500)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-frames", type=int, default=5, help="frames the C checker is timed on")
    args = ap.parse_args()
    import torch

    import bev_amd
    import regfront_lib as rl
    from bev_amd import synth

    rl.build()
    p = bev_amd.params_for_sensor("HDL_64E")
    F, S = args.frames, p.slots
    dev = torch.device("cuda:0")
    with ThreadPoolExecutor(16) as ex:
        frames = list(ex.map(lambda i: synth.sweep(p, i, keep=0.98, n_dup=5000), range(F)))
    offs = np.zeros(F + 1, np.uint64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    d_in = torch.from_numpy(np.concatenate(frames).view(np.uint8).reshape(-1)).to(dev)
    n_max = max(len(f) for f in frames)
    del frames
    d_ord = torch.empty(F * S * 32, dtype=torch.uint8, device=dev)
    d_multi = torch.empty(F * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    d_single = torch.empty(F * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    stride = bev_amd.regfront_max_out(S)
    d_out = torch.empty(F * stride * 12, dtype=torch.float32, device=dev)
    d_cnt = torch.empty(F, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx = bev_amd.BevContext(p, device=0, max_batch=args.sub_batch, max_points=n_max)
    ctx.process_device(F, d_in.data_ptr(), offs, d_ord.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
    ctx.synchronize()

    def step():
        ctx.registration_front_device(F, d_ord.data_ptr(), None, d_out.data_ptr(), stride, d_cnt.data_ptr())

    for _ in range(args.warmup):
        step()
    ctx.synchronize()
    fenced = []
    for _ in range(args.steps):
        t = time.perf_counter()
        step()
        ctx.synchronize()
        fenced.append(time.perf_counter() - t)
    t = time.perf_counter()
    for _ in range(args.steps):
        step()
    ctx.synchronize()
    unfenced = (time.perf_counter() - t) / args.steps
    ctx.profile_reset()
    ctx.profile_enable(True)
    step()
    ctx.synchronize()
    kernels = [k for k in ctx.profile_get() if k["name"].startswith("k_rf_")]
    ctx.profile_enable(False)
    cnt = d_cnt.cpu().numpy()

    ordered = d_ord[: args.cpu_frames * S * 32].cpu().numpy().view(bev_amd.POINT_DTYPE).reshape(args.cpu_frames, S)
    t = time.perf_counter()
    for i in range(args.cpu_frames):
        rl.chain(ordered[i])
    cpu_s = (time.perf_counter() - t) / args.cpu_frames
    ctx.close()
    print(json.dumps({
        "metric": "regfront_frames_per_s", "sensor": "HDL_64E", "frames": F, "sub_batch": args.sub_batch,
        "steps": args.steps, "warmup": args.warmup,
        "fenced_median_ms": statistics.median(fenced) * 1e3, "fenced_frames_per_s": F / statistics.median(fenced),
        "unfenced_mean_ms": unfenced * 1e3, "unfenced_frames_per_s": F / unfenced,
        "records_per_frame_mean": float(cnt.mean()), "records_per_frame_max": int(cnt.max()),
        "kernels_ms_per_step": {k["name"]: k["total_ms"] for k in kernels},
        "checker_single_core_frames_per_s": 1.0 / cpu_s,
        "device": torch.cuda.get_device_name(0), "host": socket.gethostname(),
    }))


if __name__ == "__main__":
    main()
