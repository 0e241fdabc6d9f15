"""Float max-height BEV of a batch (bev_float_bev_device_resident) on device-resident frames.

    python scripts/bench_manip.py [--frames 1000] [--steps 20] [--warmup 5] [--copybw PATH] [--per-cloud]

One JSON line.  The frames are marked HDL_64E sweeps (ordered and ground-marked by the oracle: what
bev_process_device_resident leaves in d_ordered), interval 1.0, label 0 skipped.  Per n_poses of 0, 1 and 8: frames/s of
one call over all frames as the median of fenced steps (call, bev_synchronize) and as the mean of unfenced steps (back to
back, one synchronisation at the end), k_float_bev_batch's time from bev_profile_get over one more step, and the algorithmic
bytes (32 n read + 4 M * M per grid zeroed and touched) over that time.  --copybw: the built scripts/microbench/copybw.hip,
run in the same process tree on the same box: its best plain-copy rate is the yardstick.  --per-cloud: the loop of
bev_float_bev over the same frames in host memory, for context.  BEV_AMD_LIB selects another build of the library."""
import argparse
import json
import os
import re
import socket
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "point-cloud-preprocessing-tools_amd"))
sys.path.insert(0, str(REPO / "tests"))


def _timed(ctx, step, steps, warmup):
    for _ in range(warmup):
        step()
    ctx.synchronize()
    fenced = []
    for _ in range(steps):
        t = time.perf_counter()
        step()
        ctx.synchronize()
        fenced.append(time.perf_counter() - t)
    t = time.perf_counter()
    for _ in range(steps):
        step()
    ctx.synchronize()
    return statistics.median(fenced), (time.perf_counter() - t) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=8, help="distinct sweeps the frames are tiled from")
    ap.add_argument("--copybw", default=None, help="the built scripts/microbench/copybw.hip")
    ap.add_argument("--per-cloud", action="store_true", help="also time the loop of bev_float_bev over the frames")
    args = ap.parse_args()
    import torch

    import bev_amd
    import oracle_lib as orc
    from bev_amd import synth

    dev = torch.device("cuda:0")
    F, interval = args.frames, 1.0
    p = bev_amd.params_for_sensor("HDL_64E")
    sp = orc.sensor_from_params(p)
    S = p.slots
    result = {"metric": "float_bev_frames_per_s", "frames": F, "steps": args.steps, "warmup": args.warmup,
              "records_per_frame": S, "interval": interval, "skip_label0": True,
              "library": os.environ.get("BEV_AMD_LIB", "csrc/libbev_mi355x.so"), "n_poses": {}}

    copy_tbs = None
    if args.copybw:
        out = subprocess.run([args.copybw], capture_output=True, text=True, timeout=600).stdout
        rates = [float(m.group(1)) for m in re.finditer(r"^copy .*? ([0-9.]+) TB/s$", out, flags=re.M)]
        copy_tbs = max(rates) if rates else None
        result["copy_rate_GBps"] = copy_tbs * 1e3 if copy_tbs else None
        result["copybw_lines"] = [l.strip() for l in out.splitlines() if l.startswith(("copy", "grid"))]

    distinct = [orc.mark_ground(sp, orc.order_cloud(sp, synth.sweep(p, s)))[0] for s in range(args.distinct)]
    up = [torch.from_numpy(c.view(np.uint8).reshape(-1).copy()).to(dev) for c in distinct]
    d_clouds = torch.empty(F * S * 32, dtype=torch.uint8, device=dev)
    for f in range(F):
        d_clouds[f * S * 32:(f + 1) * S * 32] = up[f % len(up)]
    offs = np.arange(F + 1, dtype=np.uint64) * np.uint64(S)
    ctx = bev_amd.BevContext(p, device=0, max_batch=8, max_points=S)
    M = int(ctx.lib.bev_float_bev_size(interval))
    rng = np.random.default_rng(1)
    for n_poses in (0, 1, 8):
        G = max(1, n_poses)
        poses = None
        if n_poses:
            poses = np.stack([np.stack([bev_amd.yaw_translate_matrix(rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-0.5, 0.5),
                                                                      rng.uniform(-180, 180)) for _ in range(n_poses)])
                              for _ in range(F)])
        d_out = torch.empty(F * G * M * M, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        step = lambda: ctx.float_bev_device(F, d_clouds.data_ptr(), offs, d_out.data_ptr(), interval, True, poses=poses)
        fenced, unfenced = _timed(ctx, step, args.steps, args.warmup)
        ctx.profile_reset()
        ctx.profile_enable(True)
        step()
        ctx.synchronize()
        kernel_ms = sum(k["total_ms"] for k in ctx.profile_get() if k["name"] == "k_float_bev_batch")
        ctx.profile_enable(False)
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
            t = time.perf_counter()
            for c in host:
                ctx.float_bev(c, interval, True)
            times.append(time.perf_counter() - t)
        result["per_cloud_bev_float_bev_loop"] = {"passes_ms": [x * 1e3 for x in times], "frames_per_s": F / min(times)}
    ctx.close()
    result["device"] = torch.cuda.get_device_name(0)
    result["host"] = socket.gethostname()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
