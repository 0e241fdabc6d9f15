"""Coarse point-to-plane ICP (bev_coarse_registration_device_resident) on the registration front end's output of
device-resident HDL_64E frames.

    python scripts/bench_icp.py [--frames 1000] [--steps 10] [--warmup 2] [--out profiles/icp_bench.json]

The frames are bench.py's default workload (synthetic HDL_64E sweeps, 98 % of the slots, 5,000 duplicates), run once
through bev_process_device_resident and bev_registration_front_device_resident.  The matches are the tool's match list
shape: frame i against (i + 1) mod N and against a seeded random partner, with seeded angle guesses (1000 matches for
1000 frames: every other frame gets one of each), each run from both guesses.  One JSON line (also written to --out):
matches/s as the median of fenced steps (launch, bev_synchronize) and as the mean of unfenced steps (back to back, one
synchronisation at the end), the per-kernel times of bev_profile_get over one more step, the mean iterations, the
states, and the sequential C checker's matches/s on one core (context only)."""
import argparse
import json
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-matches", type=int, default=4, help="matches the C checker is timed on")
    ap.add_argument("--out", default=str(REPO / "profiles" / "icp_bench.json"))
    args = ap.parse_args()
    import torch

    import bev_amd
    import icp_lib as il
    from bev_amd import synth

    il.build()
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
    d_pn = torch.empty(F * stride * 12, dtype=torch.float32, device=dev)
    d_cnt = torch.empty(F, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx = bev_amd.BevContext(p, device=0, max_batch=args.sub_batch, max_points=n_max)
    ctx.process_device(F, d_in.data_ptr(), offs, d_ord.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
    ctx.registration_front_device(F, d_ord.data_ptr(), None, d_pn.data_ptr(), stride, d_cnt.data_ptr())
    ctx.synchronize()

    rng = np.random.default_rng(2026)
    n = F
    m = np.zeros(n, bev_amd.MATCH_DTYPE)
    m["query_idx"] = np.arange(n) % F
    m["match_idx"] = np.where(np.arange(n) % 2 == 0, (np.arange(n) + 1) % F, rng.integers(0, F, n))
    m["angle_guess"] = rng.uniform(-180, 180, n).astype(np.float32)
    d_res = torch.zeros(n * 2 * bev_amd.ICP_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_best = torch.zeros(n, dtype=torch.int32, device=dev)

    def step():
        ctx.coarse_registration_device(F, d_pn.data_ptr(), stride, d_cnt.data_ptr(), m, d_res.data_ptr(),
                                       d_best.data_ptr())

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
    kernels = [k for k in ctx.profile_get() if k["name"].startswith("k_icp")]
    ctx.profile_enable(False)
    res = d_res.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE).reshape(n, 2)
    cnt = d_cnt.cpu().numpy()

    pn = d_pn.cpu().numpy().reshape(F, stride, 12)
    t = time.perf_counter()
    for k in range(args.cpu_matches):
        q, tg, a = m[k]
        for g in range(2):
            il.run(pn[q, : cnt[q]], pn[tg, : cnt[tg]], il.tool_guess(float(a), g))
    cpu_s = (time.perf_counter() - t) / args.cpu_matches
    ctx.close()
    line = json.dumps({
        "metric": "icp_matches_per_s", "sensor": "HDL_64E", "frames": F, "matches": n, "problems": 2 * n,
        "steps": args.steps, "warmup": args.warmup,
        "fenced_median_ms": statistics.median(fenced) * 1e3, "fenced_matches_per_s": n / statistics.median(fenced),
        "unfenced_mean_ms": unfenced * 1e3, "unfenced_matches_per_s": n / unfenced,
        "records_per_frame_mean": float(cnt.mean()), "iterations_mean": float(res["iterations"].mean()),
        "states": np.bincount(res["state"].reshape(-1), minlength=6).tolist(),
        "kernels_ms_per_step": {k["name"]: k["total_ms"] for k in kernels},
        "checker_single_core_matches_per_s": 1.0 / cpu_s,
        "device": torch.cuda.get_device_name(0), "host": socket.gethostname(),
    })
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
