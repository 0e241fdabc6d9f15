"""Coarse point-to-plane ICP (bev_coarse_registration_device_resident) on the registration front end's output of
device-resident HDL_64E frames.

    python scripts/bench_icp.py [--frames 1000] [--steps 10] [--warmup 2] [--out profiles/icp_bench.json]

The frames are benchlib's sweeps (no moved copies), run once through bev_process_device_resident and
bev_registration_front_device_resident; the context is created after the buffers.  The matches are the tool's match list
shape: frame i against (i + 1) mod N and against a seeded random partner, with seeded angle guesses (1000 matches for
1000 frames: every other frame gets one of each), each run from both guesses.  One JSON line: matches/s by benchlib.timed, the
per-kernel times of bev_profile_get over one more step, the mean iterations, the states, and the sequential C checker's
matches/s on one core (context only)."""
import argparse
import time

import numpy as np

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-matches", type=int, default=4, help="matches the C checker is timed on")
    bl.std_args(ap, frames=1000, sub_batch=500, steps=10, warmup=2, out="icp_bench.json")
    args = ap.parse_args()
    import torch

    import bev_amd
    import icp_lib as il

    il.build()
    p = bev_amd.params_for_sensor("HDL_64E")
    F, S = args.frames, p.slots
    dev = torch.device("cuda:0")
    frames = bl.sweeps(p, F)
    offs, d_in = bl.upload(frames, dev)
    n_max = max(len(f) for f in frames)
    del frames
    d_ord, d_multi, d_single = bl.bev_outputs(p, F, dev)
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

    step = lambda: ctx.coarse_registration_device(F, d_pn.data_ptr(), stride, d_cnt.data_ptr(), m, d_res.data_ptr(), d_best.data_ptr())
    fenced, unfenced = bl.timed(ctx, step, args.steps, args.warmup)
    kernels = bl.kernel_ms(ctx, step, "k_icp")
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
    bl.emit({
        "metric": "icp_matches_per_s", "sensor": "HDL_64E", "frames": F, "matches": n, "problems": 2 * n,
        "steps": args.steps, "warmup": args.warmup,
        "fenced_median_ms": fenced * 1e3, "fenced_matches_per_s": n / fenced,
        "unfenced_mean_ms": unfenced * 1e3, "unfenced_matches_per_s": n / unfenced,
        "records_per_frame_mean": float(cnt.mean()), "iterations_mean": float(res["iterations"].mean()),
        "states": np.bincount(res["state"].reshape(-1), minlength=6).tolist(),
        "kernels_ms_per_step": kernels,
        "checker_single_core_matches_per_s": 1.0 / cpu_s,
    }, args)


if __name__ == "__main__":
    main()
