"""Fine ICP (bev_fine_registration_device_resident) behind the whole device-resident chain of HDL_64E frames.

    python scripts/bench_fine_icp.py [--frames 1000] [--moved 500] [--steps 3] [--warmup 1] [--out profiles/fine_icp_bench.json]

The frames are benchlib's sweeps and moved copies, run once through bev_process_device_resident, the registration front end
and the coarse entry (the front end's buffers are allocated before the BEV path runs, and nothing is released).  Two match
lists: bench_icp.py's (frame i against (i + 1) mod N or a seeded random partner, seeded angle guesses) and benchlib's
moved-copy pairs.  For each list and tool setting (top-part: guesses from the coarse device output; whole: the yaw guess):
matches/s by benchlib.timed, the per-kernel times of bev_profile_get over one more step, the iterations and states, the voxels
per full cloud; and the sequential C checker's matches/s on one core (context only).  One JSON line."""
import argparse
import time
from types import SimpleNamespace

import numpy as np

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-matches", type=int, default=2, help="matches the C checker is timed on")
    bl.std_args(ap, frames=1000, moved=500, sub_batch=500, steps=3, warmup=1, out="fine_icp_bench.json")
    args = ap.parse_args()
    import torch

    import bev_amd
    import fineicp_lib as fl

    fl.build()
    p = bev_amd.params_for_sensor("HDL_64E")
    F0, M, S = args.frames, args.moved, p.slots
    dev = torch.device("cuda:0")
    frames = bl.sweeps(p, F0)
    ctx = bev_amd.BevContext(p, device=0, max_batch=args.sub_batch, max_points=max(len(f) for f in frames))
    rng, yaw, tr = bl.world_draws(M)
    frames += bl.moved_copies(ctx, frames, yaw, tr)
    F = len(frames)
    offs, d_in = bl.upload(frames, dev)
    del frames
    d_ord, d_multi, d_single = bl.bev_outputs(p, F, dev)
    stride = bev_amd.regfront_max_out(S)
    d_pn = torch.empty(F * stride * 12, dtype=torch.float32, device=dev)
    d_cnt = torch.empty(F, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.process_device(F, d_in.data_ptr(), offs, d_ord.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
    ctx.registration_front_device(F, d_ord.data_ptr(), None, d_pn.data_ptr(), stride, d_cnt.data_ptr())
    ctx.synchronize()

    lists = {}
    a = np.zeros(F0, bev_amd.MATCH_DTYPE)
    a["query_idx"] = np.arange(F0)
    a["match_idx"] = np.where(np.arange(F0) % 2 == 0, (np.arange(F0) + 1) % F0, rng.integers(0, F0, F0))
    a["angle_guess"] = rng.uniform(-180, 180, F0).astype(np.float32)
    lists["bench_icp"] = a
    lists["moved_copies"] = bl.moved_copy_pairs(SimpleNamespace(rng=rng, yaw=yaw, F0=F0, M=M))
    R = bev_amd.ICP_RESULT_DTYPE.itemsize
    out = {"metric": "fine_icp_matches_per_s", "sensor": "HDL_64E", "frames": F, "steps": args.steps,
           "warmup": args.warmup, "runs": {}}
    for name, m in lists.items():
        n = len(m)
        d_coarse = torch.zeros(n * 2 * R, dtype=torch.uint8, device=dev)
        d_best = torch.zeros(n, dtype=torch.int32, device=dev)
        ctx.coarse_registration_device(F, d_pn.data_ptr(), stride, d_cnt.data_ptr(), m, d_coarse.data_ptr(),
                                       d_best.data_ptr())
        ctx.synchronize()
        d_res = torch.zeros(n * R, dtype=torch.uint8, device=dev)
        for tool in ("top_part", "whole"):
            def step():
                if tool == "top_part":
                    ctx.fine_registration_device(F, d_ord.data_ptr(), None, m, d_res.data_ptr(), d_coarse.data_ptr(),
                                                 d_best.data_ptr())
                else:
                    ctx.fine_registration_device(F, d_ord.data_ptr(), None, m, d_res.data_ptr(),
                                                 params=bev_amd.icp_whole_defaults())

            fenced, unfenced = bl.timed(ctx, step, args.steps, args.warmup)
            kernels = bl.kernel_ms(ctx, step, "k_fine")
            res = d_res.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE)
            it = res["iterations"]
            out["runs"][f"{name}/{tool}"] = {
                "matches": n, "fenced_median_ms": fenced * 1e3, "fenced_matches_per_s": n / fenced,
                "unfenced_mean_ms": unfenced * 1e3, "unfenced_matches_per_s": n / unfenced,
                "iterations": {"mean": float(it.mean()), "p50": float(np.percentile(it, 50)),
                               "p90": float(np.percentile(it, 90)), "max": int(it.max())},
                "states": np.bincount(res["state"], minlength=6).tolist(),
                "success_fitness_le_1_5": int((~(res["fitness"] > 1.5)).sum()),
                "kernels_ms_per_step": kernels,
            }
    ordered = d_ord[: 4 * S * 32].cpu().numpy().view(bev_amd.POINT_DTYPE).reshape(4, S)
    vox = [fl.voxel_irct(o) for o in ordered]
    out["voxels_per_full_cloud_sample"] = [len(v) for v in vox]
    t = time.perf_counter()
    for k in range(args.cpu_matches):
        fl.run(vox[k], vox[(k + 1) % 4], fl.tool_guess(0.0), fl.params(**fl.WHOLE))
    out["checker_single_core_matches_per_s"] = args.cpu_matches / (time.perf_counter() - t)
    ctx.close()
    bl.emit(out, args)


if __name__ == "__main__":
    main()
