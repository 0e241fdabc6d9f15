"""Scan-to-map coarse ICP against maps thinned over their union (bev_submap_coarse_voxel_registration_device_resident with
pn_leaf > 0) beside the same call with pn_leaf = 0 (bev_submap_coarse_registration_device_resident's code) on the
same matches, in one process.

    python scripts/bench_submap_pn_voxel_registration.py [--frames 1000] [--moved 500] [--rounds 3] [--pn-leaf 0.2]
                                                         [--window-matches 1:500,5:100,21:40]
                                                         [--out profiles/submap_pn_voxel_registration_bench.json]

Frames, moved copies, matches, windows and protocol are benchlib's, on the front end's rows as in
bench_submap_coarse_registration.py (d_ordered is released before anything is timed).  The yardstick is the pn_leaf = 0 call,
never an absolute figure.  Per window: --rounds alternations of [pn_leaf = 0 call, thinned call]: the medians and ranges,
matches/s, the ratio; the maps' rows before and after thinning (bev_submap_pn_cloud_device_resident's counts); then one
profiled step of each: per-kernel ms, the results' iteration counts, the ICP kernel's time over the sum of those counts; the
states, the choices and the fitness on both sides.  One JSON line."""
import argparse
import json
import statistics
import sys

import numpy as np

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn-leaf", type=float, default=0.2)
    ap.add_argument("--radius", type=float, default=2.0)
    bl.std_args(ap, frames=1000, moved=500, window_matches="1:500,5:100,21:40", sub_batch=500, rounds=3,
                out="submap_pn_voxel_registration_bench.json")
    args = ap.parse_args()
    import torch

    import bev_amd

    w = bl.registration_world(args)
    ctx, F, M, dev = w.ctx, w.F, w.M, w.dev
    pn_stride, d_pn, d_cnt = bl.front_end(w)
    del w.d_ord
    counts = d_cnt.cpu().numpy()
    pairs = bl.moved_copy_pairs(w)
    R = bev_amd.ICP_RESULT_DTYPE.itemsize
    out = {"metric": "submap_pn_voxel_registration_matches_per_s", "sensor": "HDL_64E", "frames": F, "stride": int(pn_stride),
           "rows_per_frame": {"mean": float(counts.mean()), "max": int(counts.max())}, "rounds": args.rounds,
           "pn_leaf": args.pn_leaf, "radius": args.radius, "settings": "coarse defaults", "windows": {}}
    for W, n in bl.parse_window_matches(args.window_matches, M):
        m_map = bl.map_matches(pairs, n)
        map_offs, entry_frame, entry_pose = bl.cyclic_windows(w.rng, w.F0, M, n, W)
        d_plain, d_thin = (torch.zeros(2 * n * R, dtype=torch.uint8, device=dev) for _ in range(2))
        b_plain, b_thin = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
        call = lambda d_res, d_best, leaf: ctx.submap_coarse_voxel_registration_device(
            F, d_pn.data_ptr(), pn_stride, d_cnt.data_ptr(), map_offs, entry_frame, entry_pose, m_map, d_res.data_ptr(),
            d_best.data_ptr(), leaf, args.radius)
        plain = lambda: call(d_plain, b_plain, 0.0)
        thin = lambda: call(d_thin, b_thin, args.pn_leaf)
        t_plain, t_thin = bl.alternate(ctx, plain, thin, args.rounds)
        k_plain, k_thin = (bl.kernel_ms(ctx, step, ("k_icp", "k_submap")) for step in (plain, thin))
        r_plain = d_plain.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE)
        r_thin = d_thin.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE)
        best_plain, best_thin = b_plain.cpu().numpy(), b_thin.cpu().numpy()
        it_plain, it_thin = int(r_plain["iterations"].sum()), int(r_thin["iterations"].sum())
        med_plain, med_thin = statistics.median(t_plain), statistics.median(t_thin)
        rows_before = np.array([counts[entry_frame[i * W:(i + 1) * W]].sum() for i in range(n)])
        # the rows after thinning: the cloud call's counts (outside the timed steps)
        cap = W * pn_stride
        d_rows = torch.empty(n * cap * 48, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(n, dtype=torch.int32, device=dev)
        ctx.submap_pn_cloud_device(F, d_pn.data_ptr(), pn_stride, d_cnt.data_ptr(), map_offs, entry_frame, entry_pose, args.pn_leaf, cap,
                                   d_rows.data_ptr(), d_n.data_ptr(), args.radius)
        ctx.synchronize()
        rows_after = d_n.cpu().numpy()
        del d_rows, d_n
        new_stages = ("k_submap_pn_move", "k_submap_pn_keys", "k_submap_vox_tile", "k_submap_vox_global", "k_submap_pn_finish",
                      "k_submap_pn_normals", "k_submap_pn_grid")
        out["windows"][str(W)] = {
            "matches": n, "problems": 2 * n, "entries": int(n * W),
            "rows_before": {"mean": float(rows_before.mean()), "max": int(rows_before.max()), "sum": int(rows_before.sum())},
            "rows_after": {"mean": float(rows_after.mean()), "max": int(rows_after.max()), "sum": int(rows_after.sum())},
            "plain_ms": [t * 1e3 for t in t_plain], "thinned_ms": [t * 1e3 for t in t_thin],
            "plain_median_ms": med_plain * 1e3, "thinned_median_ms": med_thin * 1e3,
            "plain_range_ms": [min(t_plain) * 1e3, max(t_plain) * 1e3], "thinned_range_ms": [min(t_thin) * 1e3, max(t_thin) * 1e3],
            "thinned_over_plain": med_thin / med_plain,
            "plain_matches_per_s": n / med_plain, "thinned_matches_per_s": n / med_thin,
            "plain_kernels_ms": k_plain, "thinned_kernels_ms": k_thin,
            "thinned_new_stages_ms": sum(k_thin.get(k, 0.0) for k in new_stages),
            "plain_iterations": {"sum": it_plain, "mean": it_plain / (2 * n)}, "thinned_iterations": {"sum": it_thin, "mean": it_thin / (2 * n)},
            "plain_icp_us_per_iteration_problem": k_plain.get("k_submap_coarse_icp", 0.0) * 1e3 / max(it_plain, 1),
            "thinned_icp_us_per_iteration_problem": k_thin.get("k_submap_coarse_icp", 0.0) * 1e3 / max(it_thin, 1),
            "plain_states": np.bincount(r_plain["state"], minlength=6).tolist(), "thinned_states": np.bincount(r_thin["state"], minlength=6).tolist(),
            "plain_best": np.bincount(best_plain, minlength=2).tolist(), "thinned_best": np.bincount(best_thin, minlength=2).tolist(),
            "best_agree": int((best_plain == best_thin).sum()),
            "plain_fitness": bl.best_fitness(r_plain, best_plain), "thinned_fitness": bl.best_fitness(r_thin, best_thin),
        }
        print(f"window {W}: {json.dumps(out['windows'][str(W)])}", file=sys.stderr, flush=True)
    ctx.close()
    bl.emit(out, args)


if __name__ == "__main__":
    main()
