"""Scan-to-map fine ICP against maps thinned by a voxel grid over their union (bev_submap_voxel_registration_device_resident
with map_leaf 0.2) beside the same call with map_leaf 0 — §6k's code path, the yardstick — on the same
matches, in one process.

    python scripts/bench_submap_voxel_registration.py [--frames 1000] [--moved 500] [--rounds 3] [--map-leaf 0.2]
                                                      [--window-matches 1:500,5:100,21:40]
                                                      [--out profiles/submap_voxel_registration_bench.json]

Frames, moved copies, matches, windows and protocol are benchlib's (§6k's protocol), on the d_ordered layout under the whole
tool's settings.  Per window: --rounds alternations of [map_leaf 0, map_leaf --map-leaf]: the medians with min and max, the
ratio; then one profiled step of each: per-kernel ms (move, keys, the sort's stages together, centroids + grid, ICP), mean
iterations, the ICP kernel's time over the sum of the iteration counts, matches with fitness <= 1.5 on each side and how many
matches differ in that verdict; and, from bev_submap_voxel_cloud_device_resident on the first --count-maps maps, the points
per map before and after thinning.  One JSON line."""
import argparse
import json
import statistics
import sys

import numpy as np

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-leaf", type=float, default=0.2)
    ap.add_argument("--count-maps", type=int, default=8, help="maps whose point counts the cloud call reports")
    bl.std_args(ap, frames=1000, moved=500, window_matches="1:500,5:100,21:40", sub_batch=500, rounds=3,
                out="submap_voxel_registration_bench.json")
    args = ap.parse_args()
    import torch

    import bev_amd

    w = bl.registration_world(args)
    ctx, d_ord, F, M, S, dev = w.ctx, w.d_ord, w.F, w.M, w.S, w.dev
    pairs = bl.moved_copy_pairs(w)
    R = bev_amd.ICP_RESULT_DTYPE.itemsize
    prm = bev_amd.icp_whole_defaults()
    out = {"metric": "submap_voxel_registration_matches_per_s", "sensor": "HDL_64E", "frames": F, "records_per_frame": S,
           "rounds": args.rounds, "settings": "whole", "map_leaf": args.map_leaf, "windows": {}}
    spread = lambda ts: {"median": statistics.median(ts) * 1e3, "min": min(ts) * 1e3, "max": max(ts) * 1e3}
    for W, n in bl.parse_window_matches(args.window_matches, M):
        m_map = bl.map_matches(pairs, n)
        map_offs, entry_frame, entry_pose = bl.cyclic_windows(w.rng, w.F0, M, n, W)
        d_plain = torch.zeros(n * R, dtype=torch.uint8, device=dev)
        d_thin = torch.zeros(n * R, dtype=torch.uint8, device=dev)
        call = lambda d, leaf: ctx.submap_voxel_registration_device(F, d_ord.data_ptr(), None, map_offs, entry_frame, entry_pose,
                                                                    m_map, d.data_ptr(), leaf, params=prm)
        plain = lambda: call(d_plain, 0.0)
        thin = lambda: call(d_thin, args.map_leaf)
        t_plain, t_thin = bl.alternate(ctx, plain, thin, args.rounds)
        k_plain, k_thin = (bl.kernel_ms(ctx, step, ("k_fine", "k_submap")) for step in (plain, thin))
        r_plain = d_plain.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE)
        r_thin = d_thin.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE)
        it_plain, it_thin = int(r_plain["iterations"].sum()), int(r_thin["iterations"].sum())
        ok_plain, ok_thin = ~(r_plain["fitness"] > 1.5), ~(r_thin["fitness"] > 1.5)
        # the points per map, before and after: the cloud call on the first maps
        c = min(n, args.count_maps)
        d_out = torch.empty(c * W * S * 16, dtype=torch.uint8, device=dev)
        d_cnt = torch.zeros(2 * c, dtype=torch.int32, device=dev)
        for k, leaf in enumerate((0.0, args.map_leaf)):
            ctx.submap_voxel_cloud_device(F, d_ord.data_ptr(), None, map_offs[: c + 1], entry_frame[: c * W], entry_pose[: c * W], leaf,
                                          W * S, d_out.data_ptr(), d_cnt.data_ptr() + 4 * c * k)
        ctx.synchronize()
        counts = d_cnt.cpu().numpy().reshape(2, c)
        del d_out
        sort_ms = k_thin.get("k_submap_vox_tile", 0.0) + k_thin.get("k_submap_vox_global", 0.0)
        med_plain, med_thin = statistics.median(t_plain), statistics.median(t_thin)
        out["windows"][str(W)] = {
            "matches": n, "entries": int(n * W),
            "plain_ms": spread(t_plain), "thin_ms": spread(t_thin), "thin_over_plain": med_thin / med_plain,
            "plain_matches_per_s": n / med_plain, "thin_matches_per_s": n / med_thin,
            "plain_kernels_ms": k_plain, "thin_kernels_ms": k_thin,
            "thin_stages_ms": {"move": k_thin.get("k_submap_vox_move", 0.0), "keys": k_thin.get("k_submap_vox_keys", 0.0),
                               "sort": sort_ms, "centroids_grid": k_thin.get("k_submap_vox_finish", 0.0),
                               "icp": k_thin.get("k_submap_icp", 0.0)},
            "plain_iterations": {"sum": it_plain, "mean": it_plain / n}, "thin_iterations": {"sum": it_thin, "mean": it_thin / n},
            "plain_icp_us_per_iteration_match": k_plain.get("k_submap_icp", 0.0) * 1e3 / max(it_plain, 1),
            "thin_icp_us_per_iteration_match": k_thin.get("k_submap_icp", 0.0) * 1e3 / max(it_thin, 1),
            "points_per_map_before": {"mean": float(counts[0].mean()), "min": int(counts[0].min()), "max": int(counts[0].max())},
            "points_per_map_after": {"mean": float(counts[1].mean()), "min": int(counts[1].min()), "max": int(counts[1].max())},
            "maps_counted": c,
            "plain_states": np.bincount(r_plain["state"], minlength=6).tolist(),
            "thin_states": np.bincount(r_thin["state"], minlength=6).tolist(),
            "plain_success_fitness_le_1_5": int(ok_plain.sum()), "thin_success_fitness_le_1_5": int(ok_thin.sum()),
            "matches_whose_verdict_differs": int((ok_plain != ok_thin).sum()),
            "identical_results": bool(r_plain.tobytes() == r_thin.tobytes()),
        }
        print(f"window {W}: {json.dumps(out['windows'][str(W)])}", file=sys.stderr, flush=True)
    ctx.close()
    bl.emit(out, args)


if __name__ == "__main__":
    main()
