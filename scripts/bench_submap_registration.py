"""Scan-to-map fine ICP (bev_submap_registration_device_resident) beside the pair call
(bev_fine_registration_device_resident) on the same matches, in one process.

    python scripts/bench_submap_registration.py [--frames 1000] [--moved 500] [--rounds 3] [--window-matches 1:500,5:100,21:40]
                                                [--out profiles/submap_registration_bench.json]

Frames, moved copies, matches, windows and protocol are benchlib's; both calls read the d_ordered layout, under the whole
tool's settings.  Per window, --rounds alternations of [pair call, submap call]: the medians, matches/s, the ratio; then one
profiled step of each: per-kernel ms, the results' iteration counts, and the ICP kernels' time over the sum of those counts
(every match is one workgroup, and a launch's workgroups run side by side: a kernel's time over the MEAN count is the time of
one iteration of the launch).  One JSON line."""
import argparse
import json
import statistics
import sys

import numpy as np

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    bl.std_args(ap, frames=1000, moved=500, window_matches="1:500,5:100,21:40", sub_batch=500, rounds=3,
                out="submap_registration_bench.json")
    args = ap.parse_args()
    import torch

    import bev_amd

    w = bl.registration_world(args)
    ctx, d_ord, F, M, dev = w.ctx, w.d_ord, w.F, w.M, w.dev
    pairs = bl.moved_copy_pairs(w)
    R = bev_amd.ICP_RESULT_DTYPE.itemsize
    prm = bev_amd.icp_whole_defaults()
    out = {"metric": "submap_registration_matches_per_s", "sensor": "HDL_64E", "frames": F, "records_per_frame": w.S,
           "rounds": args.rounds, "settings": "whole", "windows": {}}
    for W, n in bl.parse_window_matches(args.window_matches, M):
        m_pair = pairs[:n].copy()
        m_map = bl.map_matches(pairs, n)
        map_offs, entry_frame, entry_pose = bl.cyclic_windows(w.rng, w.F0, M, n, W)
        d_pair = torch.zeros(n * R, dtype=torch.uint8, device=dev)
        d_map = torch.zeros(n * R, dtype=torch.uint8, device=dev)
        pair = lambda: ctx.fine_registration_device(F, d_ord.data_ptr(), None, m_pair, d_pair.data_ptr(), params=prm)
        submap = lambda: ctx.submap_registration_device(F, d_ord.data_ptr(), None, map_offs, entry_frame, entry_pose, m_map,
                                                        d_map.data_ptr(), params=prm)
        t_pair, t_map = bl.alternate(ctx, pair, submap, args.rounds)
        k_pair, k_map = bl.kernel_ms(ctx, pair, "k_fine"), bl.kernel_ms(ctx, submap, ("k_fine", "k_submap"))
        r_pair = d_pair.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE)
        r_map = d_map.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE)
        it_pair, it_map = int(r_pair["iterations"].sum()), int(r_map["iterations"].sum())
        med_pair, med_map = statistics.median(t_pair), statistics.median(t_map)
        out["windows"][str(W)] = {
            "matches": n, "entries": int(n * W), "identical_to_pair_call": bool(W == 1 and r_pair.tobytes() == r_map.tobytes()),
            "pair_ms": [t * 1e3 for t in t_pair], "submap_ms": [t * 1e3 for t in t_map],
            "pair_median_ms": med_pair * 1e3, "submap_median_ms": med_map * 1e3, "submap_over_pair": med_map / med_pair,
            "pair_matches_per_s": n / med_pair, "submap_matches_per_s": n / med_map,
            "pair_kernels_ms": k_pair, "submap_kernels_ms": k_map,
            "pair_iterations": {"sum": it_pair, "mean": it_pair / n}, "submap_iterations": {"sum": it_map, "mean": it_map / n},
            "k_fine_icp_us_per_iteration_match": k_pair.get("k_fine_icp", 0.0) * 1e3 / max(it_pair, 1),
            "k_submap_icp_us_per_iteration_match": k_map.get("k_submap_icp", 0.0) * 1e3 / max(it_map, 1),
            "submap_states": np.bincount(r_map["state"], minlength=6).tolist(),
            "submap_success_fitness_le_1_5": int((~(r_map["fitness"] > 1.5)).sum()),
            "pair_success_fitness_le_1_5": int((~(r_pair["fitness"] > 1.5)).sum()),
        }
        print(f"window {W}: {json.dumps(out['windows'][str(W)])}", file=sys.stderr, flush=True)
    ctx.close()
    bl.emit(out, args)


if __name__ == "__main__":
    main()
