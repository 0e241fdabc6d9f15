"""Scan-to-map coarse ICP against the thinned top part over the union of a map's moved full clouds
(bev_submap_top_part_coarse_registration_device_resident) beside the parent's call on the same matches at the same
pn_leaf (bev_submap_coarse_voxel_registration_device_resident: the thinned concatenation of each sweep's own top part, §6q), in
one process; and the selection stages of the new call beside the front end's own top stage on the same sweeps.

    python scripts/bench_submap_top_union.py [--frames 1000] [--moved 500] [--rounds 3] [--pn-leaf 0.2]
                                             [--window-matches 1:500,5:100,21:40] [--out profiles/submap_top_union_bench.json]

Frames, moved copies, matches, windows and protocol are benchlib's: the marked clouds stay on the device (they are the new
call's full clouds) beside the front end's rows (the queries of both calls).  The yardstick is the parent's code in the same
process, never an absolute figure.  Per window: --rounds alternations of [concatenation call, union call]: the medians and
ranges, the ratio (a different target, not a faster copy: no ratio is required of it), the rows per map of both targets, one
profiled step of each (per-kernel ms, the ICP kernel's time over the sum of the iteration counts), states, choices and their
agreement; the front end's time on the call's frames beside it.  Then the selection stages alone: one profiled cloud call with
pn_leaf = 0 (keys, cells, select, compaction, sort, rows: per map) beside one profiled front end on the W sweeps of one window
(k_rf_cells + k_rf_top: both rank the same records and select the same number), each the median of --rounds.  One JSON line."""
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
                out="submap_top_union_bench.json")
    args = ap.parse_args()
    import torch

    import bev_amd

    w = bl.registration_world(args)
    ctx, d_ord, F, M, S, dev = w.ctx, w.d_ord, w.F, w.M, w.S, w.dev
    stride, d_pn, d_cnt = bl.front_end(w)
    whole_front = lambda: ctx.registration_front_device(F, d_ord.data_ptr(), None, d_pn.data_ptr(), stride, d_cnt.data_ptr())
    # once more, fenced: the front end's time per frame at a batch's throughput
    front_ms_per_frame = bl.fenced(ctx, whole_front, log=False) * 1e3 / F
    counts = d_cnt.cpu().numpy()
    labelled = int((np.frombuffer(d_ord[: S * 32].cpu().numpy().tobytes(), bev_amd.POINT_DTYPE)["label"] != 0).sum())
    pn_stride = stride
    front_k = bl.kernel_ms(ctx, whole_front, "k_rf")
    top_stage_ms_per_frame = (front_k.get("k_rf_cells", 0.0) + front_k.get("k_rf_top", 0.0)) / F

    pairs = bl.moved_copy_pairs(w)
    R = bev_amd.ICP_RESULT_DTYPE.itemsize
    out = {"metric": "submap_top_union_matches_per_s", "sensor": "HDL_64E", "frames": F, "stride": int(pn_stride),
           "rows_per_frame": {"mean": float(counts.mean()), "max": int(counts.max())}, "rounds": args.rounds, "records_per_frame": int(S),
           "labelled_records_of_frame_0": labelled, "front_end_ms_per_frame_in_a_batch": front_ms_per_frame,
           "front_end_kernels_ms_of_all_frames": front_k, "pn_leaf": args.pn_leaf, "radius": args.radius, "settings": "coarse defaults", "windows": {}}
    profiled = lambda step: bl.kernel_ms(ctx, step, ("k_icp", "k_submap", "k_rf"))
    for W, n in bl.parse_window_matches(args.window_matches, M):
        m_map = bl.map_matches(pairs, n)
        map_offs, entry_frame, entry_pose = bl.cyclic_windows(w.rng, w.F0, M, n, W)
        d_cat, d_uni = (torch.zeros(2 * n * R, dtype=torch.uint8, device=dev) for _ in range(2))
        b_cat, b_uni = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
        cat = lambda: ctx.submap_coarse_voxel_registration_device(
            F, d_pn.data_ptr(), pn_stride, d_cnt.data_ptr(), map_offs, entry_frame, entry_pose, m_map, d_cat.data_ptr(),
            b_cat.data_ptr(), args.pn_leaf, args.radius)
        uni = lambda: ctx.submap_top_part_coarse_registration_device(
            F, d_ord.data_ptr(), None, d_pn.data_ptr(), pn_stride, d_cnt.data_ptr(), map_offs, entry_frame, entry_pose, m_map,
            d_uni.data_ptr(), b_uni.data_ptr(), args.pn_leaf, args.radius)
        t_cat, t_uni = bl.alternate(ctx, cat, uni, args.rounds)
        k_cat, k_uni = profiled(cat), profiled(uni)
        r_cat = d_cat.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE)
        r_uni = d_uni.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE)
        best_cat, best_uni = b_cat.cpu().numpy(), b_uni.cpu().numpy()
        it_cat, it_uni = int(r_cat["iterations"].sum()), int(r_uni["iterations"].sum())
        med_cat, med_uni = statistics.median(t_cat), statistics.median(t_uni)
        # the rows of both targets: the cloud calls' counts (outside the timed steps)
        cap = W * pn_stride
        d_rows = torch.empty(n * cap * 48, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(n, dtype=torch.int32, device=dev)
        ctx.submap_pn_cloud_device(F, d_pn.data_ptr(), pn_stride, d_cnt.data_ptr(), map_offs, entry_frame, entry_pose, args.pn_leaf, cap,
                                   d_rows.data_ptr(), d_n.data_ptr(), args.radius)
        ctx.synchronize()
        rows_cat = d_n.cpu().numpy().copy()
        top_cap = bev_amd.submap_top_part_max_out(W * S)
        assert top_cap <= cap
        top_cloud = lambda leaf: ctx.submap_top_part_cloud_device(F, d_ord.data_ptr(), None, map_offs, entry_frame, entry_pose, leaf,
                                                                  top_cap, d_rows.data_ptr(), d_n.data_ptr(), args.radius)
        top_cloud(args.pn_leaf)
        ctx.synchronize()
        rows_uni = d_n.cpu().numpy().copy()
        # the selection stages alone (pn_leaf = 0: steps 1 - 6 and the copy out) beside the front end's top stage on one window's sweeps
        sel_ms, sel_k = [], None
        for _ in range(args.rounds):
            sel_k = profiled(lambda: top_cloud(0.0))
            sel_ms.append(sum(v for k, v in sel_k.items() if k != "k_submap_pn_out"))
        rows_top = d_n.cpu().numpy().copy()
        first = int(entry_frame[:W].min())
        span = list(range(first, min(first + W, F)))     # W consecutive moved sweeps (the windows are cyclic: the same kind of sweeps)
        d_pn2 = torch.empty(len(span) * stride * 48, dtype=torch.uint8, device=dev)
        d_cnt2 = torch.zeros(len(span), dtype=torch.int32, device=dev)
        front = lambda: ctx.registration_front_device(len(span), d_ord.data_ptr() + first * S * 32, None, d_pn2.data_ptr(), stride,
                                                      d_cnt2.data_ptr())
        rf_ms, rf_k = [], None
        for _ in range(args.rounds):
            rf_k = profiled(front)
            rf_ms.append(rf_k.get("k_rf_cells", 0.0) + rf_k.get("k_rf_top", 0.0))
        named = sorted({int(f) for f in entry_frame} | {int(q) for q in m_map["query_idx"]})
        del d_rows, d_n, d_pn2, d_cnt2
        new_stages = ("k_submap_top_keys", "k_submap_top_cells", "k_submap_top_hist", "k_submap_top_scan", "k_submap_top_compact",
                      "k_submap_top_rows", "k_submap_top_overflow")
        sel_per_map = statistics.median(sel_ms) / n
        rf_per_window = statistics.median(rf_ms) * W / len(span)
        out["windows"][str(W)] = {
            "matches": n, "problems": 2 * n, "entries": int(n * W), "union_records_per_map": int(W * S),
            "rows_concatenation": {"mean": float(rows_cat.mean()), "max": int(rows_cat.max()), "sum": int(rows_cat.sum())},
            "rows_union": {"mean": float(rows_uni.mean()), "max": int(rows_uni.max()), "sum": int(rows_uni.sum())},
            "rows_top_before_thinning": {"mean": float(rows_top.mean()), "max": int(rows_top.max())},
            "concatenation_ms": [t * 1e3 for t in t_cat], "union_ms": [t * 1e3 for t in t_uni],
            "concatenation_median_ms": med_cat * 1e3, "union_median_ms": med_uni * 1e3,
            "concatenation_range_ms": [min(t_cat) * 1e3, max(t_cat) * 1e3], "union_range_ms": [min(t_uni) * 1e3, max(t_uni) * 1e3],
            "union_over_concatenation": med_uni / med_cat,
            "frames_named": len(named), "front_end_ms_of_named_frames": front_ms_per_frame * len(named),
            "front_end_ms_per_frame_of_one_window_alone": sum(v for k, v in rf_k.items() if k.startswith("k_rf")) / len(span),
            "front_end_top_stage_ms_of_w_frames_at_batch_throughput": top_stage_ms_per_frame * W,
            "selection_over_front_end_top_stage_at_batch_throughput": sel_per_map / max(top_stage_ms_per_frame * W, 1e-9),
            "concatenation_matches_per_s": n / med_cat, "union_matches_per_s": n / med_uni,
            "concatenation_kernels_ms": k_cat, "union_kernels_ms": k_uni,
            "union_new_kernels_ms": sum(k_uni.get(k, 0.0) for k in new_stages),
            "union_new_kernels_share": sum(k_uni.get(k, 0.0) for k in new_stages) / max(sum(k_uni.values()), 1e-9),
            "selection_kernels_ms": sel_k, "selection_ms_rounds": sel_ms, "selection_ms_per_map": sel_per_map,
            "front_end_top_stage_kernels_ms": {k: v for k, v in rf_k.items() if k.startswith("k_rf")}, "front_end_top_stage_ms_rounds": rf_ms,
            "front_end_top_stage_ms_per_window_of_sweeps": rf_per_window,
            "selection_over_front_end_top_stage": sel_per_map / max(rf_per_window, 1e-9),
            "concatenation_iterations": {"sum": it_cat, "mean": it_cat / (2 * n)}, "union_iterations": {"sum": it_uni, "mean": it_uni / (2 * n)},
            "concatenation_icp_us_per_iteration_problem": k_cat.get("k_submap_coarse_icp", 0.0) * 1e3 / max(it_cat, 1),
            "union_icp_us_per_iteration_problem": k_uni.get("k_submap_coarse_icp", 0.0) * 1e3 / max(it_uni, 1),
            "concatenation_states": np.bincount(r_cat["state"], minlength=6).tolist(), "union_states": np.bincount(r_uni["state"], minlength=6).tolist(),
            "concatenation_best": np.bincount(best_cat, minlength=2).tolist(), "union_best": np.bincount(best_uni, minlength=2).tolist(),
            "best_agree": int((best_cat == best_uni).sum()),
            "concatenation_fitness": bl.best_fitness(r_cat, best_cat), "union_fitness": bl.best_fitness(r_uni, best_uni),
        }
        print(f"window {W}: {json.dumps(out['windows'][str(W)])}", file=sys.stderr, flush=True)
    ctx.close()
    bl.emit(out, args)


if __name__ == "__main__":
    main()
