"""Scan-to-map coarse ICP against the thinned top part over the union of a map's moved full clouds
(bev_submap_top_part_coarse_registration_device_resident) beside the parent's call on the same matches at the same
pn_leaf (bev_submap_coarse_voxel_registration_device_resident: the thinned concatenation of each sweep's own top part, §6q), in
one process; and the selection stages of the new call beside the front end's own top stage on the same sweeps.

    python scripts/bench_submap_top_union.py [--frames 1000] [--moved 500] [--rounds 3] [--pn-leaf 0.2]
                                             [--window-matches 1:500,5:100,21:40] [--out profiles/submap_top_union_bench.json]

Frames, moved copies, matches and windows are scripts/bench_submap_pn_voxel_registration.py's: bench.py's synthetic HDL_64E
sweeps through bev_process_device_resident (the marked clouds stay on the device: they are the new call's full clouds) and the
registration front end (leaf 0.2, radius 2: the queries of both calls), frame i against a map of the moved copies
i - W // 2 .. i + W // 2 (cyclic), the centre under the identity, the others under a seeded planar matrix within +-1 degree and
+-0.3 m.  The yardstick is the parent's code in the same process, never an absolute figure.  Per window: one warm-up of each
call, --rounds alternations of [concatenation call, union call], each fenced (launch, bev_synchronize): the medians and ranges,
the ratio (a different target, not a faster copy: no ratio is required of it), the rows per map of both targets, one profiled
step of each (per-kernel ms, the ICP kernel's time over the sum of the iteration counts), states, choices and their agreement;
the front end's time on the call's frames beside it.  Then the selection stages alone: one profiled cloud call with
pn_leaf = 0 (keys, cells, select, compaction, sort, rows: per map) beside one profiled front end on the W sweeps of one window
(k_rf_cells + k_rf_top: both rank the same records and select the same number), each the median of --rounds.  One JSON line."""
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
    ap.add_argument("--moved", type=int, default=500)
    ap.add_argument("--window-matches", default="1:500,5:100,21:40", help="W:n pairs: the window sizes and their matches")
    ap.add_argument("--sub-batch", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pn-leaf", type=float, default=0.2)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--out", default=str(REPO / "profiles" / "submap_top_union_bench.json"))
    args = ap.parse_args()
    import torch

    import bev_amd
    from bev_amd import synth

    p = bev_amd.params_for_sensor("HDL_64E")
    F0, M, S = args.frames, args.moved, p.slots
    dev = torch.device("cuda:0")
    with ThreadPoolExecutor(16) as ex:
        frames = list(ex.map(lambda i: synth.sweep(p, i, keep=0.98, n_dup=5000), range(F0)))
    n_max = max(len(f) for f in frames)
    ctx = bev_amd.BevContext(p, device=0, max_batch=args.sub_batch, max_points=n_max)
    rng = np.random.default_rng(2026)
    yaw = rng.uniform(-20, 20, M).astype(np.float32)
    tr = rng.uniform(-1.5, 1.5, (M, 2)).astype(np.float32)
    frames += [ctx.transform_cloud(frames[i], bev_amd.yaw_translate_matrix(float(tr[i, 0]), float(tr[i, 1]), 0.0,
                                                                           float(yaw[i]))) for i in range(M)]
    F = len(frames)
    offs = np.zeros(F + 1, np.uint64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    d_in = torch.from_numpy(np.concatenate(frames).view(np.uint8).reshape(-1)).to(dev)
    del frames
    d_ord = torch.empty(F * S * 32, dtype=torch.uint8, device=dev)
    d_multi = torch.empty(F * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    d_single = torch.empty(F * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.process_device(F, d_in.data_ptr(), offs, d_ord.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
    ctx.synchronize()
    del d_in, d_multi, d_single
    stride = bev_amd.regfront_max_out(S)
    d_pn = torch.empty(F * stride * 48, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(F, dtype=torch.int32, device=dev)
    ctx.registration_front_device(F, d_ord.data_ptr(), None, d_pn.data_ptr(), stride, d_cnt.data_ptr())
    ctx.synchronize()
    t_front = time.perf_counter()       # once more, fenced: the front end's time per frame at a batch's throughput
    ctx.registration_front_device(F, d_ord.data_ptr(), None, d_pn.data_ptr(), stride, d_cnt.data_ptr())
    ctx.synchronize()
    front_ms_per_frame = (time.perf_counter() - t_front) * 1e3 / F
    counts = d_cnt.cpu().numpy()
    labelled = int((np.frombuffer(d_ord[: S * 32].cpu().numpy().tobytes(), bev_amd.POINT_DTYPE)["label"] != 0).sum())
    pn_stride = stride

    ctx.profile_reset()
    ctx.profile_enable(True)
    ctx.registration_front_device(F, d_ord.data_ptr(), None, d_pn.data_ptr(), stride, d_cnt.data_ptr())
    ctx.synchronize()
    front_k = {s_["name"]: s_["total_ms"] for s_ in ctx.profile_get() if s_["name"].startswith("k_rf")}
    ctx.profile_enable(False)
    top_stage_ms_per_frame = (front_k.get("k_rf_cells", 0.0) + front_k.get("k_rf_top", 0.0)) / F

    pairs = np.zeros(M, bev_amd.MATCH_DTYPE)
    pairs["query_idx"] = np.arange(M)
    pairs["match_idx"] = F0 + np.arange(M)
    pairs["angle_guess"] = yaw + rng.uniform(-2, 2, M).astype(np.float32)
    R = bev_amd.ICP_RESULT_DTYPE.itemsize
    identity = np.eye(3, 4, dtype=np.float32).reshape(12)
    out = {"metric": "submap_top_union_matches_per_s", "sensor": "HDL_64E", "frames": F, "stride": int(pn_stride),
           "rows_per_frame": {"mean": float(counts.mean()), "max": int(counts.max())}, "rounds": args.rounds, "records_per_frame": int(S),
           "labelled_records_of_frame_0": labelled, "front_end_ms_per_frame_in_a_batch": front_ms_per_frame,
           "front_end_kernels_ms_of_all_frames": front_k, "pn_leaf": args.pn_leaf, "radius": args.radius, "settings": "coarse defaults", "windows": {}}

    def fenced(step):
        t = time.perf_counter()
        step()
        ctx.synchronize()
        t = time.perf_counter() - t
        print(f"  step {t * 1e3:.1f} ms", file=sys.stderr, flush=True)
        return t

    def profiled(step):
        ctx.profile_reset()
        ctx.profile_enable(True)
        step()
        ctx.synchronize()
        k = {s["name"]: s["total_ms"] for s in ctx.profile_get() if s["name"].startswith(("k_icp", "k_submap", "k_rf"))}
        ctx.profile_enable(False)
        return k

    def fitness(r, best):
        f = r.reshape(-1, 2)["fitness"][np.arange(len(best)), best]
        return {"median": float(np.median(f)), "max": float(f.max()), "above_1.5": int((f > 1.5).sum())}

    for W, n in [(int(w.split(":")[0]), min(M, int(w.split(":")[1]))) for w in args.window_matches.split(",")]:
        half = W // 2
        m_map = pairs[:n].copy()
        m_map["match_idx"] = np.arange(n)
        map_offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(W)
        entry_frame = np.zeros(n * W, np.int32)
        entry_pose = np.zeros((n * W, 12), np.float32)
        for i in range(n):
            for k, d in enumerate(range(-half, half + 1)):
                entry_frame[i * W + k] = F0 + (i + d) % M
                entry_pose[i * W + k] = identity if d == 0 else bev_amd.yaw_translate_matrix(
                    float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.3, 0.3)), 0.0, float(rng.uniform(-1, 1)))
        d_cat, d_uni = (torch.zeros(2 * n * R, dtype=torch.uint8, device=dev) for _ in range(2))
        b_cat, b_uni = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
        cat = lambda: ctx.submap_coarse_voxel_registration_device(
            F, d_pn.data_ptr(), pn_stride, d_cnt.data_ptr(), map_offs, entry_frame, entry_pose, m_map, d_cat.data_ptr(),
            b_cat.data_ptr(), args.pn_leaf, args.radius)
        uni = lambda: ctx.submap_top_part_coarse_registration_device(
            F, d_ord.data_ptr(), None, d_pn.data_ptr(), pn_stride, d_cnt.data_ptr(), map_offs, entry_frame, entry_pose, m_map,
            d_uni.data_ptr(), b_uni.data_ptr(), args.pn_leaf, args.radius)
        fenced(cat)
        fenced(uni)
        t_cat, t_uni = [], []
        for _ in range(args.rounds):
            t_cat.append(fenced(cat))
            t_uni.append(fenced(uni))
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
            "concatenation_fitness": fitness(r_cat, best_cat), "union_fitness": fitness(r_uni, best_uni),
        }
        print(f"window {W}: {json.dumps(out['windows'][str(W)])}", file=sys.stderr, flush=True)
    out["device"] = torch.cuda.get_device_name(0)
    out["host"] = socket.gethostname()
    ctx.close()
    line = json.dumps(out)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
