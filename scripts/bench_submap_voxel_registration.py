"""Scan-to-map fine ICP against maps thinned by a voxel grid over their union (bev_submap_voxel_registration_device_resident
with map_leaf 0.2) beside the same call with map_leaf 0 — §6k's code path, the yardstick — on the same
matches, in one process.

    python scripts/bench_submap_voxel_registration.py [--frames 1000] [--moved 500] [--rounds 3] [--map-leaf 0.2]
                                                      [--window-matches 1:500,5:100,21:40]
                                                      [--out profiles/submap_voxel_registration_bench.json]

Frames, moved copies, matches, windows and their seeded matrices are scripts/bench_submap_registration.py's (§6k's protocol):
bench.py's default workload plus a moved copy of each of the first --moved frames, run once through
bev_process_device_resident; for a window of W entries the map of match i holds the copies i - W // 2 .. i + W // 2 (cyclic),
the centre under the identity, the others under a seeded planar matrix within +-1 degree and +-0.3 m.  Per window: one
warm-up and --rounds alternations of [map_leaf 0, map_leaf --map-leaf], each fenced (launch, bev_synchronize): the medians
with min and max, the ratio; then one profiled step of each: per-kernel ms (move, keys, the sort's stages together,
centroids + grid, ICP), mean iterations, the ICP kernel's time over the sum of the iteration counts, matches with fitness
<= 1.5 on each side and how many matches differ in that verdict; and, from bev_submap_voxel_cloud_device_resident on the
first --count-maps maps, the points per map before and after thinning.  One JSON line."""
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
    ap.add_argument("--map-leaf", type=float, default=0.2)
    ap.add_argument("--count-maps", type=int, default=8, help="maps whose point counts the cloud call reports")
    ap.add_argument("--out", default=str(REPO / "profiles" / "submap_voxel_registration_bench.json"))
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

    pairs = np.zeros(M, bev_amd.MATCH_DTYPE)
    pairs["query_idx"] = np.arange(M)
    pairs["match_idx"] = F0 + np.arange(M)
    pairs["angle_guess"] = yaw + rng.uniform(-2, 2, M).astype(np.float32)
    R = bev_amd.ICP_RESULT_DTYPE.itemsize
    prm = bev_amd.icp_whole_defaults()
    identity = np.eye(3, 4, dtype=np.float32).reshape(12)
    out = {"metric": "submap_voxel_registration_matches_per_s", "sensor": "HDL_64E", "frames": F, "records_per_frame": S,
           "rounds": args.rounds, "settings": "whole", "map_leaf": args.map_leaf, "windows": {}}
    spread = lambda ts: {"median": statistics.median(ts) * 1e3, "min": min(ts) * 1e3, "max": max(ts) * 1e3}

    def fenced(step):
        t = time.perf_counter()
        step()
        ctx.synchronize()
        t = time.perf_counter() - t
        print(f"  step {t * 1e3:.1f} ms", file=sys.stderr, flush=True)
        return t

    def profiled(step, prefix):
        ctx.profile_reset()
        ctx.profile_enable(True)
        step()
        ctx.synchronize()
        k = {s["name"]: s["total_ms"] for s in ctx.profile_get() if s["name"].startswith(prefix)}
        ctx.profile_enable(False)
        return k

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
        d_plain = torch.zeros(n * R, dtype=torch.uint8, device=dev)
        d_thin = torch.zeros(n * R, dtype=torch.uint8, device=dev)
        call = lambda d, leaf: ctx.submap_voxel_registration_device(F, d_ord.data_ptr(), None, map_offs, entry_frame, entry_pose,
                                                                    m_map, d.data_ptr(), leaf, params=prm)
        plain = lambda: call(d_plain, 0.0)
        thin = lambda: call(d_thin, args.map_leaf)
        fenced(plain)
        fenced(thin)
        t_plain, t_thin = [], []
        for _ in range(args.rounds):
            t_plain.append(fenced(plain))
            t_thin.append(fenced(thin))
        k_plain, k_thin = profiled(plain, ("k_fine", "k_submap")), profiled(thin, ("k_fine", "k_submap"))
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
    out["device"] = torch.cuda.get_device_name(0)
    out["host"] = socket.gethostname()
    ctx.close()
    line = json.dumps(out)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
