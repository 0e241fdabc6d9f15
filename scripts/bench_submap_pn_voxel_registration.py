"""Scan-to-map coarse ICP against maps thinned over their union (bev_submap_coarse_voxel_registration_device_resident with
pn_leaf > 0) beside the same call with pn_leaf = 0 (bev_submap_coarse_registration_device_resident's code) on the
same matches, in one process.

    python scripts/bench_submap_pn_voxel_registration.py [--frames 1000] [--moved 500] [--rounds 3] [--pn-leaf 0.2]
                                                         [--window-matches 1:500,5:100,21:40]
                                                         [--out profiles/submap_pn_voxel_registration_bench.json]

Frames, moved copies, matches and windows are scripts/bench_submap_coarse_registration.py's: bench.py's synthetic HDL_64E
sweeps through bev_process_device_resident and the registration front end (leaf 0.2, radius 2), frame i against a map of the
moved copies i - W // 2 .. i + W // 2 (cyclic), the centre under the identity, the others under a seeded planar matrix within
+-1 degree and +-0.3 m.  The yardstick is the pn_leaf = 0 call, never an absolute figure.  Per window: one warm-up of each
call, --rounds alternations of [pn_leaf = 0 call, thinned call], each fenced (launch, bev_synchronize): the medians and ranges,
matches/s, the ratio; the maps' rows before and after thinning (bev_submap_pn_cloud_device_resident's counts); then one
profiled step of each: per-kernel ms, the results' iteration counts, the ICP kernel's time over the sum of those counts; the
states, the choices and the fitness on both sides.  One JSON line."""
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
    ap.add_argument("--out", default=str(REPO / "profiles" / "submap_pn_voxel_registration_bench.json"))
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
    del d_ord
    counts = d_cnt.cpu().numpy()
    pn_stride = stride

    pairs = np.zeros(M, bev_amd.MATCH_DTYPE)
    pairs["query_idx"] = np.arange(M)
    pairs["match_idx"] = F0 + np.arange(M)
    pairs["angle_guess"] = yaw + rng.uniform(-2, 2, M).astype(np.float32)
    R = bev_amd.ICP_RESULT_DTYPE.itemsize
    identity = np.eye(3, 4, dtype=np.float32).reshape(12)
    out = {"metric": "submap_pn_voxel_registration_matches_per_s", "sensor": "HDL_64E", "frames": F, "stride": int(pn_stride),
           "rows_per_frame": {"mean": float(counts.mean()), "max": int(counts.max())}, "rounds": args.rounds,
           "pn_leaf": args.pn_leaf, "radius": args.radius, "settings": "coarse defaults", "windows": {}}

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
        k = {s["name"]: s["total_ms"] for s in ctx.profile_get() if s["name"].startswith(("k_icp", "k_submap"))}
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
        d_plain, d_thin = (torch.zeros(2 * n * R, dtype=torch.uint8, device=dev) for _ in range(2))
        b_plain, b_thin = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
        call = lambda d_res, d_best, leaf: ctx.submap_coarse_voxel_registration_device(
            F, d_pn.data_ptr(), pn_stride, d_cnt.data_ptr(), map_offs, entry_frame, entry_pose, m_map, d_res.data_ptr(),
            d_best.data_ptr(), leaf, args.radius)
        plain = lambda: call(d_plain, b_plain, 0.0)
        thin = lambda: call(d_thin, b_thin, args.pn_leaf)
        fenced(plain)
        fenced(thin)
        t_plain, t_thin = [], []
        for _ in range(args.rounds):
            t_plain.append(fenced(plain))
            t_thin.append(fenced(thin))
        k_plain, k_thin = profiled(plain), profiled(thin)
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
            "plain_fitness": fitness(r_plain, best_plain), "thinned_fitness": fitness(r_thin, best_thin),
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
