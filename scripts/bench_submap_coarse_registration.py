"""Scan-to-map coarse ICP (bev_submap_coarse_registration_device_resident) beside the pair call
(bev_coarse_registration_device_resident) on the same matches, in one process.

    python scripts/bench_submap_coarse_registration.py [--frames 1000] [--moved 500] [--rounds 3]
                                                       [--window-matches 1:500,5:100,21:40]
                                                       [--out profiles/submap_coarse_registration_bench.json]

The frames are bench.py's default workload (synthetic HDL_64E sweeps, 98 % of the slots, 5,000 duplicates) plus a moved copy
(seeded yaw within +-20 degrees, translation within +-1.5 m, by bev_transform_cloud) of each of the first --moved frames, run
once through bev_process_device_resident and then through the registration front end (leaf 0.2, radius 2): both calls read its
PointNormal clouds.  The matches are bench_icp.py's moved-copy pairs (frame i against its copy, the yaw within +-2 degrees as
the guess) under the coarse defaults.  For a window of W entries the map of match i holds the copies i - W // 2 .. i + W // 2
(cyclic), the centre under the identity, the others under a seeded planar matrix within +-1 degree and +-0.3 m; W = 1 is the
pair call's problem, and the yardstick: the two compute the same thing there.  A window of W runs on the first n matches of
--window-matches W:n.  Per window, --rounds alternations of [pair call, submap call], each fenced (launch, bev_synchronize):
the medians, matches/s, the ratio; then one profiled step of each: per-kernel ms, the results' iteration counts, and the ICP
kernels' time over the sum of those counts (every problem is one workgroup, and a launch's workgroups run side by side: a
kernel's time over the MEAN count is the time of one iteration of the launch).  One JSON line."""
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
    ap.add_argument("--out", default=str(REPO / "profiles" / "submap_coarse_registration_bench.json"))
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

    pairs = np.zeros(M, bev_amd.MATCH_DTYPE)
    pairs["query_idx"] = np.arange(M)
    pairs["match_idx"] = F0 + np.arange(M)
    pairs["angle_guess"] = yaw + rng.uniform(-2, 2, M).astype(np.float32)
    R = bev_amd.ICP_RESULT_DTYPE.itemsize
    identity = np.eye(3, 4, dtype=np.float32).reshape(12)
    out = {"metric": "submap_coarse_registration_matches_per_s", "sensor": "HDL_64E", "frames": F, "stride": int(stride),
           "rows_per_frame": {"mean": float(counts.mean()), "max": int(counts.max())}, "rounds": args.rounds,
           "settings": "coarse defaults", "windows": {}}

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
        m_pair = pairs[:n].copy()
        m_map = m_pair.copy()
        m_map["match_idx"] = np.arange(n)
        map_offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(W)
        entry_frame = np.zeros(n * W, np.int32)
        entry_pose = np.zeros((n * W, 12), np.float32)
        for i in range(n):
            for k, d in enumerate(range(-half, half + 1)):
                entry_frame[i * W + k] = F0 + (i + d) % M
                entry_pose[i * W + k] = identity if d == 0 else bev_amd.yaw_translate_matrix(
                    float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.3, 0.3)), 0.0, float(rng.uniform(-1, 1)))
        d_pair, d_map = (torch.zeros(2 * n * R, dtype=torch.uint8, device=dev) for _ in range(2))
        b_pair, b_map = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
        pair = lambda: ctx.coarse_registration_device(F, d_pn.data_ptr(), stride, d_cnt.data_ptr(), m_pair, d_pair.data_ptr(),
                                                      b_pair.data_ptr())
        submap = lambda: ctx.submap_coarse_registration_device(F, d_pn.data_ptr(), stride, d_cnt.data_ptr(), map_offs, entry_frame,
                                                               entry_pose, m_map, d_map.data_ptr(), b_map.data_ptr())
        fenced(pair)
        fenced(submap)
        t_pair, t_map = [], []
        for _ in range(args.rounds):
            t_pair.append(fenced(pair))
            t_map.append(fenced(submap))
        k_pair, k_map = profiled(pair, "k_icp"), profiled(submap, ("k_icp", "k_submap"))
        r_pair = d_pair.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE)
        r_map = d_map.cpu().numpy().view(bev_amd.ICP_RESULT_DTYPE)
        it_pair, it_map = int(r_pair["iterations"].sum()), int(r_map["iterations"].sum())
        med_pair, med_map = statistics.median(t_pair), statistics.median(t_map)
        target_rows = np.array([counts[entry_frame[i * W:(i + 1) * W]].sum() for i in range(n)])
        out["windows"][str(W)] = {
            "matches": n, "problems": 2 * n, "entries": int(n * W), "target_rows": {"mean": float(target_rows.mean()), "max": int(target_rows.max())},
            "identical_to_pair_call": bool(W == 1 and r_pair.tobytes() == r_map.tobytes() and
                                           b_pair.cpu().numpy().tobytes() == b_map.cpu().numpy().tobytes()),
            "pair_ms": [t * 1e3 for t in t_pair], "submap_ms": [t * 1e3 for t in t_map],
            "pair_median_ms": med_pair * 1e3, "submap_median_ms": med_map * 1e3, "submap_over_pair": med_map / med_pair,
            "pair_matches_per_s": n / med_pair, "submap_matches_per_s": n / med_map,
            "pair_kernels_ms": k_pair, "submap_kernels_ms": k_map,
            "pair_iterations": {"sum": it_pair, "mean": it_pair / (2 * n)}, "submap_iterations": {"sum": it_map, "mean": it_map / (2 * n)},
            "k_icp_us_per_iteration_problem": k_pair.get("k_icp", 0.0) * 1e3 / max(it_pair, 1),
            "k_submap_coarse_icp_us_per_iteration_problem": k_map.get("k_submap_coarse_icp", 0.0) * 1e3 / max(it_map, 1),
            "submap_states": np.bincount(r_map["state"], minlength=6).tolist(),
            "submap_best": np.bincount(b_map.cpu().numpy(), minlength=2).tolist(),
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
