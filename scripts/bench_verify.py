"""Verification of registered matches (bev_verify_registration_device_resident, bev_submap_verify_registration_device_resident;
DESIGN.md §6aa) beside the registration call whose results it judges.

    python scripts/bench_verify.py [--frames 1000] [--moved 500] [--sub-batch 500] [--rounds 3]
                                   [--window-matches 5:100,21:40] [--map-leaf 0.2] [--out profiles/verify_bench.json]

Frames, moved copies and matches are benchlib's (bench_fine_icp.py's moved-copy pairs on the d_ordered layout).  The yardstick
is bev_fine_registration_device_resident under the whole tool's settings, whose output is the verify call's input; --rounds
alternations of [fine, verify] in one process, every run fenced; every verify run must equal the first byte for byte.  Then one
profiled verify step: per-kernel ms of k_fine_voxel, k_fine_grid, k_verify_move and k_verify_count (both directions are one
launch: the direction is a grid dimension).  The same against maps of W sweeps thinned at --map-leaf, beside
bev_submap_voxel_registration_device_resident.  What the counts say of the matches goes along: the shares at 0.2 m.  One JSON
line."""
import argparse
import json
import statistics
import sys

import numpy as np

import benchlib as bl

KERNELS = ("k_fine_voxel", "k_fine_grid", "k_submap_target", "k_submap_vox_move", "k_submap_vox_keys", "k_submap_vox_tile",
           "k_submap_vox_global", "k_submap_vox_finish", "k_verify_move", "k_verify_count")
TH = (0.1, 0.2, 0.5, 1.0)


def compare(ctx, register, verify, read, rounds):
    """`rounds` alternations behind one unrecorded run of each; the record of the pair"""
    bl.fenced(ctx, register)
    bl.fenced(ctx, verify)
    first = read()
    t_reg, t_ver = [], []
    for _ in range(rounds):
        t_reg.append(bl.fenced(ctx, register))
        t_ver.append(bl.fenced(ctx, verify))
        if read().tobytes() != first.tobytes():
            raise SystemExit("a verify run differs from the first")
    kernels = bl.kernel_ms(ctx, verify, names=KERNELS)
    v = first
    fwd = v["query_within"][:, 1] / np.maximum(v["n_query"], 1)
    rev = v["target_within"][:, 1] / np.maximum(v["n_target"], 1)
    return {"matches": len(v), "register_ms": [t * 1e3 for t in t_reg], "verify_ms": [t * 1e3 for t in t_ver],
            "register_median_ms": statistics.median(t_reg) * 1e3, "verify_median_ms": statistics.median(t_ver) * 1e3,
            "verify_over_register": statistics.median(t_ver) / statistics.median(t_reg), "verify_runs_byte_equal": True,
            "kernels_ms_per_step": kernels, "n_query_mean": float(v["n_query"].mean()), "n_target_mean": float(v["n_target"].mean()),
            "forward_share_at_0.2": {"median": float(np.median(fwd)), "min": float(fwd.min())},
            "reverse_share_at_0.2": {"median": float(np.median(rev)), "min": float(rev.min())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-leaf", type=float, default=0.2)
    bl.std_args(ap, frames=1000, moved=500, sub_batch=500, rounds=3, window_matches="5:100,21:40", out="verify_bench.json")
    args = ap.parse_args()
    import torch

    import bev_amd

    w = bl.registration_world(args)
    ctx, dev = w.ctx, w.dev
    pairs = bl.moved_copy_pairs(w)
    R, V = bev_amd.ICP_RESULT_DTYPE.itemsize, bev_amd.VERIFY_RESULT_DTYPE.itemsize
    whole, prm = bev_amd.icp_whole_defaults(), bev_amd.verify_params(TH)
    d_res = torch.zeros(len(pairs) * R, dtype=torch.uint8, device=dev)
    d_ver = torch.zeros(len(pairs) * V, dtype=torch.uint8, device=dev)

    def read(n):
        return d_ver[: n * V].cpu().numpy().view(bev_amd.VERIFY_RESULT_DTYPE).copy()

    out = {"metric": "verify_over_register", "sensor": "HDL_64E", "frames": w.F, "rounds": args.rounds, "settings": "whole",
           "thresholds": list(TH), "map_leaf": args.map_leaf, "windows": {}}
    out["pairs"] = compare(
        ctx, lambda: ctx.fine_registration_device(w.F, w.d_ord.data_ptr(), None, pairs, d_res.data_ptr(), params=whole),
        lambda: ctx.verify_registration_device(w.F, w.d_ord.data_ptr(), None, pairs, d_res.data_ptr(), d_ver.data_ptr(), prm),
        lambda: read(len(pairs)), args.rounds)
    print(f"pairs: {json.dumps(out['pairs'])}", file=sys.stderr, flush=True)
    for W, n in bl.parse_window_matches(args.window_matches, w.M):
        m = bl.map_matches(pairs, n)
        maps = bl.cyclic_windows(w.rng, w.F0, w.M, n, W)
        out["windows"][str(W)] = compare(
            ctx, lambda: ctx.submap_voxel_registration_device(w.F, w.d_ord.data_ptr(), None, *maps, m, d_res.data_ptr(), args.map_leaf,
                                                              params=whole),
            lambda: ctx.submap_verify_registration_device(w.F, w.d_ord.data_ptr(), None, *maps, m, d_res.data_ptr(), d_ver.data_ptr(),
                                                          args.map_leaf, prm),
            lambda: read(n), args.rounds)
        print(f"window {W}: {json.dumps(out['windows'][str(W)])}", file=sys.stderr, flush=True)
    ctx.close()
    bl.emit(out, args)


if __name__ == "__main__":
    main()
