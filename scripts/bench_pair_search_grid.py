"""Pair registration with search grids sized to the cloud (bev_set_pair_search_grid) beside the same calls at
D = 0, the fixed grids of 128 x 128 (fine) and 64 x 64 (coarse) cells at most, on the same matches, in one process.

    python scripts/bench_pair_search_grid.py [--frames 1000] [--moved 500] [--matches 500] [--rounds 3] [--dims 256,512,1024]
                                             [--out profiles/pair_search_grid_bench.json]

Frames, moved copies and matches (the first --matches of them) are benchlib's, at bench_submap_search_grid.py's scale: the
marked clouds and the front end's PointNormal rows, frame i against its moved copy under the tools' yaw guess.  Fine: bev_fine_registration_device_resident under the whole tool's settings (the yaw guess) and under the
top-part settings (from the coarse stage's own table); coarse: bev_coarse_registration_device_resident under the coarse
defaults.  The yardstick is the D = 0 call of the same build, never an absolute figure.  Per workload: one warm-up of each call,
then for every D of [the stage's fixed cap through the new path, --dims] --rounds alternations of [D = 0 call, D call], each
fenced (launch, bev_synchronize); the D call's results are compared byte for byte with the D = 0 call's BEFORE any of its times
is recorded (a difference ends the run with status 1); then one profiled step of each: the ICP kernel's time over the sum of the
results' iteration counts, the build's time (D > 0: the point counts and the six launches of bev_submap_grid.h; D = 0:
k_fine_grid or k_icp_grid), and from the hook max(nx, ny) and the largest count of one cell over the matches' targets.  One
JSON line, rewritten after every run, so that a run that is cut short leaves what it measured."""
import argparse
import statistics
import sys

import numpy as np

import benchlib as bl

GRID_KERNELS = ("k_pairgrid_desc", "k_subgrid_bounds", "k_subgrid_header", "k_subgrid_count", "k_subgrid_sums", "k_subgrid_scan",
                "k_subgrid_scatter")
OLD_BUILD = {"fine": ("k_fine_grid",), "coarse": ("k_icp_grid",)}
ICP_KERNELS = {"fine": ("k_fine_icp", "k_fine_icp_wide"), "coarse": ("k_icp", "k_icp_wide")}
FIXED_CAP = {"fine": 128, "coarse": 64}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matches", type=int, default=500)
    ap.add_argument("--dims", default="256,512,1024", help="the caps beside the stage's fixed one")
    ap.add_argument("--workloads", default="coarse,whole,top")
    bl.std_args(ap, frames=1000, moved=500, sub_batch=500, rounds=3, out="pair_search_grid_bench.json")
    args = ap.parse_args()
    import torch

    import bev_amd

    w = bl.registration_world(args)
    ctx, d_ord, F, dev = w.ctx, w.d_ord, w.F, w.dev
    stride, d_pn, d_cnt = bl.front_end(w)
    n = min(w.M, args.matches)
    pairs = bl.moved_copy_pairs(w, n)
    R = bev_amd.ICP_RESULT_DTYPE.itemsize
    whole = bev_amd.icp_whole_defaults()
    out = {"metric": "pair_search_grid_time_over_fixed_grid", "sensor": "HDL_64E", "frames": F, "matches": n, "rounds": args.rounds,
           "settings": {"whole": "whole tool, yaw guess", "top": "top-part settings, guesses from the coarse table",
                        "coarse": "coarse defaults"},
           "every_run_byte_equal_to_its_fixed_grid_partner": True, "equal_pairs": 0, "runs": []}

    fenced = lambda step: bl.fenced(ctx, step, log=False)
    profiled = lambda step: bl.kernel_ms(ctx, step)

    def grids(coarse):
        g = ctx.debug_pair_grid(coarse, 0, n)
        return {"targets": n, "max_dim": int(g[:, :2].max()), "largest_cell": int(g[:, 3].max()), "searchable_mean": float(g[:, 2].mean())}

    # the top-part settings start from the coarse stage's table: the D = 0 coarse call's, made once
    d_table = torch.zeros(2 * n * R, dtype=torch.uint8, device=dev)
    b_table = torch.zeros(n, dtype=torch.int32, device=dev)
    ctx.set_pair_search_grid(0, 0)
    ctx.coarse_registration_device(F, d_pn.data_ptr(), stride, d_cnt.data_ptr(), pairs, d_table.data_ptr(), b_table.data_ptr())
    ctx.synchronize()
    for work in args.workloads.split(","):
        coarse = work == "coarse"
        stage = "coarse" if coarse else "fine"
        per = 2 if coarse else 1
        d_old, d_new = (torch.zeros(per * n * R, dtype=torch.uint8, device=dev) for _ in range(2))
        b_old, b_new = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))

        def call(D, d_res, d_best):
            ctx.set_pair_search_grid(0 if coarse else D, D if coarse else 0)
            if coarse:
                ctx.coarse_registration_device(F, d_pn.data_ptr(), stride, d_cnt.data_ptr(), pairs, d_res.data_ptr(), d_best.data_ptr())
            elif work == "whole":
                ctx.fine_registration_device(F, d_ord.data_ptr(), None, pairs, d_res.data_ptr(), params=whole)
            else:
                ctx.fine_registration_device(F, d_ord.data_ptr(), None, pairs, d_res.data_ptr(), d_table.data_ptr(), b_table.data_ptr())

        old = lambda: call(0, d_old, b_old)
        fenced(old)
        k_old = profiled(old)
        g_old = grids(int(coarse))
        ref = (d_old.cpu().numpy().tobytes(), b_old.cpu().numpy().tobytes())
        its = int(np.frombuffer(ref[0], bev_amd.ICP_RESULT_DTYPE)["iterations"].sum())
        for D in [FIXED_CAP[stage]] + [int(d) for d in args.dims.split(",")]:
            new = lambda: call(D, d_new, b_new)
            d_new.zero_()
            b_new.zero_()
            fenced(new)                                                  # the warm-up: its results are compared first
            if (d_new.cpu().numpy().tobytes(), b_new.cpu().numpy().tobytes()) != ref:
                print(f"{work} D {D}: the results differ from the D = 0 call's", file=sys.stderr)
                sys.exit(1)
            t_old, t_new = [], []
            for _ in range(args.rounds):
                t_old.append(fenced(old))
                d_new.zero_()
                t_new.append(fenced(new))
                if (d_new.cpu().numpy().tobytes(), d_old.cpu().numpy().tobytes()) != (ref[0], ref[0]):
                    print(f"{work} D {D}: a timed run's results differ from the D = 0 call's", file=sys.stderr)
                    sys.exit(1)
                out["equal_pairs"] += 1
            k_new = profiled(new)
            g_new = grids(int(coarse))
            med_old, med_new = statistics.median(t_old), statistics.median(t_new)
            icp_old = sum(k_old.get(k, 0.0) for k in ICP_KERNELS[stage])
            icp_new = sum(k_new.get(k, 0.0) for k in ICP_KERNELS[stage])
            run = {"workload": work, "stage": stage, "matches": n, "D": D, "byte_equal": True,
                   "fixed_ms": [t * 1e3 for t in t_old], "wide_ms": [t * 1e3 for t in t_new],
                   "fixed_median_ms": med_old * 1e3, "wide_median_ms": med_new * 1e3, "wide_over_fixed": med_new / med_old,
                   "iterations": its,
                   "fixed_icp_us_per_iteration_problem": icp_old * 1e3 / max(its, 1),
                   "wide_icp_us_per_iteration_problem": icp_new * 1e3 / max(its, 1),
                   "fixed_build_ms": sum(k_old.get(k, 0.0) for k in OLD_BUILD[stage]),
                   "wide_build_ms": sum(k_new.get(k, 0.0) for k in GRID_KERNELS),
                   "fixed_kernels_ms": k_old, "wide_kernels_ms": k_new, "fixed_grid": g_old, "wide_grid": g_new}
            out["runs"].append(run)
            bl.emit(out, args, final=False)
            print(f"{work} D {D}: fixed {med_old * 1e3:.2f} ms, wide {med_new * 1e3:.2f} ms, ratio {med_new / med_old:.3f}; icp us/it "
                  f"{run['fixed_icp_us_per_iteration_problem']:.2f} -> {run['wide_icp_us_per_iteration_problem']:.2f}; build "
                  f"{run['fixed_build_ms']:.3f} -> {run['wide_build_ms']:.3f} ms; grids {g_old} -> {g_new}", file=sys.stderr, flush=True)
    ctx.set_pair_search_grid(0, 0)
    ctx.close()
    bl.emit(out, args)


if __name__ == "__main__":
    main()
