"""Scan-to-map ICP with search grids sized to the map (bev_set_submap_search_grid) beside the same calls at
D = 0, the fixed grids of 128 x 128 (fine) and 64 x 64 (coarse) cells at most, on the same matches, in one process.

    python scripts/bench_submap_search_grid.py [--frames 1000] [--moved 500] [--rounds 3] [--map-leaf 0.2] [--pn-leaf 0.2]
                                               [--window-matches 1:500,5:100,21:40] [--coarse-window-matches ...]
                                               [--dims 256,512,1024]
                                               [--out profiles/submap_search_grid_bench.json]

Frames, moved copies, matches and windows are benchlib's; the settings are bench_submap_voxel_registration.py's (fine: the
whole tool's settings on the marked clouds) and bench_submap_pn_voxel_registration.py's (coarse: the coarse defaults on the
front end's rows).  The yardstick is the D = 0 call of the same build, never an absolute figure.  Per stage (fine, coarse),
leaf (0 and the thinning leaf) and window: one warm-up of each call, then for every D of [the stage's fixed cap through the new
path, --dims] --rounds alternations of [D = 0 call, D call], each fenced; the D call's results are compared byte for byte with the D = 0
call's BEFORE any of its times is recorded (a difference ends the run with status 1); then one profiled step of each: the ICP
kernel's time over the sum of the results' iteration counts, the build's time (D > 0: the six launches of bev_submap_grid.h;
D = 0: the kernels that hold the one-workgroup build), and from the hook max(nx, ny) and the largest count of one cell over
the maps of the last launch group.  One JSON line, rewritten after every run, so that a run that is cut short leaves what it
measured.  The fine D = 0 call on unthinned maps of 5 and 21 sweeps takes seconds per match list: --window-matches sets the fine
stage's lists, --coarse-window-matches the coarse stage's (default: the same)."""
import argparse
import statistics
import sys

import numpy as np

import benchlib as bl

GRID_KERNELS = ("k_subgrid_bounds", "k_subgrid_header", "k_subgrid_count", "k_subgrid_sums", "k_subgrid_scan", "k_subgrid_scatter")
# D = 0: the kernels whose one workgroup per map builds the grid (with the concatenation or the centroids, which cannot be split off)
OLD_BUILD = {"fine": ("k_submap_target", "k_submap_vox_finish"), "coarse": ("k_submap_pn_target", "k_submap_pn_grid")}
ICP_KERNELS = {"fine": ("k_submap_icp", "k_submap_icp_wide"), "coarse": ("k_submap_coarse_icp", "k_submap_coarse_icp_wide")}
FIXED_CAP = {"fine": 128, "coarse": 64}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coarse-window-matches", default=None, help="the coarse stage's W:n pairs (default: --window-matches)")
    ap.add_argument("--map-leaf", type=float, default=0.2)
    ap.add_argument("--pn-leaf", type=float, default=0.2)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--dims", default="256,512,1024", help="the caps beside the stage's fixed one")
    ap.add_argument("--stages", default="fine,coarse")
    bl.std_args(ap, frames=1000, moved=500, window_matches="1:500,5:100,21:40", sub_batch=500, rounds=3,
                out="submap_search_grid_bench.json")
    args = ap.parse_args()
    import torch

    import bev_amd

    w = bl.registration_world(args)
    ctx, d_ord, F, M, dev = w.ctx, w.d_ord, w.F, w.M, w.dev
    stride, d_pn, d_cnt = bl.front_end(w)
    pairs = bl.moved_copy_pairs(w)
    R = bev_amd.ICP_RESULT_DTYPE.itemsize
    whole = bev_amd.icp_whole_defaults()
    out = {"metric": "submap_search_grid_time_over_fixed_grid", "sensor": "HDL_64E", "frames": F, "rounds": args.rounds,
           "map_leaf": args.map_leaf, "pn_leaf": args.pn_leaf, "settings": {"fine": "whole tool", "coarse": "coarse defaults"},
           "every_run_byte_equal_to_its_fixed_grid_partner": True, "runs": []}

    fenced = lambda step: bl.fenced(ctx, step, log=False)
    profiled = lambda step: bl.kernel_ms(ctx, step, ("k_submap", "k_subgrid"))

    def grids(coarse, n_maps):
        for n in (n_maps, 1):
            try:
                g = ctx.debug_submap_grid(coarse, 0, n)
                return {"maps": n, "max_dim": int(g[:, :2].max()), "largest_cell": int(g[:, 3].max()), "searchable_mean": float(g[:, 2].mean())}
            except bev_amd.BevError:
                continue
        return None

    lists = [(stage, W, n) for stage in args.stages.split(",") for W, n in bl.parse_window_matches(
        args.coarse_window_matches if stage == "coarse" and args.coarse_window_matches else args.window_matches, M)]
    for stage, W, n in sorted(lists, key=lambda l: l[1]):
        m_map = bl.map_matches(pairs, n)
        map_offs, entry_frame, entry_pose = bl.cyclic_windows(w.rng, w.F0, M, n, W)
        coarse = stage == "coarse"
        for leaf in (0.0, args.pn_leaf if coarse else args.map_leaf):
            per = 2 if coarse else 1
            d_old, d_new = (torch.zeros(per * n * R, dtype=torch.uint8, device=dev) for _ in range(2))
            b_old, b_new = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))

            def call(D, d_res, d_best):
                ctx.set_submap_search_grid(0 if coarse else D, D if coarse else 0)
                if coarse:
                    ctx.submap_coarse_voxel_registration_device(F, d_pn.data_ptr(), stride, d_cnt.data_ptr(), map_offs, entry_frame,
                                                                entry_pose, m_map, d_res.data_ptr(), d_best.data_ptr(), leaf, args.radius)
                else:
                    ctx.submap_voxel_registration_device(F, d_ord.data_ptr(), None, map_offs, entry_frame, entry_pose, m_map,
                                                         d_res.data_ptr(), leaf, params=whole)

            old = lambda: call(0, d_old, b_old)
            fenced(old)
            k_old = profiled(old)
            g_old = grids(int(coarse), n)
            ref = (d_old.cpu().numpy().tobytes(), b_old.cpu().numpy().tobytes())
            its = int(np.frombuffer(ref[0], bev_amd.ICP_RESULT_DTYPE)["iterations"].sum())
            for D in [FIXED_CAP[stage]] + [int(d) for d in args.dims.split(",")]:
                new = lambda: call(D, d_new, b_new)
                d_new.zero_()
                b_new.zero_()
                fenced(new)                                                  # the warm-up: its results are compared first
                same = (d_new.cpu().numpy().tobytes(), b_new.cpu().numpy().tobytes()) == ref
                if not same:
                    print(f"{stage} W {W} leaf {leaf} D {D}: the results differ from the D = 0 call's", file=sys.stderr)
                    sys.exit(1)
                t_old, t_new = bl.alternate(ctx, old, new, args.rounds, warm=False, log=False)
                k_new = profiled(new)
                g_new = grids(int(coarse), n)
                assert (d_new.cpu().numpy().tobytes(), b_new.cpu().numpy().tobytes()) == ref
                med_old, med_new = statistics.median(t_old), statistics.median(t_new)
                icp_old = sum(k_old.get(k, 0.0) for k in ICP_KERNELS[stage])
                icp_new = sum(k_new.get(k, 0.0) for k in ICP_KERNELS[stage])
                run = {"stage": stage, "window": W, "matches": n, "leaf": leaf, "D": D, "byte_equal": True,
                       "fixed_ms": [t * 1e3 for t in t_old], "wide_ms": [t * 1e3 for t in t_new],
                       "fixed_median_ms": med_old * 1e3, "wide_median_ms": med_new * 1e3, "wide_over_fixed": med_new / med_old,
                       "iterations": its,
                       "fixed_icp_us_per_iteration_problem": icp_old * 1e3 / max(its, 1),
                       "wide_icp_us_per_iteration_problem": icp_new * 1e3 / max(its, 1),
                       "fixed_build_kernels_ms": sum(k_old.get(k, 0.0) for k in OLD_BUILD[stage]),
                       "wide_build_ms": sum(k_new.get(k, 0.0) for k in GRID_KERNELS),
                       "fixed_kernels_ms": k_old, "wide_kernels_ms": k_new, "fixed_grid": g_old, "wide_grid": g_new}
                out["runs"].append(run)
                bl.emit(out, args, final=False)
                print(f"{stage} W {W} leaf {leaf} D {D}: fixed {med_old * 1e3:.2f} ms, wide {med_new * 1e3:.2f} ms, ratio "
                      f"{med_new / med_old:.3f}; icp us/it {run['fixed_icp_us_per_iteration_problem']:.2f} -> "
                      f"{run['wide_icp_us_per_iteration_problem']:.2f}; build {run['wide_build_ms']:.3f} ms; grids {g_old} -> {g_new}",
                      file=sys.stderr, flush=True)
    ctx.set_submap_search_grid(0, 0)
    ctx.close()
    bl.emit(out, args)


if __name__ == "__main__":
    main()
