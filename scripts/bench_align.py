"""The translation guess of retrieved pairs (bev_align_grid_device_resident, bev_align_hits_device_resident) on
device-resident frames.

    python scripts/bench_align.py [--frames 1000] [--hits 1000] [--steps 10] [--warmup 2] [--rounds 5]

One JSON line, written to profiles/align_bench.json as well.  The frames are benchlib's marked HDL_64E sweeps, the parameters
the defaults (128 x 128 cells of 0.5 m, shifts of +-16 cells, yaw +-1 step of 2 degrees, label 0 skipped).  Hit h is frame h
against frame h + 1 (another sweep) from a seeded yaw guess: what a hit costs does not depend on whether it is a true one.
  grids   one call over all frames by benchlib.timed, and its kernels' times from bev_profile_get;
  hits    one call over all hits: benchlib.timed and the kernels' times; the last hit is checked against the sequential checker
          of the tests where that has been built;
  against_place_match   alternated --rounds times with bev_place_match_device_resident, frames x frames at top_k 1: the step
          that makes the hit list;
  against_fine          alternated with bev_fine_registration_device_resident under the whole tool's settings on the same hits
          from the table just made: the step the table feeds; stage_share_of_fine is the medians' ratio."""
import argparse
import statistics
import sys

import numpy as np

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=1000)
    bl.std_args(ap, frames=1000, steps=10, warmup=2, distinct=8, rounds=5, out="align_bench.json")
    args = ap.parse_args()
    import torch

    import bev_amd

    dev = torch.device("cuda:0")
    F, H = args.frames, args.hits
    p = bev_amd.params_for_sensor("HDL_64E")
    S = p.slots
    prm = bev_amd.align_params()
    cells = bev_amd.align_grid_bytes(prm)
    R, D = bev_amd.ICP_RESULT_DTYPE.itemsize, bev_amd.ALIGN_DETAIL_DTYPE.itemsize
    result = {"metric": "align", "frames": F, "hits": H, "steps": args.steps, "warmup": args.warmup, "records_per_frame": S,
              "grid": prm.grid, "cell": prm.cell, "max_shift": prm.max_shift, "yaw_steps": prm.yaw_steps, "yaw_step": prm.yaw_step,
              "skip_label0": True, "byte_shift_form": "alignbyte"}

    t = bl.tiled_marked_frames(p, args.distinct, F, dev)
    ctx = bev_amd.BevContext(p, device=0, max_batch=8, max_points=S)
    rng = np.random.default_rng(2027)
    hits = np.zeros(H, bev_amd.MATCH_DTYPE)
    hits["query_idx"], hits["match_idx"] = np.arange(H) % F, (np.arange(H) + 1) % F
    hits["angle_guess"] = rng.uniform(-180.0, 180.0, H).astype(np.float32)
    d_grids = torch.empty(F * cells, dtype=torch.uint8, device=dev)
    d_energy = torch.empty(F * 4, dtype=torch.uint8, device=dev)
    d_tab = torch.empty(2 * H * R, dtype=torch.uint8, device=dev)
    d_best = torch.empty(4 * H, dtype=torch.uint8, device=dev)
    d_det = torch.empty(2 * H * D, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    grid_call = lambda: ctx.align_grid_device(F, t.d_clouds.data_ptr(), t.offs, d_grids.data_ptr(), d_energy.data_ptr(), prm)
    hits_call = lambda: ctx.align_hits_device(F, t.d_clouds.data_ptr(), t.offs, F, d_grids.data_ptr(), d_energy.data_ptr(), hits,
                                              d_tab.data_ptr(), d_best.data_ptr(), d_det.data_ptr(), prm)
    fenced, unfenced = bl.timed(ctx, grid_call, args.steps, args.warmup)
    result["grids"] = {"fenced_median_ms": fenced * 1e3, "fenced_frames_per_s": F / fenced, "unfenced_mean_ms": unfenced * 1e3,
                       "kernels_ms_per_step": bl.kernel_ms(ctx, grid_call, names=("k_align_grid", "k_align_finish"))}
    fenced, unfenced = bl.timed(ctx, hits_call, args.steps, args.warmup)
    kernels = bl.kernel_ms(ctx, hits_call, names=("k_align_hit", "k_align_pick"))
    result["hits_call"] = {"fenced_median_ms": fenced * 1e3, "fenced_hits_per_s": H / fenced, "unfenced_mean_ms": unfenced * 1e3,
                           "unfenced_hits_per_s": H / unfenced, "kernels_ms_per_step": kernels}
    total = sum(k["ms_per_step"] for k in kernels.values())
    result["hits_call"]["kernel_shares"] = {n: k["ms_per_step"] / total for n, k in kernels.items()} if total > 0 else {}
    checked = False
    try:  # the numbers are of kernels that compute the right thing (the checker is the tests': built by them)
        import align_lib
        h = hits[H - 1]
        cl = lambda f: t.clouds[f % len(t.clouds)]
        want = align_lib.hit(cl(h["query_idx"]), align_lib.grid([(cl(h["match_idx"]), None)], prm, p.lidar_to_ground), h["angle_guess"],
                             prm, p.lidar_to_ground)
        assert d_tab[2 * (H - 1) * R:].cpu().numpy().tobytes() == want[0].tobytes()
        assert d_det[2 * (H - 1) * D:].cpu().numpy().tobytes() == want[2].tobytes()
        assert int(d_best[4 * (H - 1):].cpu().numpy().view(np.int32)[0]) == want[1]
        checked = True
    except (ImportError, OSError, RuntimeError) as e:
        print(f"  hits not checked: {e}", file=sys.stderr)
    result["hits_call"]["checked_against_the_checker"] = checked

    pprm = bev_amd.place_params()
    HB = bev_amd.place_desc_handle_bytes(pprm)
    d_units = torch.empty(F * HB, dtype=torch.uint8, device=dev)
    d_phits = torch.empty(F * bev_amd.PLACE_HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.place_descriptor_device(F, t.d_clouds.data_ptr(), t.offs, 0, d_units.data_ptr(), pprm)
    match_call = lambda: ctx.place_match_device(F, d_units.data_ptr(), F, d_units.data_ptr(), d_phits.data_ptr(), 1, None, pprm)
    t_align, t_match = bl.alternate(ctx, hits_call, match_call, args.rounds, log=False)
    result["against_place_match"] = {"queries": F, "database": F, "alternated_hits_ms": [x * 1e3 for x in t_align],
                                     "alternated_place_match_ms": [x * 1e3 for x in t_match],
                                     "alternated_hits_median_ms": statistics.median(t_align) * 1e3,
                                     "alternated_place_match_median_ms": statistics.median(t_match) * 1e3}
    del d_units, d_phits

    d_fine = torch.empty(H * R, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    fine_call = lambda: ctx.fine_registration_device(F, t.d_clouds.data_ptr(), t.offs, hits, d_fine.data_ptr(), d_tab.data_ptr(),
                                                     d_best.data_ptr(), 0.2, bev_amd.icp_whole_defaults())
    t_align, t_fine = bl.alternate(ctx, hits_call, fine_call, args.rounds, log=False)
    ma, mf = statistics.median(t_align), statistics.median(t_fine)
    result["against_fine"] = {"settings": "whole", "alternated_hits_ms": [x * 1e3 for x in t_align],
                              "alternated_fine_ms": [x * 1e3 for x in t_fine], "alternated_hits_median_ms": ma * 1e3,
                              "alternated_fine_median_ms": mf * 1e3, "stage_share_of_fine": ma / mf}
    ctx.close()
    bl.emit(result, args)


if __name__ == "__main__":
    main()
