"""Place retrieval (bev_place_descriptor_device_resident, bev_place_match_device_resident) on device-resident
frames.

    python scripts/bench_place_retrieval.py [--frames 1000] [--steps 20] [--warmup 5] [--rounds 5] [--max-square 32768]

One JSON line, written to profiles/place_retrieval_bench.json as well.  The frames are benchlib's marked HDL_64E sweeps, the
parameters the defaults (20 rings, 60 sectors, 80 m, label 0 skipped).
  descriptor   one call over all frames by benchlib.timed, its kernels' times from bev_profile_get, and — the yardstick for a
               raster of the same input — bev_float_bev_device_resident (interval 1.0, no poses) over the same frames,
               the two alternated --rounds times in one process (benchlib.alternate); the last frame's descriptor is checked against the
               sequential checker of the tests where that has been built;
  match        frames x frames at top_k 1, every query against the whole database: benchlib.timed and the kernels' times;
               then squares of twice the side each (the unit records tiled) while a fenced call takes less than a second
               and the side is at most --max-square: every side tried, and the largest that fitted."""
import argparse
import statistics
import sys

import numpy as np

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-square", type=int, default=32768, help="the largest side of a match call that is tried")
    bl.std_args(ap, frames=1000, steps=20, warmup=5, distinct=8, rounds=5, out="place_retrieval_bench.json")
    args = ap.parse_args()
    import torch

    import bev_amd

    dev = torch.device("cuda:0")
    F = args.frames
    p = bev_amd.params_for_sensor("HDL_64E")
    S = p.slots
    prm = bev_amd.place_params()
    cells, HB = bev_amd.place_descriptor_bytes(prm), bev_amd.place_desc_handle_bytes(prm)
    hit = bev_amd.PLACE_HIT_DTYPE.itemsize
    result = {"metric": "place_retrieval", "frames": F, "steps": args.steps, "warmup": args.warmup, "records_per_frame": S,
              "n_rings": prm.n_rings, "n_sectors": prm.n_sectors, "max_range": prm.max_range, "skip_label0": True}

    t = bl.tiled_marked_frames(p, args.distinct, F, dev)
    ctx = bev_amd.BevContext(p, device=0, max_batch=8, max_points=S)
    d_desc = torch.empty(F * cells, dtype=torch.uint8, device=dev)
    d_units = torch.empty(F * HB, dtype=torch.uint8, device=dev)
    M = int(ctx.lib.bev_float_bev_size(1.0))
    d_grid = torch.empty(F * M * M, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    describe = lambda: ctx.place_descriptor_device(F, t.d_clouds.data_ptr(), t.offs, d_desc.data_ptr(), d_units.data_ptr(), prm)
    raster = lambda: ctx.float_bev_device(F, t.d_clouds.data_ptr(), t.offs, d_grid.data_ptr(), 1.0, True)
    fenced, unfenced = bl.timed(ctx, describe, args.steps, args.warmup)
    kernels = bl.kernel_ms(ctx, describe, names=("k_place_splat", "k_place_finish"))
    t_desc, t_float = bl.alternate(ctx, describe, raster, args.rounds, log=False)
    result["descriptor"] = {"fenced_median_ms": fenced * 1e3, "fenced_frames_per_s": F / fenced,
                            "unfenced_mean_ms": unfenced * 1e3, "unfenced_frames_per_s": F / unfenced, "kernels_ms_per_step": kernels,
                            "alternated_ms": [x * 1e3 for x in t_desc], "alternated_float_bev_ms": [x * 1e3 for x in t_float],
                            "alternated_median_ms": statistics.median(t_desc) * 1e3,
                            "alternated_float_bev_median_ms": statistics.median(t_float) * 1e3}
    checked = False
    try:  # the numbers are of kernels that compute the right thing (the checker is the tests': built by them)
        import place_lib
        want = place_lib.descriptor([(t.clouds[(F - 1) % len(t.clouds)], None)], prm, p.lidar_to_ground)
        assert d_desc[(F - 1) * cells:].cpu().numpy().tobytes() == want.tobytes()
        assert d_units[(F - 1) * HB:].cpu().numpy().tobytes() == place_lib.handle(want).tobytes()
        checked = True
    except (ImportError, OSError, RuntimeError) as e:
        print(f"  descriptor not checked: {e}", file=sys.stderr)
    result["descriptor"]["checked_against_the_checker"] = checked
    del d_grid

    def match_call(n, units):
        d_hits = torch.empty(n * hit, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        return d_hits, lambda: ctx.place_match_device(n, units.data_ptr(), n, units.data_ptr(), d_hits.data_ptr(), 1, None, prm)

    d_hits, step = match_call(F, d_units)
    fenced, unfenced = bl.timed(ctx, step, args.steps, args.warmup)
    hits = d_hits.cpu().numpy().view(bev_amd.PLACE_HIT_DTYPE)
    assert (hits["match_idx"] == np.arange(F) % min(F, len(t.clouds))).all() and not hits["shift"].any()  # a frame's first copy
    result["match"] = {"queries": F, "database": F, "top_k": 1, "fenced_median_ms": fenced * 1e3, "fenced_pairs_per_s": F * F / fenced,
                       "unfenced_mean_ms": unfenced * 1e3, "unfenced_pairs_per_s": F * F / unfenced,
                       "kernels_ms_per_step": bl.kernel_ms(ctx, step, names=("k_place_pairs", "k_place_topk"))}
    squares, largest, n = [], None, F
    while n <= args.max_square:
        units = d_units.repeat((n + F - 1) // F)[: n * HB].contiguous()
        d_hits, step = match_call(n, units)
        bl.fenced(ctx, step, log=False)
        ms = statistics.median(bl.fenced(ctx, step, log=False) for _ in range(3)) * 1e3
        squares.append({"side": n, "fenced_median_ms": ms, "pairs_per_s": n * n / (ms * 1e-3)})
        del units, d_hits
        torch.cuda.empty_cache()
        if ms >= 1000.0:
            break
        largest = n
        n *= 2
    result["match"]["squares"] = squares
    result["match"]["largest_square_side_within_1s"] = largest
    ctx.close()
    bl.emit(result, args)


if __name__ == "__main__":
    main()
