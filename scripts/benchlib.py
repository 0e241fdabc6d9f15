"""What the scripts/bench_*.py scripts share: the workloads, the windows of a map, the measurement protocol and the JSON line
(DESIGN.md §6y).  A script keeps its arguments, the two calls it compares and the fields of its result; ratios between scripts
mean something only while all of them draw from the generator in the same order and fence the same way, and this is the one
place where they do (tests/test_benchlib_cpu.py pins the draws and the protocol against the text the scripts once carried).

Registration family.  The frames are bench.py's default workload (synthetic HDL_64E sweeps, 98 % of the slots, 5,000
duplicates) plus a moved copy (seeded yaw within +-20 degrees, translation within +-1.5 m, by bev_transform_cloud) of each of
the first --moved frames, run once through bev_process_device_resident: d_ord is the d_ordered layout, which the fine calls
read; front_end() makes the PointNormal rows (leaf 0.2, radius 2) the coarse calls read.  The matches are the moved-copy pairs
(frame i against its copy, the yaw within +-2 degrees as the guess).  For a window of W entries the map of match i holds the
copies i - W // 2 .. i + W // 2 (cyclic), the centre under the identity, the others under a seeded planar matrix within
+-1 degree and +-0.3 m; W = 1 is the pair call's problem.  A window of W runs on the first n matches of --window-matches W:n (a
match against 21 full sweeps takes seconds).

Raster family.  The frames are marked HDL_64E sweeps (ordered and ground-marked by the oracle: what
bev_process_device_resident leaves in d_ordered), --distinct of them tiled to --frames.  The submap scripts' windows slide at
stride 1 (map i = frames i - W // 2 .. i + W // 2, clipped), frame j in map i under 2 m along x and 1 degree of yaw per frame
of distance j - i, the key frame itself under the identity.

Protocol.  A fenced step is (launch, bev_synchronize) between two perf_counter readings.  Two calls are compared by
alternation, [a, b] round by round after one unrecorded run of each, and reported as medians; one call alone by timed(): the
median of fenced steps and the mean of unfenced ones (back to back, one synchronisation at the end).  Kernel times come from
bev_profile_get over one more step.  Every line names the machine and the library measured: BEV_AMD_LIB selects another build,
--label names it in the line."""
import json
import os
import re
import socket
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from types import SimpleNamespace

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "point-cloud-preprocessing-tools_amd"))
sys.path.insert(0, str(REPO / "tests"))

_ARGS = {"frames": (int, None), "moved": (int, None), "sub_batch": (int, None), "rounds": (int, None),
         "window_matches": (str, "W:n pairs: the window sizes and their matches"), "steps": (int, None), "warmup": (int, None),
         "distinct": (int, "distinct sweeps the frames are tiled from"), "out": (str, None), "label": (str, None)}


def std_args(ap, **defaults):
    """the arguments several scripts define identically, in the order given, each with the script's default (out: a file name
    under profiles/, or None for no file); --label always"""
    for name, default in {**defaults, "label": None}.items():
        kind, text = _ARGS[name]
        if name == "out" and default is not None:
            default = str(REPO / "profiles" / default)
        ap.add_argument("--" + name.replace("_", "-"), type=kind, default=default, help=text)


# ---- workloads

def sweeps(p, n):
    from bev_amd import synth
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda i: synth.sweep(p, i, keep=0.98, n_dup=5000), range(n)))


def upload(frames, dev):
    """(offsets, the frames' bytes on the device)"""
    import torch
    offs = np.zeros(len(frames) + 1, np.uint64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    return offs, torch.from_numpy(np.concatenate(frames).view(np.uint8).reshape(-1)).to(dev)


def bev_outputs(p, F, dev):
    """d_ord, d_multi, d_single of bev_process_device_resident over F frames, allocated in that order"""
    import torch
    return (torch.empty(F * p.slots * 32, dtype=torch.uint8, device=dev),
            torch.empty(F * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device=dev),
            torch.empty(F * p.mat_size ** 2, dtype=torch.uint8, device=dev))


def world_draws(M):
    """the generator and the moved copies' yaw and translation: the first draws of every registration script"""
    rng = np.random.default_rng(2026)
    yaw = rng.uniform(-20, 20, M).astype(np.float32)
    tr = rng.uniform(-1.5, 1.5, (M, 2)).astype(np.float32)
    return rng, yaw, tr


def moved_copies(ctx, frames, yaw, tr):
    import bev_amd
    return [ctx.transform_cloud(frames[i], bev_amd.yaw_translate_matrix(float(tr[i, 0]), float(tr[i, 1]), 0.0, float(yaw[i])))
            for i in range(len(yaw))]


def registration_world(args):
    """--frames sweeps and --moved moved copies, processed into d_ord; the inputs and the images are released.  The
    generator comes back in the state the draws left it in: the pairs and the windows go on from there."""
    import torch

    import bev_amd

    p = bev_amd.params_for_sensor("HDL_64E")
    F0, M = args.frames, args.moved
    dev = torch.device("cuda:0")
    frames = sweeps(p, F0)
    ctx = bev_amd.BevContext(p, device=0, max_batch=args.sub_batch, max_points=max(len(f) for f in frames))
    rng, yaw, tr = world_draws(M)
    frames += moved_copies(ctx, frames, yaw, tr)
    F = len(frames)
    offs, d_in = upload(frames, dev)
    del frames
    d_ord, d_multi, d_single = bev_outputs(p, F, dev)
    torch.cuda.synchronize()
    ctx.process_device(F, d_in.data_ptr(), offs, d_ord.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
    ctx.synchronize()
    del d_in, d_multi, d_single
    return SimpleNamespace(ctx=ctx, d_ord=d_ord, rng=rng, yaw=yaw, F0=F0, M=M, F=F, S=p.slots, dev=dev)


def front_end(w):
    """(stride, d_pn, d_cnt): the world's frames through the registration front end.  d_ord stays: a script whose timed calls
    ran without it deletes w.d_ord itself."""
    import torch

    import bev_amd

    stride = bev_amd.regfront_max_out(w.S)
    d_pn = torch.empty(w.F * stride * 48, dtype=torch.uint8, device=w.dev)
    d_cnt = torch.zeros(w.F, dtype=torch.int32, device=w.dev)
    w.ctx.registration_front_device(w.F, w.d_ord.data_ptr(), None, d_pn.data_ptr(), stride, d_cnt.data_ptr())
    w.ctx.synchronize()
    return stride, d_pn, d_cnt


def tiled_marked_frames(p, distinct, F, dev):
    """oracle-ordered and marked synth.sweep(p, s) for s < distinct, tiled to F frames on the device: .clouds (host), .d_clouds,
    .offs (f * S), and .up, the distinct uploads, which stay allocated while the calls are timed, as they always did"""
    import torch

    import oracle_lib as orc
    from bev_amd import synth

    sp, S = orc.sensor_from_params(p), p.slots
    clouds = [orc.mark_ground(sp, orc.order_cloud(sp, synth.sweep(p, s)))[0] for s in range(distinct)]
    up = [torch.from_numpy(c.view(np.uint8).reshape(-1).copy()).to(dev) for c in clouds]
    d_clouds = torch.empty(F * S * 32, dtype=torch.uint8, device=dev)
    for f in range(F):
        d_clouds[f * S * 32:(f + 1) * S * 32] = up[f % len(up)]
    return SimpleNamespace(clouds=clouds, up=up, d_clouds=d_clouds, offs=np.arange(F + 1, dtype=np.uint64) * np.uint64(S))


def frame_poses(rng, F, n_poses):
    """n_poses seeded matrices per frame (None for 0): within +-5 m, +-0.5 m of height, any yaw"""
    import bev_amd
    if not n_poses:
        return None
    return np.stack([np.stack([bev_amd.yaw_translate_matrix(rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-0.5, 0.5),
                                                            rng.uniform(-180, 180)) for _ in range(n_poses)]) for _ in range(F)])


def copy_rate(path, result):
    """runs the built scripts/microbench/copybw.hip (in the same process tree on the same machine: its best plain-copy rate is
    the yardstick), records it in the result; the rate in TB/s, or None"""
    if not path:
        return None
    out = subprocess.run([path], capture_output=True, text=True, timeout=600).stdout
    rates = [float(m.group(1)) for m in re.finditer(r"^copy .*? ([0-9.]+) TB/s$", out, flags=re.M)]
    tbs = max(rates) if rates else None
    result["copy_rate_GBps"] = tbs * 1e3 if tbs else None
    result["copybw_lines"] = [l.strip() for l in out.splitlines() if l.startswith(("copy", "grid"))]
    return tbs


# ---- problems

def moved_copy_pairs(w, n=None):
    """frame i against its moved copy, the yaw within +-2 degrees as the guess, for the first n (default all) copies: n draws"""
    import bev_amd
    n = w.M if n is None else n
    pairs = np.zeros(n, bev_amd.MATCH_DTYPE)
    pairs["query_idx"] = np.arange(n)
    pairs["match_idx"] = w.F0 + np.arange(n)
    pairs["angle_guess"] = w.yaw[:n] + w.rng.uniform(-2, 2, n).astype(np.float32)
    return pairs


def map_matches(pairs, n):
    """the first n pairs as matches against maps: match i against map i"""
    m = pairs[:n].copy()
    m["match_idx"] = np.arange(n)
    return m


def parse_window_matches(text, M):
    return [(int(w.split(":")[0]), min(M, int(w.split(":")[1]))) for w in text.split(",")]


def cyclic_windows(rng, F0, M, n, W):
    """(map_offs, entry_frame, entry_pose) of n maps of W entries; three draws per entry off the centre, none for the centre"""
    import bev_amd
    half = W // 2
    identity = np.eye(3, 4, dtype=np.float32).reshape(12)
    map_offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(W)
    entry_frame = np.zeros(n * W, np.int32)
    entry_pose = np.zeros((n * W, 12), np.float32)
    for i in range(n):
        for k, d in enumerate(range(-half, half + 1)):
            entry_frame[i * W + k] = F0 + (i + d) % M
            entry_pose[i * W + k] = identity if d == 0 else bev_amd.yaw_translate_matrix(
                float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.3, 0.3)), 0.0, float(rng.uniform(-1, 1)))
    return map_offs, entry_frame, entry_pose


def best_fitness(r, best):
    """the fitness of each match's chosen problem (coarse results: two problems per match)"""
    f = r.reshape(-1, 2)["fitness"][np.arange(len(best)), best]
    return {"median": float(np.median(f)), "max": float(f.max()), "above_1.5": int((f > 1.5).sum())}


def relative_poses(W):
    """{d: the pose of a frame d frames from the key frame}, d = -W // 2 .. W // 2"""
    import bev_amd
    rel = {d: bev_amd.yaw_translate_matrix(2.0 * d, 0.0, 0.0, 1.0 * d) for d in range(-(W // 2), W // 2 + 1)}
    assert np.array_equal(rel[0], np.eye(3, 4, dtype=np.float32).reshape(12))
    return rel


def sliding_windows(F, W, rel):
    """(windows, map_offs, entry_frame, entry_pose): map i = frames i - W // 2 .. i + W // 2, clipped to the frames there are"""
    h = W // 2
    windows = [range(max(0, i - h), min(F - 1, i + h) + 1) for i in range(F)]
    map_offs = np.zeros(F + 1, dtype=np.uint64)
    map_offs[1:] = np.cumsum([len(w) for w in windows])
    entry_frame = np.array([j for w in windows for j in w], dtype=np.int32)
    entry_pose = np.stack([rel[j - i] for i, w in enumerate(windows) for j in w])
    return windows, map_offs, entry_frame, entry_pose


# ---- protocol

def fenced(ctx, step, log=True):
    t = time.perf_counter()
    step()
    ctx.synchronize()
    t = time.perf_counter() - t
    if log:
        print(f"  step {t * 1e3:.1f} ms", file=sys.stderr, flush=True)
    return t


def alternate(ctx, a, b, rounds, warm=True, log=True):
    """one unrecorded fenced run of each (warm), then `rounds` times [a, b]; the two lists of seconds"""
    if warm:
        fenced(ctx, a, log)
        fenced(ctx, b, log)
    t_a, t_b = [], []
    for _ in range(rounds):
        t_a.append(fenced(ctx, a, log))
        t_b.append(fenced(ctx, b, log))
    return t_a, t_b


def timed(ctx, step, steps, warmup):
    """(median of `steps` fenced steps, mean of `steps` unfenced steps), in seconds, after `warmup` steps"""
    for _ in range(warmup):
        step()
    ctx.synchronize()
    times = [fenced(ctx, step, log=False) for _ in range(steps)]
    t = time.perf_counter()
    for _ in range(steps):
        step()
    ctx.synchronize()
    return statistics.median(times), (time.perf_counter() - t) / steps


def kernel_ms(ctx, step, prefix="", names=None):
    """one profiled step: {name: total_ms} of the kernels whose name starts with `prefix` (a string or a tuple of them), or,
    with `names`, {name: {"ms_per_step", "launches"}} of those that ran"""
    ctx.profile_reset()
    ctx.profile_enable(True)
    step()
    ctx.synchronize()
    got = ctx.profile_get()
    ctx.profile_enable(False)
    if names is None:
        return {k["name"]: k["total_ms"] for k in got if k["name"].startswith(prefix)}
    got = {k["name"]: k for k in got}
    return {n: {"ms_per_step": got[n]["total_ms"], "launches": got[n]["launches"]} for n in names if n in got}


# ---- the line

def device_name():
    import torch
    return torch.cuda.get_device_name(0)


def emit(result, args, machine=("device", "host"), final=True):
    """completes the result (the machine's keys the script has always reported, the library measured), writes it to --out where
    the script has one, and, unless this is a partial result saved on the way (final=False), prints it: one JSON line"""
    if "device" in machine:
        result["device"] = device_name()
    if "host" in machine:
        result["host"] = socket.gethostname()
    result["library"] = args.label or os.environ.get("BEV_AMD_LIB", "csrc/libbev_mi355x.so")
    line = json.dumps(result)
    if final:
        print(line)
    if getattr(args, "out", None):
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
