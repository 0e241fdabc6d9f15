"""GPU: the registration stages past one launch group, on ragged and skewed clouds (the seeded cases of tests/reg_cases.py,
anchored on the host by test_registration_cases_cpu.py).  Every result of every frame and every match is compared byte for
byte with the sequential checkers (tests/fineicp, tests/icp, tests/regfront):

  a. the batched fine entry on 600 ragged packed frames and more than 2348 matches — three voxel groups of 256 slots, three
     launches of 1024 problems — with the whole tool's yaw guesses and with guesses read from an uploaded coarse table;
  b. the batched coarse entry on PointNormal frames longer than the stride (d_counts[f] > stride), empty and tiny frames;
  c. the front end at eight (leaf, radius) pairs, on d_ordered frames and on packed frames with several oversized cells,
     with a guard region behind d_out, then with more than 1024 packed frames on the same context;
  d. the per-problem entries on geometry that degenerates the search grid and on sources at the chunk boundaries;
  e. calls of different sizes on one context with no synchronisation in between, and calls right behind work the caller
     queued on the default stream.
"""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import icp_lib as il
import reg_cases as rc
import regfront_lib as rl
from bev_amd import ICP_RESULT_DTYPE, POINT_DTYPE, synth

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 4)
F32 = np.float32
R = ICP_RESULT_DTYPE.itemsize


@pytest.fixture(scope="module", autouse=True)
def _checker():
    fl.build()
    il.build()
    rl.build()


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(name, got, exp):
    """Every record of got against exp; on a mismatch how many differ and the first."""
    assert len(got) == len(exp), f"{name}: {len(got)} records, expected {len(exp)}"
    bad = [k for k in range(len(exp)) if not _same(got[k], exp[k])]
    assert not bad, f"{name}: {len(bad)} of {len(exp)} differ, first {bad[0]}: {got[bad[0]]} != {exp[bad[0]]}"


def _pmap(fn, items):
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(fn, items))


def _dev(a):
    """A host array's bytes on the device."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(torch.device("cuda:0"))


def _results(d, shape=-1):
    return d.cpu().numpy().view(ICP_RESULT_DTYPE).reshape(shape)


def _ctx(sensor="HDL_32E", max_batch=2, max_points=1000):
    return bev_amd.BevContext(bev_amd.params_for_sensor(sensor), device=0, max_batch=max_batch, max_points=max_points)


@functools.lru_cache(maxsize=None)
def _pack():
    """The ragged pack, its matches, the made-up coarse table and the checker's results under both tools' settings."""
    pack = rc.ragged_pack()
    m, truth = rc.ragged_matches(pack)
    coarse, best, guesses = rc.synthetic_coarse(m, truth)
    whole = fl.fine(pack.clouds, m, None, fl.params(**fl.WHOLE), threads=THREADS)
    top = fl.fine(pack.clouds, m, guesses, fl.params(**fl.FINE), threads=THREADS)
    return dict(pack=pack, m=m, coarse=coarse, best=best, guesses=guesses, whole=whole, top=top,
                bytes=rc.packed(pack.clouds))


@functools.lru_cache(maxsize=None)
def _coarse():
    """The coarse entry's frames (cut at the stride, as the kernels read them) and the checker's results."""
    pack = _pack()["pack"]
    cf = rc.coarse_frames(pack, rl.chain)
    cut = [f[: min(len(f), cf.stride)] for f in cf.frames]
    exp, exp_best = il.coarse(cut, cf.matches, threads=THREADS)
    m4 = cf.matches[:4].copy()
    exp4, exp_best4 = il.coarse(cut, m4, threads=THREADS)
    return dict(cf=cf, pn=rc.strided(cf.frames, cf.stride), exp=exp, exp_best=exp_best, m4=m4, exp4=exp4, exp_best4=exp_best4)


def _fine_whole(ctx, P, d_clouds, d_res):
    ctx.fine_registration_device(len(P["pack"].clouds), d_clouds.data_ptr(), P["pack"].offsets, P["m"], d_res.data_ptr(),
                                 params=bev_amd.icp_whole_defaults())


def _fine_top(ctx, P, d_clouds, d_res, d_coarse, d_best):
    ctx.fine_registration_device(len(P["pack"].clouds), d_clouds.data_ptr(), P["pack"].offsets, P["m"], d_res.data_ptr(),
                                 d_coarse.data_ptr(), d_best.data_ptr())


# ---- a. the fine stage on the ragged pack -------------------------------------------------------------------------------
def test_fine_stage_on_the_ragged_pack_equals_the_checker():
    import torch

    P = _pack()
    pack, m = P["pack"], P["m"]
    n = len(m)
    pos = rc.slot_positions(m)
    assert n > 2 * rc.PROBLEMS_PER_LAUNCH and max(pos.values()) >= 2 * rc.FINE_VOXEL_GROUP  # a third launch, a third group
    ctx = _ctx()
    try:
        d_clouds = _dev(P["bytes"])
        d_coarse, d_best = _dev(P["coarse"]), _dev(P["best"])
        d_whole = torch.zeros(n * R, dtype=torch.uint8, device=d_clouds.device)
        d_top = torch.zeros_like(d_whole)
        torch.cuda.synchronize()
        _fine_whole(ctx, P, d_clouds, d_whole)
        _fine_top(ctx, P, d_clouds, d_top, d_coarse, d_best)
        ctx.synchronize()
        whole, top = _results(d_whole), _results(d_top)
        print(f"fine: {n} matches, {len(pos)} slots; states whole {np.bincount(whole['state'], minlength=6)} "
              f"top-part {np.bincount(top['state'], minlength=6)}")
        _check("whole", whole, P["whole"])
        _check("top-part", top, P["top"])
        # the voxel clouds are visible only through the results: every named frame that can register is in one that did
        for name, exp in (("whole", P["whole"]), ("top-part", P["top"])):
            seen = set()
            for k in np.nonzero(exp["state"] != bev_amd.ICP_NO_CORRESPONDENCES)[0]:
                seen |= {int(m["query_idx"][k]), int(m["match_idx"][k])}
            missed = [f for f in pos if f not in seen and f not in pack.degenerate]
            assert not missed, f"{name}: frames in no compared registration: {missed}"
        for name, f in pack.special.items():  # the special frames one by one
            for g in (f, pack.half + f):
                got, exp = ctx.voxel_grid_irct(pack.clouds[g], 0.2), fl.voxel_irct(pack.clouds[g], 0.2)
                assert len(got) == len(exp) and _same(got, exp), f"{name} (frame {g})"
    finally:
        ctx.close()


# ---- b. the coarse stage on ragged PointNormal frames -------------------------------------------------------------------
def _coarse_call(ctx, Cc, d_pn, d_cnt, matches, d_res, d_best):
    cf = Cc["cf"]
    ctx.coarse_registration_device(len(cf.frames), d_pn.data_ptr(), cf.stride, d_cnt.data_ptr(), matches, d_res.data_ptr(),
                                   d_best.data_ptr())


def test_coarse_stage_on_frames_longer_than_the_stride_equals_the_checker():
    import torch

    Cc = _coarse()
    cf = Cc["cf"]
    m = cf.matches
    n = len(m)
    named = set(m["query_idx"].tolist()) | set(m["match_idx"].tolist())
    assert n >= 1100 and any(cf.counts[f] > cf.stride for f in named)
    assert any(cf.counts[f] > cf.stride for f in m["query_idx"].tolist())
    assert any(cf.counts[f] > cf.stride for f in m["match_idx"].tolist())
    ctx = _ctx()
    try:
        d_pn, d_cnt = _dev(Cc["pn"]), _dev(cf.counts)  # the true lengths: some above the stride
        d_res = torch.zeros(n * 2 * R, dtype=torch.uint8, device=d_pn.device)
        d_best = torch.full((n,), -7, dtype=torch.int32, device=d_pn.device)
        torch.cuda.synchronize()
        _coarse_call(ctx, Cc, d_pn, d_cnt, m, d_res, d_best)
        ctx.synchronize()
        got, best = _results(d_res, (n, 2)), d_best.cpu().numpy()
        print(f"coarse: {n} matches, stride {cf.stride}, longest frame {cf.counts.max()}, "
              f"states {np.bincount(got['state'].reshape(-1), minlength=6)}")
        _check("coarse", got, Cc["exp"])
        bad = np.nonzero(best != Cc["exp_best"])[0]
        assert len(bad) == 0, f"best: {len(bad)} of {n} differ, first {bad[0]}: {best[bad[0]]} != {Cc['exp_best'][bad[0]]}"
        assert len(set(np.unique(Cc["exp"]["state"]).tolist())) >= 2 and set(np.unique(best).tolist()) == {0, 1}
    finally:
        ctx.close()


# ---- c. the front end at other leaf sizes and radii -----------------------------------------------------------------------
GUARD = 4096
PATTERN = -12345.5


def _front_call(ctx, n_frames, d_in, offs, n_max, leaf, radius, vp=(0.0, 0.0, 0.0)):
    """One call with out_stride == bev_regfront_max_out(n_max) exactly and a guard region behind d_out: (counts, rows)."""
    import torch

    stride = bev_amd.regfront_max_out(n_max)
    d_out = torch.full((n_frames * stride * 12 + GUARD,), PATTERN, dtype=torch.float32, device=d_in.device)
    d_cnt = torch.full((n_frames + 64,), -7, dtype=torch.int32, device=d_in.device)
    torch.cuda.synchronize()
    ctx.registration_front_device(n_frames, d_in.data_ptr(), offs, d_out.data_ptr(), stride, d_cnt.data_ptr(), leaf, radius,
                                  vp)
    ctx.synchronize()
    out, cnt = d_out.cpu().numpy(), d_cnt.cpu().numpy()
    assert (out[n_frames * stride * 12:] == F32(PATTERN)).all(), "the guard region behind d_out was written"
    assert (cnt[n_frames:] == -7).all(), "d_counts was written past n_frames"
    assert (cnt[:n_frames] >= 0).all() and (cnt[:n_frames] <= stride).all(), "a count above out_stride"
    return cnt[:n_frames].astype(np.int64), out[: n_frames * stride * 12].reshape(n_frames, stride, 12)


def _front_check(name, clouds, cnt, out, leaf, radius, vp=(0.0, 0.0, 0.0)):
    exp = _pmap(lambda c: rl.chain(c, leaf, radius, vp), clouds)
    bad = [f for f in range(len(clouds)) if cnt[f] != len(exp[f]) or not _same(out[f, : cnt[f]], exp[f])]
    assert not bad, (f"{name} leaf {leaf} radius {radius}: {len(bad)} of {len(clouds)} frames differ, first {bad[0]}: "
                     f"{cnt[bad[0]]} rows, expected {len(exp[bad[0]])}")
    return exp


PAIRS = [(lr, (0.0, 0.0, 0.0)) for lr in rc.LEAF_RADIUS] + [((0.35, 3.3), (5.0, -3.0, 0.0))]


def test_front_end_at_other_leaf_sizes_and_radii_equals_the_checker():
    import torch

    p = bev_amd.params_for_sensor("HDL_64E")
    S, F = p.slots, 8
    dev = torch.device("cuda:0")
    frames = _pmap(lambda i: synth.sweep(p, 61000 + i, keep=0.98, n_dup=2000), range(F))
    fp = rc.front_pack(_pack()["pack"])
    small = rc.small_frames()
    n_max = max(len(c) for c in fp.clouds)
    ctx = bev_amd.BevContext(p, device=0, max_batch=5, max_points=max(n_max, max(len(f) for f in frames)))
    try:
        assert len(fp.clouds) > ctx.max_batch and len(fp.clouds) % ctx.max_batch != 0
        offs = np.zeros(F + 1, np.uint64)
        offs[1:] = np.cumsum([len(f) for f in frames])
        d_in = _dev(np.concatenate(frames))
        d_ord = torch.zeros(F * S * 32, dtype=torch.uint8, device=dev)
        d_multi = torch.zeros(F * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device=dev)
        d_single = torch.zeros(F * p.mat_size ** 2, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.process_device(F, d_in.data_ptr(), offs, d_ord.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
        ctx.synchronize()
        ordered = list(d_ord.cpu().numpy().view(POINT_DTYPE).reshape(F, S))
        p_offs = np.zeros(len(fp.clouds) + 1, np.uint64)
        p_offs[1:] = np.cumsum([len(c) for c in fp.clouds])
        d_pack = _dev(rc.packed(fp.clouds))
        rows_seen = set()
        for (leaf, radius), vp in PAIRS:
            cnt, out = _front_call(ctx, F, d_ord, None, S, leaf, radius, vp)
            _front_check("d_ordered", ordered, cnt, out, leaf, radius, vp)
            assert cnt.min() > 0
            cnt, out = _front_call(ctx, len(fp.clouds), d_pack, p_offs, n_max, leaf, radius, vp)
            exp = _front_check("packed", fp.clouds, cnt, out, leaf, radius, vp)
            rows_seen |= {min(len(e), 2) for e in exp}
            print(f"front end leaf {leaf} radius {radius} viewpoint {vp}: rows {cnt.tolist()}")
        assert rows_seen == {0, 1, 2}  # empty frames, one-voxel frames, the rest
        # more than 1024 packed frames on the same context: the offsets table grows
        assert len(small) > 1024 > len(fp.clouds)
        s_offs = np.zeros(len(small) + 1, np.uint64)
        s_offs[1:] = np.cumsum([len(c) for c in small])
        d_small = _dev(rc.packed(small))
        cnt, out = _front_call(ctx, len(small), d_small, s_offs, max(len(c) for c in small), 0.2, 2.0)
        _front_check("1100 small frames", small, cnt, out, 0.2, 2.0)
        assert (cnt > 0).sum() > 100
        # and the first packed set again behind it
        cnt, out = _front_call(ctx, len(fp.clouds), d_pack, p_offs, n_max, 0.35, 3.3)
        _front_check("packed again", fp.clouds, cnt, out, 0.35, 3.3)
    finally:
        ctx.close()


# ---- d. the per-problem entries on skewed geometry and at the chunk boundaries ------------------------------------------
def _p2p_settings():
    return [("top-part", fl.params(**fl.FINE)), ("whole", fl.params(**fl.WHOLE)),
            ("D 1e-3", fl.params(max_correspondence_distance=1e-3, max_iterations=5)),
            ("D 1e6", fl.params(max_correspondence_distance=1e6, max_iterations=5))]


def _p2plane_settings():
    return [("D 10", bev_amd.icp_params(max_correspondence_distance=10.0)),
            ("D 0.7", bev_amd.icp_params(max_correspondence_distance=0.7))]


def test_per_problem_entries_on_skewed_geometry_and_chunk_boundaries_equal_the_checker():
    p2p, p2plane = [], []
    for name, tgt in rc.skewed_targets():
        for kind in rc.SOURCE_KINDS:
            for label, prm in _p2p_settings():
                src = rc.skewed_source(name, tgt, kind, prm.max_correspondence_distance)
                p2p.append((f"{name} / {kind} / {label}", src, tgt, prm))
            for label, prm in _p2plane_settings():
                src = rc.skewed_source(name, tgt, kind, prm.max_correspondence_distance)
                p2plane.append((f"{name} / {kind} / {label}", rc.point_normals(src, 1), rc.point_normals(tgt, 2), prm))
    full = rc.scene(max(rc.CHUNK_SIZES), 77)
    xyz = lambda c: np.c_[c["x"], c["y"], c["z"]].astype(F32)
    tgt = xyz(rc.moved(full, 3.0, 0.3, -0.2))
    for n in rc.CHUNK_SIZES:  # 63 .. 65: one chunk and the next; 2047 .. 2049: the 32 chunk sums in LDS and the next round
        for label, prm in _p2p_settings()[:2]:
            p2p.append((f"scene of {n} / {label}", xyz(full[:n]), tgt, prm))
        for label, prm in _p2plane_settings():
            p2plane.append((f"scene of {n} / {label}", rc.point_normals(xyz(full[:n]), 3), rc.point_normals(tgt, 4), prm))
    assert {len(c[1]) for c in p2p if c[0].split(" / ")[0] in rc.ONE_CELL} == {rc.SKEW_N}
    exp_p2p = _pmap(lambda c: fl.run(c[1], c[2], None, c[3]), p2p)
    exp_p2plane = _pmap(lambda c: il.run(c[1], c[2], None, c[3]), p2plane)
    ctx = _ctx()
    try:
        got_p2p = [ctx.icp_point_to_point(c[1], c[2], None, c[3]) for c in p2p]
        got_p2plane = [ctx.icp_point_to_plane(c[1], c[2], None, c[3]) for c in p2plane]
    finally:
        ctx.close()
    for what, cases, got, exp, ends in (("point to point", p2p, got_p2p, exp_p2p, 2),
                                        ("point to plane", p2plane, got_p2plane, exp_p2plane, 1)):
        states = np.bincount([int(e["state"]) for e in exp], minlength=6)
        print(f"{what}: {len(cases)} problems, states {states}")
        bad = [k for k in range(len(cases)) if not _same(got[k], exp[k])]
        assert not bad, (f"{what}: {len(bad)} of {len(cases)} differ, first {cases[bad[0]][0]}: {got[bad[0]]} != {exp[bad[0]]}; "
                         f"all: {[cases[k][0] for k in bad]}")
        assert states[bev_amd.ICP_NO_CORRESPONDENCES] > 0 and (states[1:5] > 0).sum() >= ends  # (the coarse settings end on the count)


# ---- e. reuse and ordering ------------------------------------------------------------------------------------------------
def test_calls_of_different_sizes_on_one_context_without_a_sync_equal_the_checker():
    import torch

    P, Cc = _pack(), _coarse()
    pack, m, cf = P["pack"], P["m"], Cc["cf"]
    n, nc = len(m), len(cf.matches)
    small = [rc.scene(700, 501), rc.moved(rc.scene(700, 501), 4.0, 0.3, 0.1), rc.scene(65, 502)]
    small_m = np.array([(0, 1, 3.0), (2, 0, 0.0)], bev_amd.MATCH_DTYPE)
    small_offs = np.zeros(4, np.uint64)
    small_offs[1:] = np.cumsum([len(c) for c in small])
    exp_small = fl.fine(small, small_m, None, fl.params(**fl.FINE), threads=THREADS)
    a100, b100 = rc.scene(100, 503), rc.moved(rc.scene(100, 503), 2.0, 0.1, -0.1)
    exp_100 = fl.run(a100, b100)
    ctx = _ctx()
    try:
        dev = torch.device("cuda:0")
        d_clouds, d_small_in = _dev(P["bytes"]), _dev(np.concatenate(small))
        d_pn, d_cnt = _dev(Cc["pn"]), _dev(cf.counts)
        d_res1 = torch.zeros(n * R, dtype=torch.uint8, device=dev)
        d_res2 = torch.zeros_like(d_res1)
        d_small = torch.zeros(len(small_m) * R, dtype=torch.uint8, device=dev)
        d_c4 = torch.zeros(4 * 2 * R, dtype=torch.uint8, device=dev)
        d_b4 = torch.full((4,), -7, dtype=torch.int32, device=dev)
        d_cres = torch.zeros(nc * 2 * R, dtype=torch.uint8, device=dev)
        d_cbest = torch.full((nc,), -7, dtype=torch.int32, device=dev)
        d_small0 = torch.zeros_like(d_small)
        torch.cuda.synchronize()
        # 0: a small call first, so that call 1 grows the workspace and both tables of a context that is in use
        ctx.fine_registration_device(3, d_small_in.data_ptr(), small_offs, small_m, d_small0.data_ptr())
        _fine_whole(ctx, P, d_clouds, d_res1)                                                   # 1
        ctx.fine_registration_device(3, d_small_in.data_ptr(), small_offs, small_m, d_small.data_ptr())  # 2
        got_100 = ctx.icp_point_to_point(a100, b100)                                           # 3 (syncs by itself)
        _fine_whole(ctx, P, d_clouds, d_res2)                                                   # 4
        _coarse_call(ctx, Cc, d_pn, d_cnt, Cc["m4"], d_c4, d_b4)                                # 5
        _coarse_call(ctx, Cc, d_pn, d_cnt, cf.matches, d_cres, d_cbest)                         # 6
        ctx.synchronize()
        _check("0: three frames first", _results(d_small0), exp_small)
        _check("1: whole", _results(d_res1), P["whole"])
        _check("2: three frames", _results(d_small), exp_small)
        assert _same(got_100, exp_100), f"3: {got_100} != {exp_100}"
        _check("4: whole again", _results(d_res2), P["whole"])
        assert _same(d_res1.cpu().numpy(), d_res2.cpu().numpy())
        _check("5: four coarse matches", _results(d_c4, (4, 2)), Cc["exp4"])
        assert np.array_equal(d_b4.cpu().numpy(), Cc["exp_best4"])
        _check("6: coarse", _results(d_cres, (nc, 2)), Cc["exp"])
        assert np.array_equal(d_cbest.cpu().numpy(), Cc["exp_best"])
    finally:
        ctx.close()


def _pinned(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).pin_memory()


def test_entries_wait_for_work_queued_on_the_default_stream():
    """A non-blocking upload of the inputs and a fill of the outputs queued on the default stream, then the call at once:
    the library waits for both, and the fill does not land on top of the results."""
    import torch

    P, Cc = _pack(), _coarse()
    pack, m, cf = P["pack"], P["m"], Cc["cf"]
    n, nc = len(m), len(cf.matches)
    fp = rc.front_pack(pack)
    f_offs = np.zeros(len(fp.clouds) + 1, np.uint64)
    f_offs[1:] = np.cumsum([len(c) for c in fp.clouds])
    f_max = max(len(c) for c in fp.clouds)
    f_stride = bev_amd.regfront_max_out(f_max)
    exp_front = _pmap(rl.chain, fp.clouds)
    dev = torch.device("cuda:0")
    h_clouds, h_coarse, h_best = _pinned(P["bytes"]), _pinned(P["coarse"]), _pinned(P["best"])
    h_pn, h_cnt, h_front = _pinned(Cc["pn"]), _pinned(cf.counts), _pinned(rc.packed(fp.clouds))
    ctx = _ctx(max_batch=5, max_points=f_max)
    try:
        # fine entry
        d_clouds, d_coarse, d_best = (torch.zeros(h.numel(), dtype=torch.uint8, device=dev) for h in (h_clouds, h_coarse, h_best))
        d_res = torch.zeros(n * R, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        d_clouds.copy_(h_clouds, non_blocking=True)
        d_coarse.copy_(h_coarse, non_blocking=True)
        d_best.copy_(h_best, non_blocking=True)
        d_res.fill_(0xFF)
        _fine_top(ctx, P, d_clouds, d_res, d_coarse, d_best)
        ctx.synchronize()
        _check("fine behind an upload and a fill", _results(d_res), P["top"])
        # coarse entry
        d_pn, d_cnt = (torch.zeros(h.numel(), dtype=torch.uint8, device=dev) for h in (h_pn, h_cnt))
        d_cres = torch.zeros(nc * 2 * R, dtype=torch.uint8, device=dev)
        d_cbest = torch.zeros(nc, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        d_pn.copy_(h_pn, non_blocking=True)
        d_cnt.copy_(h_cnt, non_blocking=True)
        d_cres.fill_(0xFF)
        d_cbest.fill_(-7)
        _coarse_call(ctx, Cc, d_pn, d_cnt, cf.matches, d_cres, d_cbest)
        ctx.synchronize()
        _check("coarse behind an upload and a fill", _results(d_cres, (nc, 2)), Cc["exp"])
        assert np.array_equal(d_cbest.cpu().numpy(), Cc["exp_best"])
        # front end
        d_front = torch.zeros(h_front.numel(), dtype=torch.uint8, device=dev)
        d_out = torch.zeros(len(fp.clouds) * f_stride * 12, dtype=torch.float32, device=dev)
        d_fcnt = torch.zeros(len(fp.clouds), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        d_front.copy_(h_front, non_blocking=True)
        d_out.fill_(PATTERN)
        d_fcnt.fill_(-7)
        ctx.registration_front_device(len(fp.clouds), d_front.data_ptr(), f_offs, d_out.data_ptr(), f_stride,
                                      d_fcnt.data_ptr())
        ctx.synchronize()
        cnt = d_fcnt.cpu().numpy()
        out = d_out.cpu().numpy().reshape(len(fp.clouds), f_stride, 12)
        bad = [f for f in range(len(fp.clouds)) if cnt[f] != len(exp_front[f]) or not _same(out[f, : cnt[f]], exp_front[f])]
        assert not bad, f"front end behind an upload and a fill: {len(bad)} of {len(fp.clouds)} frames differ, first {bad[0]}"
    finally:
        ctx.close()
