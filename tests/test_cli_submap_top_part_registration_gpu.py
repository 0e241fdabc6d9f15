"""GPU: batch_submap_top_part_registration (host C++ over the front end, bev_submap_coarse_registration_device_resident and
bev_submap_voxel_registration_device_resident) end to end.  A half window of 0 with map_leaf 0 writes the report
file and the stdout lines other than [TIME] of batch_top_part_registration, on the scene that test_registration_cli_gpu.py
builds (the BEV path's ordered HDL_64E clouds and moved copies); windows of 5 files under exact relative poses equal the checker
composition (front end's chain, submap_coarse_cases.py, submap_reg_cases.py from the coarse table) through the report
arithmetic of fineicp_lib.report_line, at two chunk sizes; an unreadable cloud exits 1."""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import icp_lib as il
import pcd_util
import reg_cases as rc
import regfront_lib as rl
import submap_coarse_cases as cc
import submap_reg_cases as sc
from bev_amd import synth

pytestmark = pytest.mark.gpu
HOST = Path(bev_amd.PKG_DIR) / "host"
TOOL = "batch_submap_top_part_registration"
THREADS = min(16, os.cpu_count() or 4)
F32 = np.float32
N = 6
# test_cli_submap_registration_gpu.py's poses: rotations about z by multiples of 90 degrees and translations in multiples of
# 0.25 m, so that numpy gives the tool's relative matrices exactly (up to the sign of a zero, which reaches no result)
RZ = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
ROT = [np.eye(3), RZ, RZ @ RZ, np.eye(3), RZ @ RZ @ RZ, RZ]
TRANS = np.array([[0, 0, 0], [0.25, 0.5, 0], [0.75, -0.25, 0.25], [1.5, 0, 0], [1.25, 0.75, 0], [2.0, 0.5, -0.25]], np.float64)
YAW = [0.0, 90.0, 180.0, 0.0, 270.0, 90.0]


@pytest.fixture(scope="module", autouse=True)
def _checkers():
    fl.build()
    il.build()
    rl.build()


def _pose_line(i, rot=None, trans=None):
    rot = ROT[i] if rot is None else rot
    trans = TRANS[i] if trans is None else trans
    return ",".join([str(i)] + [repr(float(v)) for v in trans] + ["0", "0", "0"] + [repr(float(v)) for v in rot.reshape(9)])


def _relative(i, j):
    m = np.zeros((3, 4), np.float64)
    m[:, :3] = ROT[i].T @ ROT[j]
    m[:, 3] = ROT[i].T @ (TRANS[j] - TRANS[i])
    return m.astype(F32).reshape(12)


def _summary(fit):
    ok = int((~(fit > 1.5)).sum())
    bad = len(fit) - ok
    return f"count_success: {ok}, count_failure: {bad}, SR: {'%g' % float(F32(ok) / F32(ok + bad))}. "


def _run(tool, args, cwd, expect=0):
    r = subprocess.run([str(HOST / tool), *[str(a) for a in args]], cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == expect, r.stdout + r.stderr
    return r


def _stdout_without_times(r):
    return re.sub(r"(\[TIME\] Avg Tiempo for \S+ Stage \(\w+\): )\S+", r"\1T", r.stdout)


def test_half_window_0_writes_what_the_top_part_tool_writes(tmp_path):
    """the scene of test_registration_cli_gpu.py: eight HDL_64E sweeps and a moved copy of each, as the BEV path orders them"""
    p = bev_amd.params_for_sensor("HDL_64E")
    rng = np.random.default_rng(31)
    F0 = 8
    base = [synth.sweep(p, 700 + i, keep=0.98, n_dup=2000) for i in range(F0)]
    ctx = bev_amd.BevContext(p, device=0, max_batch=4, max_points=max(len(f) for f in base))
    try:
        yaw = rng.uniform(-15, 15, F0).astype(F32)
        tr = rng.uniform(-1, 1, (F0, 2)).astype(F32)
        moved = [ctx.transform_cloud(base[i], bev_amd.yaw_translate_matrix(float(tr[i, 0]), float(tr[i, 1]), 0.0,
                                                                           float(yaw[i]))) for i in range(F0)]
        ordered = [ctx.process_batch([f], want_multi=False, want_single=False)[0][0] for f in base + moved]
    finally:
        ctx.close()
    root = tmp_path / "kf"
    pcd = root / "non_ground_point_cloud"
    pcd.mkdir(parents=True)
    ids = [3 + 2 * k for k in range(len(ordered))]  # file names are not frame positions
    for k, o in enumerate(ordered):
        pcd_util.write_pcd_binary(pcd / f"{ids[k]:06d}.pcd", o)
    rows = [(i, F0 + i, float(F32(yaw[i] + rng.uniform(-2, 2)))) for i in range(F0)]
    rows += [(i, (i + 1) % F0, float(F32(rng.uniform(-3, 3)))) for i in range(F0)]
    (root / "by_name.txt").write_text("".join(f"{ids[q]} {ids[t]} {a!r}\n" for q, t, a in rows))   # the top-part tool: file names
    (root / "by_place.txt").write_text("".join(f"{q} {t} {a!r}\n" for q, t, a in rows))            # this tool: sorted places
    (root / "keyframe_pose.csv").write_text("\n".join(_pose_line(k, np.eye(3), np.array([0.5 * k, 0.0, 0.0]))
                                                      for k in range(len(ordered))) + "\n")
    (tmp_path / "pair").mkdir()
    (tmp_path / "submap").mkdir()
    pair = _run("batch_top_part_registration", [root / "by_name.txt", pcd], tmp_path / "pair")
    own = _run(TOOL, [root / "by_place.txt", root, 0], tmp_path / "submap")
    assert _stdout_without_times(own) == _stdout_without_times(pair) and "count_success: " in own.stdout
    assert own.stdout.count("[TIME] Avg Tiempo for") == 2
    report = (tmp_path / "submap" / "icp_precision_report.txt").read_bytes()
    assert report == (tmp_path / "pair" / "icp_precision_report.txt").read_bytes() and report.count(b"\n") >= F0
    own0 = _run(TOOL, [root / "by_place.txt", root, 0, 256, 0], tmp_path / "submap")               # map_leaf 0, spelled out
    assert (tmp_path / "submap" / "icp_precision_report.txt").read_bytes() == report
    assert _stdout_without_times(own0) == _stdout_without_times(own)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    rng = np.random.default_rng(515)
    world = rc.scene(2400, 8001)
    w = np.c_[world["x"], world["y"], world["z"]].astype(np.float64)
    clouds = []
    for i in range(N):  # frame i sees a part of the world from pose i
        keep = np.sort(rng.permutation(len(world))[:1500])
        local = (w[keep] - TRANS[i]) @ ROT[i]          # R_i^T (p - t_i)
        c = world[keep].copy()
        c["x"], c["y"], c["z"] = local[:, 0].astype(F32), local[:, 1].astype(F32), local[:, 2].astype(F32)
        clouds.append(c)
    root = tmp_path_factory.mktemp("kf")
    (root / "non_ground_point_cloud").mkdir()
    for i, c in enumerate(clouds):
        pcd_util.write_pcd_binary(root / "non_ground_point_cloud" / f"{i:06d}.pcd", c)
    (root / "keyframe_pose.csv").write_text("\n".join(_pose_line(i) for i in range(N)) + "\n")
    rows = []
    for q, t in [(0, 1), (1, 0), (2, 3), (5, 2), (3, 4), (4, 4), (0, 5), (5, 0), (1, 3)]:
        yaw = (YAW[q] - YAW[t] + 180.0) % 360.0 - 180.0
        rows.append((q, t, float(F32(yaw + rng.uniform(-2, 2)))))
    rows.append((2, 0, 77.0))                          # a wrong guess
    rows.append((0, 1, float(F32(YAW[0] - YAW[1] + 180.0 + 1.0))))   # the right place half a turn away: the second guess's case
    (root / "matches.txt").write_text("".join(f"{q} {t} {a!r}\n" for q, t, a in rows))
    return dict(root=root, clouds=clouds, rows=rows)


def test_half_window_2_equals_the_checker_at_two_chunk_sizes(tree, tmp_path):
    root, rows, clouds = tree["root"], tree["rows"], tree["clouds"]
    maps = sc.Maps()
    for k, (q, t, a) in enumerate(rows):  # one map per match: the window of its key frame, ascending
        maps.add([(j, sc.IDENTITY if j == t else _relative(t, j)) for j in range(max(0, t - 2), min(N - 1, t + 2) + 1)])
    m = sc.matches([(q, k, a) for k, (q, t, a) in enumerate(rows)])
    pn = [rl.chain(c) for c in clouds]
    coarse, best = cc.expected(pn, maps, m, threads=THREADS)
    guesses = [coarse[k, best[k]]["T"].reshape(4, 4).copy() for k in range(len(m))]
    fine = sc.expected(clouds, maps, m, fl.params(**fl.FINE), guesses, threads=THREADS)
    lines = "".join(fl.report_line(fine[k]["T"], guesses[k]) for k in range(len(m)) if not fine[k]["fitness"] > 1.5)
    print(f"coarse states {coarse['state'].tolist()} best {best.tolist()} fine fitness {fine['fitness'].tolist()}")
    assert lines.count("\n") >= 5 and (best == 1).any() and (best == 0).any()
    pair_coarse, pair_best = il.coarse(pn, [tuple(r) for r in sc.matches(rows)], threads=THREADS)
    assert pair_coarse.tobytes() != coarse.tobytes()                       # more than the key frame alone
    outs = {}
    for chunk in ("6", None):
        d = tmp_path / f"chunk{chunk}"
        d.mkdir()
        r = _run(TOOL, [root / "matches.txt", root, 2] + ([chunk] if chunk else []), d)
        assert (d / "icp_precision_report.txt").read_text() == lines, chunk
        assert not (d / "icp_precision_report_submap.txt").exists()
        assert _summary(fine["fitness"]) in r.stdout
        assert re.search(r"\[TIME\] Avg Tiempo for 1st Stage \(coarse\): ", r.stdout)
        assert re.search(r"\[TIME\] Avg Tiempo for 2nd Stage \(fine\): ", r.stdout)
        outs[chunk] = (_stdout_without_times(r), (d / "icp_precision_report.txt").read_bytes())
    assert outs["6"] == outs[None]


def test_an_unreadable_cloud_exits_1(tree, tmp_path):
    root = tmp_path / "kf"
    (root / "non_ground_point_cloud").mkdir(parents=True)
    pcd_util.write_pcd_binary(root / "non_ground_point_cloud" / "000000.pcd", tree["clouds"][0])
    (root / "non_ground_point_cloud" / "000001.pcd").write_bytes(b"this is no point cloud\n")
    (root / "keyframe_pose.csv").write_text("\n".join(_pose_line(i) for i in range(2)) + "\n")
    (root / "m.txt").write_text("0 1 0.0\n")
    r = _run(TOOL, [root / "m.txt", root, 1], tmp_path, expect=1)
    assert "Cloud NOT load file" in r.stderr and "000001.pcd" in r.stderr
