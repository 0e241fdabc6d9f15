"""GPU: batch_submap_registration with its optional <map_leaf> (host C++ over bev_submap_voxel_registration_device_resident;
DESIGN.md §6l) end to end on a small tree of PCD files and a pose file.  <map_leaf> 0 and absent write identical files; 0.2 at
half window 2 equals the checker composition (submap_vox_cases.py) through the report arithmetic of fineicp_lib.report_line,
at two chunk sizes."""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import pcd_util
import reg_cases as rc
import submap_reg_cases as sc
import submap_vox_cases as vc

pytestmark = pytest.mark.gpu
HOST = Path(bev_amd.PKG_DIR) / "host"
THREADS = min(16, os.cpu_count() or 4)
F32 = np.float32
N = 6
# Rotations about z by multiples of 90 degrees and translations in multiples of 0.25 m: every product and sum of R_i^T R_j and
# R_i^T (t_j - t_i) is exact in double, so numpy gives the tool's matrices (up to the sign of a zero, which reaches no result).
RZ = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
ROT = [np.eye(3), RZ, RZ @ RZ, np.eye(3), RZ @ RZ @ RZ, RZ]
TRANS = np.array([[0, 0, 0], [0.25, 0.5, 0], [0.75, -0.25, 0.25], [1.5, 0, 0], [1.25, 0.75, 0], [2.0, 0.5, -0.25]], np.float64)
YAW = [0.0, 90.0, 180.0, 0.0, 270.0, 90.0]
REPORTS = ("icp_precision_report_submap.txt", "icp_precision_report_3d_icp_directly.txt")


def _pose_line(i):
    return ",".join([str(i)] + [repr(float(v)) for v in TRANS[i]] + ["0", "0", "0"] + [repr(float(v)) for v in ROT[i].reshape(9)])


def _relative(i, j):
    m = np.zeros((3, 4), np.float64)
    m[:, :3] = ROT[i].T @ ROT[j]
    m[:, 3] = ROT[i].T @ (TRANS[j] - TRANS[i])
    return m.astype(F32).reshape(12)


def _summary(fit):
    ok = int((~(fit > 1.5)).sum())
    bad = len(fit) - ok
    return f"count_success: {ok}, count_failure: {bad}, SR: {'%g' % float(F32(ok) / F32(ok + bad))}. "


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    fl.build()
    rng = np.random.default_rng(616)
    world = rc.scene(2400, 8101)
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
    (root / "matches.txt").write_text("".join(f"{q} {t} {a!r}\n" for q, t, a in rows))
    return dict(root=root, clouds=clouds, rows=rows)


def _run(args, cwd):
    r = subprocess.run([str(HOST / "batch_submap_registration"), *[str(a) for a in args]], cwd=cwd, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _stdout_without_times(r):
    return re.sub(r"(\[TIME\] Avg Tiempo for 2nd Stage \(fine\): )\S+", r"\1T", r.stdout)


def _outputs(r, d):
    return (_stdout_without_times(r),) + tuple((d / name).read_bytes() for name in REPORTS)


def test_map_leaf_0_and_absent_write_identical_files(tree, tmp_path):
    root = tree["root"]
    outs = {}
    for name, extra in (("absent", []), ("chunk only", [256]), ("zero", [256, 0]), ("zero point zero", [256, "0.0"])):
        d = tmp_path / name.replace(" ", "_")
        d.mkdir()
        outs[name] = _outputs(_run([root / "matches.txt", root, 2] + extra, d), d)
    assert outs["absent"] == outs["chunk only"] == outs["zero"] == outs["zero point zero"]
    assert outs["absent"][1].count(b"\n") >= 5 and outs["absent"][2] == b""


def test_map_leaf_02_at_half_window_2_equals_the_checker_at_two_chunk_sizes(tree, tmp_path):
    root, rows = tree["root"], tree["rows"]
    maps = sc.Maps()
    for k, (q, t, a) in enumerate(rows):  # one map per match: the window of its key frame, ascending
        maps.add([(j, sc.IDENTITY if j == t else _relative(t, j)) for j in range(max(0, t - 2), min(N - 1, t + 2) + 1)])
    m = sc.matches([(q, k, a) for k, (q, t, a) in enumerate(rows)])
    exp = vc.expected(tree["clouds"], maps, m, fl.params(**fl.WHOLE), 0.2, threads=THREADS)
    lines = "".join(fl.report_line(exp[k]["T"], fl.tool_guess(float(m["angle_guess"][k]))) for k in range(len(m))
                    if not exp[k]["fitness"] > 1.5)
    assert lines.count("\n") >= 5 and (exp["fitness"] > 1.5).any()      # successes and a failure
    plain = sc.expected(tree["clouds"], maps, m, fl.params(**fl.WHOLE), threads=THREADS)
    assert plain.tobytes() != exp.tobytes()                                # the second grid changes the results
    tg = vc.targets(tree["clouds"], maps, range(len(maps)), 0.2, threads=THREADS)
    assert all(4 * len(t) <= 3 * len(c) for c, t in tg.values())           # frames of one world: the union loses a quarter at least
    outs = {}
    for chunk in ("6", "256"):
        d = tmp_path / f"chunk{chunk}"
        d.mkdir()
        r = _run([root / "matches.txt", root, 2, chunk, 0.2], d)
        assert (d / REPORTS[0]).read_text() == lines, chunk
        assert (d / REPORTS[1]).read_bytes() == b""
        assert _summary(exp["fitness"]) in r.stdout and re.search(r"\[TIME\] Avg Tiempo for 2nd Stage \(fine\): ", r.stdout)
        outs[chunk] = _outputs(r, d)
    assert outs["6"] == outs["256"]
