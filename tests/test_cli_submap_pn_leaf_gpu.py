"""GPU: BEV_SUBMAP_PN_LEAF of batch_submap_top_part_registration end to end, on the kind of tree that
test_cli_submap_top_part_registration_gpu.py builds (parts of one world seen from six exact poses).  Unset, empty and 0 write
identical files and lines; 0.5 at half window 2 equals the checker composition (front end's chain, submap_pn_vox_cases.py,
submap_reg_cases.py from the coarse table) through the report arithmetic of fineicp_lib.report_line, at two chunk sizes;
batch_submap_registration, which has no coarse stage, writes the same with and without the variable."""
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
import submap_pn_vox_cases as pv
import submap_reg_cases as sc
import test_cli_submap_top_part_registration_gpu as top

pytestmark = pytest.mark.gpu
HOST = Path(bev_amd.PKG_DIR) / "host"
TOOL = "batch_submap_top_part_registration"
THREADS = min(16, os.cpu_count() or 4)
F32 = np.float32
N = top.N


@pytest.fixture(scope="module", autouse=True)
def _checkers():
    fl.build()
    il.build()
    rl.build()


def _run(tool, args, cwd, pn_leaf=None, expect=0):
    env = {k: v for k, v in os.environ.items() if k != "BEV_SUBMAP_PN_LEAF"}
    if pn_leaf is not None:
        env["BEV_SUBMAP_PN_LEAF"] = pn_leaf
    r = subprocess.run([str(HOST / tool), *[str(a) for a in args]], cwd=cwd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == expect, r.stdout + r.stderr
    return r


def _files(d):
    return {p.name: p.read_bytes() for p in sorted(Path(d).iterdir()) if p.is_file()}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    rng = np.random.default_rng(616)
    world = rc.scene(2400, 8002)
    w = np.c_[world["x"], world["y"], world["z"]].astype(np.float64)
    clouds = []
    for i in range(N):  # frame i sees a part of the world from pose i
        keep = np.sort(rng.permutation(len(world))[:1500])
        local = (w[keep] - top.TRANS[i]) @ top.ROT[i]
        c = world[keep].copy()
        c["x"], c["y"], c["z"] = local[:, 0].astype(F32), local[:, 1].astype(F32), local[:, 2].astype(F32)
        clouds.append(c)
    root = tmp_path_factory.mktemp("kf")
    (root / "non_ground_point_cloud").mkdir()
    for i, c in enumerate(clouds):
        pcd_util.write_pcd_binary(root / "non_ground_point_cloud" / f"{i:06d}.pcd", c)
    (root / "keyframe_pose.csv").write_text("\n".join(top._pose_line(i) for i in range(N)) + "\n")
    rows = []
    for q, t in [(0, 1), (1, 0), (2, 3), (5, 2), (3, 4), (4, 4), (0, 5), (5, 0), (1, 3)]:
        yaw = (top.YAW[q] - top.YAW[t] + 180.0) % 360.0 - 180.0
        rows.append((q, t, float(F32(yaw + rng.uniform(-2, 2)))))
    rows.append((2, 0, 77.0))
    rows.append((0, 1, float(F32(top.YAW[0] - top.YAW[1] + 180.0 + 1.0))))
    (root / "matches.txt").write_text("".join(f"{q} {t} {a!r}\n" for q, t, a in rows))
    return dict(root=root, clouds=clouds, rows=rows)


def test_unset_empty_and_zero_write_identical_files(tree, tmp_path):
    outs = {}
    for name, text in (("unset", None), ("empty", ""), ("zero", "0"), ("zero_point", "0.0")):
        d = tmp_path / name
        d.mkdir()
        r = _run(TOOL, [tree["root"] / "matches.txt", tree["root"], 2], d, pn_leaf=text)
        outs[name] = (top._stdout_without_times(r), _files(d))
    assert outs["unset"][1]["icp_precision_report.txt"].count(b"\n") >= 5
    assert outs["empty"] == outs["unset"] and outs["zero"] == outs["unset"] and outs["zero_point"] == outs["unset"]


def test_half_a_metre_at_half_window_2_equals_the_checker_at_two_chunk_sizes(tree, tmp_path):
    root, rows, clouds = tree["root"], tree["rows"], tree["clouds"]
    leaf = 0.5
    maps = sc.Maps()
    for k, (q, t, a) in enumerate(rows):  # one map per match: the window of its key frame, ascending
        maps.add([(j, sc.IDENTITY if j == t else top._relative(t, j)) for j in range(max(0, t - 2), min(N - 1, t + 2) + 1)])
    m = sc.matches([(q, k, a) for k, (q, t, a) in enumerate(rows)])
    pn = [rl.chain(c) for c in clouds]
    coarse, best = pv.expected(pn, maps, m, leaf, threads=THREADS)
    guesses = [coarse[k, best[k]]["T"].reshape(4, 4).copy() for k in range(len(m))]
    fine = sc.expected(clouds, maps, m, fl.params(**fl.FINE), guesses, threads=THREADS)
    lines = "".join(fl.report_line(fine[k]["T"], guesses[k]) for k in range(len(m)) if not fine[k]["fitness"] > 1.5)
    print(f"coarse states {coarse['state'].tolist()} best {best.tolist()} fine fitness {fine['fitness'].tolist()}")
    assert lines.count("\n") >= 5
    plain = cc.expected(pn, maps, m, threads=THREADS)
    assert plain[0].tobytes() != coarse.tobytes()                          # the thinned maps give other coarse results
    outs = {}
    for chunk in ("6", None):
        d = tmp_path / f"chunk{chunk}"
        d.mkdir()
        r = _run(TOOL, [root / "matches.txt", root, 2] + ([chunk] if chunk else []), d, pn_leaf="0.5")
        assert (d / "icp_precision_report.txt").read_text() == lines, chunk
        assert top._summary(fine["fitness"]) in r.stdout
        assert re.search(r"\[TIME\] Avg Tiempo for 1st Stage \(coarse\): ", r.stdout)
        outs[chunk] = (top._stdout_without_times(r), _files(d))
    assert outs["6"] == outs[None]


def test_the_whole_tool_ignores_the_variable(tree, tmp_path):
    outs = {}
    for name, text in (("unset", None), ("set", "0.5"), ("bad", "nan")):
        d = tmp_path / name
        d.mkdir()
        r = _run("batch_submap_registration", [tree["root"] / "matches.txt", tree["root"], 2], d, pn_leaf=text)
        outs[name] = (top._stdout_without_times(r), _files(d))
    assert outs["unset"][1]["icp_precision_report_submap.txt"].count(b"\n") >= 5
    assert outs["set"] == outs["unset"] and outs["bad"] == outs["unset"]
