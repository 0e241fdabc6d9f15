"""CPU: what the four batch registration tools refuse before they touch a GPU — exit status 1, the message on stderr, nothing
on stdout.  batch_top_part_registration / batch_whole_registration (host/batch_registration_main.cpp) and
batch_submap_registration / batch_submap_top_part_registration (host/batch_submap_registration_main.cpp) on trees of three tiny
clouds."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bev_amd
import pcd_util

HOST = Path(bev_amd.PKG_DIR) / "host"
FRAME_TOOLS = ["batch_top_part_registration", "batch_whole_registration"]
SUBMAP_TOOLS = ["batch_submap_registration", "batch_submap_top_part_registration"]
SUBMAP_USAGE = " <match_result_text_file> <keyframes_root_dir> <half_window> [<chunk> [<map_leaf>]]\n"
N = 3


def _pose_line(i):
    return ",".join([str(i), repr(0.5 * i), "0.0", "0.0", "0", "0", "0", "1.0", "0.0", "0.0", "0.0", "1.0", "0.0", "0.0", "0.0", "1.0"])


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("kf")
    pcd = root / "non_ground_point_cloud"
    pcd.mkdir()
    rng = np.random.default_rng(7)
    for i in range(N):
        pts = np.zeros(5, bev_amd.POINT_DTYPE)
        pts["x"], pts["y"], pts["z"] = rng.uniform(-1, 1, (3, 5)).astype(np.float32)
        pcd_util.write_pcd_binary(pcd / f"{i:06d}.pcd", pts)
    (root / "keyframe_pose.csv").write_text("\n".join(_pose_line(i) for i in range(N)) + "\n")
    (root / "matches.txt").write_text("0 1 0.0\n2 1 5.0\n")
    return root


def _refused(tool, args, cwd):
    r = subprocess.run([str(HOST / tool), *[str(a) for a in args]], cwd=cwd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    assert r.stdout == ""
    return r.stderr


@pytest.mark.parametrize("tool", FRAME_TOOLS)
def test_frame_tools_refuse(tool, tree, tmp_path):
    pcd = tree / "non_ground_point_cloud"
    usage = f"Usage: {tool} <match_list> <pcd_dir> [max_frames]\n"
    assert _refused(tool, [], tmp_path) == usage
    assert _refused(tool, [tree / "matches.txt"], tmp_path) == usage
    assert _refused(tool, [tree / "matches.txt", pcd, 1], tmp_path) == "max_frames must be at least 2\n"
    missing = tree / "no_such_list.txt"
    assert _refused(tool, [missing, pcd], tmp_path) == f"Failed to open file: {missing}\n"


@pytest.mark.parametrize("tool", SUBMAP_TOOLS)
def test_submap_tools_refuse_wrong_arguments(tool, tree, tmp_path):
    usage = "Usage: " + tool + SUBMAP_USAGE
    m = tree / "matches.txt"
    assert _refused(tool, [], tmp_path) == usage
    assert _refused(tool, [m, tree], tmp_path) == usage
    for half in ("-1", "x"):
        assert _refused(tool, [m, tree, half], tmp_path) == f"half_window '{half}': expected an integer >= 0\n"
    for half, chunk in ((0, 1), (1, 3), (3, 7)):
        assert _refused(tool, [m, tree, half, chunk], tmp_path) == f"chunk '{chunk}': expected an integer >= 2 * half_window + 2\n"
    for leaf in ("-1", "nan", "0.2x"):
        assert _refused(tool, [m, tree, 1, 4, leaf], tmp_path) == f"map_leaf '{leaf}': expected a finite number >= 0\n" + usage


@pytest.mark.parametrize("tool", SUBMAP_TOOLS)
def test_submap_tools_refuse_wrong_files(tool, tree, tmp_path):
    missing = tree / "no_such_list.txt"
    assert _refused(tool, [missing, tree, 1], tmp_path) == f"Failed to open file: {missing}\n"
    # a pose file with fewer rows than clouds (the reader's own line goes to stderr too: stdout stays empty)
    short = tmp_path / "short"
    (short / "non_ground_point_cloud").mkdir(parents=True)
    for f in (tree / "non_ground_point_cloud").iterdir():
        (short / "non_ground_point_cloud" / f.name).write_bytes(f.read_bytes())
    (short / "keyframe_pose.csv").write_text("\n".join(_pose_line(i) for i in range(N - 1)) + "\n")
    err = _refused(tool, [tree / "matches.txt", short, 1], tmp_path)
    assert err.endswith(f"pose file {short}/keyframe_pose.csv: can not be read, or fewer rows than clouds\n")
    (short / "keyframe_pose.csv").unlink()
    err = _refused(tool, [tree / "matches.txt", short, 1], tmp_path)
    assert err.endswith(f"pose file {short}/keyframe_pose.csv: can not be read, or fewer rows than clouds\n")
    # a match outside the files, either side and either end
    for q, t in ((0, N), (N, 0), (-1, 1), (1, -1)):
        (tmp_path / "outside.txt").write_text(f"0 1 0.0\n{q} {t} 1.0\n")
        err = _refused(tool, [tmp_path / "outside.txt", tree, 1], tmp_path)
        assert err.endswith(f"match {q} {t}: outside the {N} clouds\n")
