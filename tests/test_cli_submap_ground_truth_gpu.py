"""GPU: batch_submap_registration on general poses: the world of ground_truth_cases.py written as a tree of PCD
files and a pose file whose rows are neither quarter turns nor multiples of 0.25 m, so submapwin::relativePose
(host/SubmapWindows.h) meets poses that are not exact in float for the first time.  Every line of the report must equal what
ref64_registration.report gives for T_true = P_map^-1 P_q, to within what the tolerance of the whole setting (8 times float32
against float64 of the plain reference, ground_truth_cases.tol) moves those two numbers and half a unit of the sixth digit
the tool prints.  The pose rows hold float32 values, and the frames and T_true are taken from those rounded rows, so the file
and the truth agree.  The tool wants a pose row for every cloud: the six query clouds follow the seven posed key frames, with
their own poses in their rows (no window reaches them).

batch_submap_top_part_registration is left out: its front end flattens the top part of a cloud and estimates 2-D normals, and
neither keeps this world's zero residual at the true pose."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bev_amd
import ground_truth_cases as gt
import pcd_util
import ref64_registration as ref

pytestmark = pytest.mark.gpu
HOST = Path(bev_amd.PKG_DIR) / "host"


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    S = gt.setup(round_poses=True)
    root = tmp_path_factory.mktemp("kf_ground_truth")
    (root / "non_ground_point_cloud").mkdir()
    for i, c in enumerate(S["clouds"]):
        pcd_util.write_pcd_binary(root / "non_ground_point_cloud" / f"{i:06d}.pcd", c)
    rows = []
    for i, P in enumerate(S["poses"]):
        assert np.array_equal(P, P.astype(np.float32).astype(np.float64))
        rows.append(",".join([str(i)] + [repr(float(v)) for v in P[:3, 3]] + ["0", "0", "0"] + [repr(float(v)) for v in P[:3, :3].reshape(9)]))
    (root / "keyframe_pose.csv").write_text("\n".join(rows) + "\n")
    # the matches whose maps are windows of half width 2 about a key frame: map A about frame 2, map B about frame 4
    picked = [k for k, (_, g, _) in enumerate(S["matches"]) if len(S["maps"][g][1]) == 5]
    gt.precompute(round_poses=True, settings=("whole",), matches=picked)
    lines = [(S["matches"][k][0], S["maps"][S["matches"][k][1]][0], float(S["matches"][k][2])) for k in picked]
    assert [m for _, m, _ in lines] == [2, 2, 4, 4]
    (root / "matches.txt").write_text("".join(f"{q} {m} {a!r}\n" for q, m, a in lines))
    return dict(S=S, root=root, picked=picked)


def _bounds(T, guess, tol):
    """what a change of every entry of T's 3 x 4 by at most tol can move report's two numbers by, to first order: the sum over
    the entries of the larger of the moves by +tol and by -tol"""
    base = np.array(ref.report(T, guess))
    moved = np.zeros(2)
    for i in range(3):
        for j in range(4):
            one = np.zeros(2)
            for sign in (1.0, -1.0):
                U = T.copy()
                U[i, j] += sign * tol
                one = np.maximum(one, np.abs(np.array(ref.report(U, guess)) - base))
            moved += one
    return base, moved


@pytest.mark.parametrize("map_leaf", [None, "0.2"])
def test_the_report_of_general_poses_equals_the_truth(tree, tmp_path, map_leaf):
    S, root, picked = tree["S"], tree["root"], tree["picked"]
    args = [str(root / "matches.txt"), str(root), "2"] + (["256", map_leaf] if map_leaf else [])
    r = subprocess.run([str(HOST / "batch_submap_registration"), *args], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"count_success: {len(picked)}, count_failure: 0" in r.stdout, r.stdout
    lines = (tmp_path / "icp_precision_report_submap.txt").read_text().splitlines()
    assert len(lines) == len(picked), lines
    for line, k in zip(lines, picked):
        got = np.array([float(v) for v in line.split()])
        tol = gt.tol(k, "whole", round_poses=True)
        assert tol <= gt.CAP
        want, moved = _bounds(S["truth"][k], ref.yaw_guess(S["matches"][k][2], 0), tol)
        digit = np.array([0.5 * 10.0 ** (np.floor(np.log10(abs(v))) - 5) if v else 0.0 for v in want])
        print(f"match {k}, map_leaf {map_leaf}: report {got.tolist()}, truth {want.tolist()}, off by {np.abs(got - want).tolist()}, "
              f"bound {(moved + digit).tolist()} (tol {tol:.2e})")
        assert len(got) == 2 and (np.abs(got - want) <= moved + digit).all(), (line, want, moved + digit)
