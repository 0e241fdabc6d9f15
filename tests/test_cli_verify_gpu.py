"""GPU: batch_verified_registration (the whole tool's chain against windows, then bev_submap_verify_registration_device_resident per
chunk) end to end on test_cli_submap_registration_gpu.py's tree of PCD files: both files it writes equal what
the binding gives for the same matches, at half windows 0 and 2 and at two chunk sizes; the accepted list is a match list the
registration tools read; wrong guesses are rejected by their overlap alone and still listed; the refusals fire before any work."""
import math
import re
import subprocess

import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import reg_cases as rc
import submap_reg_cases as sc
import test_cli_submap_registration_gpu as base
from bev_amd import ICP_RESULT_DTYPE, VERIFY_RESULT_DTYPE, verify_params
from test_cli_submap_registration_gpu import tree  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
F32 = np.float32
THRESHOLD = 0.1
HEADER = ("query,match,fitness,converged,n_query,n_target,query_within,target_within,overlap,accepted,"
          "t00,t01,t02,t03,t10,t11,t12,t13,t20,t21,t22,t23\n")


@pytest.fixture(scope="module")
def matches_file(tree):
    """the tree's matches and, behind them, wrong guesses: true pairs started 40 ... 180 degrees off"""
    rows = list(tree["rows"])
    for k, (q, t) in enumerate([(0, 1), (2, 3), (3, 4), (5, 2), (1, 0)]):
        yaw = (base.YAW[q] - base.YAW[t] + 180.0) % 360.0 - 180.0
        rows.append((q, t, float(F32(yaw + 40.0 + 35.0 * k))))
    path = tree["root"] / "matches_verify.txt"
    path.write_text("".join(f"{q} {t} {a!r}\n" for q, t, a in rows))
    return path, rows


def _binding(tree, rows, half):
    """(fine ICP_RESULT_DTYPE, verify VERIFY_RESULT_DTYPE) of the rows through the device-resident calls"""
    import torch

    clouds = tree["clouds"]
    maps = sc.Maps()
    for q, t, a in rows:
        maps.add([(j, sc.IDENTITY if j == t else base._relative(t, j)) for j in range(max(0, t - half), min(base.N - 1, t + half) + 1)])
    m = sc.matches([(q, k, a) for k, (q, t, a) in enumerate(rows)])
    ctx = bev_amd.BevContext(bev_amd.params_for_sensor("HDL_64E"), device=0, max_batch=2, max_points=4096)
    try:
        offs = np.r_[0, np.cumsum([len(c) for c in clouds])].astype(np.uint64)
        dev = torch.device("cuda:0")
        d_clouds = torch.from_numpy(rc.packed(clouds).view(np.uint8).reshape(-1).copy()).to(dev)
        d_res = torch.zeros(len(m) * ICP_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_ver = torch.zeros(len(m) * VERIFY_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.submap_voxel_registration_device(len(clouds), d_clouds.data_ptr(), offs, *maps.arrays(), m, d_res.data_ptr(), 0.0,
                                             params=fl.params(**fl.WHOLE))
        ctx.submap_verify_registration_device(len(clouds), d_clouds.data_ptr(), offs, *maps.arrays(), m, d_res.data_ptr(),
                                              d_ver.data_ptr(), 0.0, verify_params((THRESHOLD,)))
        ctx.synchronize()
        return d_res.cpu().numpy().view(ICP_RESULT_DTYPE).copy(), d_ver.cpu().numpy().view(VERIFY_RESULT_DTYPE).copy()
    finally:
        ctx.close()


def _files(rows, fine, ver, pair, min_overlap):
    """(verification_detail.csv, verified_match_result.txt, accepted flags, rows rejected by their overlap alone, overlaps)"""
    csv, lst, accepted, by_overlap, overlaps = HEADER, "", [], [], []
    for k, (q, t, _) in enumerate(rows):
        r, v = fine[k], ver[k]
        fwd = int(v["query_within"][0]) / int(v["n_query"]) if v["n_query"] and v["query_within"][0] else 0.0
        rev = int(v["target_within"][0]) / int(v["n_target"]) if v["n_target"] and v["target_within"][0] else 0.0
        overlap = min(fwd, rev) if pair else fwd
        fit_ok = bool(r["converged"]) and bool(r["fitness"] <= 1.5)
        ok = fit_ok and overlap >= float(F32(min_overlap))
        accepted.append(ok)
        overlaps.append(overlap)
        if fit_ok and not ok:
            by_overlap.append(k)
        csv += ("%d,%d,%.17g,%d,%d,%d,%d,%d,%.17g,%d" % (q, t, r["fitness"], r["converged"], v["n_query"], v["n_target"],
                                                         v["query_within"][0], v["target_within"][0], overlap, ok))
        csv += "".join(",%.9g" % float(x) for x in r["T"][:12]) + "\n"
        if ok:
            yaw = F32(math.atan2(float(r["T"][4]), float(r["T"][0])) * 180.0 / 3.14159265358979323846)
            lst += "%d %d %.9g\n" % (q, t, float(yaw))
    return csv, lst, accepted, by_overlap, overlaps


def _run(args, cwd, env=None, ok=True):
    import os

    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([str(base.HOST / "batch_verified_registration"), *[str(a) for a in args]], cwd=cwd, capture_output=True, text=True,
                       timeout=600, env=e)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


# Every frame sees 1500 of the world's 2400 points, so two frames share about five eighths of theirs: a frame against a frame
# explains 0.62 ... 0.65 of either side at the true motion, a frame against a window of five nearly all of itself.
@pytest.mark.parametrize("half,min_overlap", [(0, 0.4), (2, 0.4), (0, 0.7)])
def test_tool_writes_what_the_binding_gives(tree, matches_file, tmp_path, half, min_overlap):
    path, rows = matches_file
    fine, ver = _binding(tree, rows, half)
    csv, lst, accepted, by_overlap, overlaps = _files(rows, fine, ver, half == 0, min_overlap)
    for k in range(len(rows)):
        print(rows[k], float(fine[k]["fitness"]), int(fine[k]["converged"]), ver[k], accepted[k])
    env = {"BEV_VERIFY_THRESHOLD": str(THRESHOLD), "BEV_VERIFY_MIN_OVERLAP": str(min_overlap)}
    outs = []
    for chunk in ("6", None):
        d = tmp_path / f"chunk{chunk}"
        d.mkdir()
        r = _run([path, tree["root"], half] + ([chunk] if chunk else []), d, env)
        assert (d / "verification_detail.csv").read_text() == csv, chunk
        assert (d / "verified_match_result.txt").read_text() == lst, chunk
        assert "count_success: " in r.stdout
        outs.append(d)
    # every input match has its row; accepted and rejected both occur; every wrong guess is below the overlap and rejected
    assert csv.count("\n") == len(rows) + 1 and any(accepted) and not all(accepted)
    wrong = [len(tree["rows"]) - 1] + list(range(len(tree["rows"]), len(rows)))
    assert all(overlaps[k] < 0.05 and not accepted[k] for k in wrong)
    if min_overlap > 0.5:
        # half-overlapping views registered correctly: converged, a fitness the tools pass, rejected by their overlap alone
        assert len(by_overlap) >= 5 and all(fine[k]["fitness"] < 0.5 and 0.55 < overlaps[k] < 0.7 for k in by_overlap)
        assert accepted[rows.index(tree["rows"][5])] and tree["rows"][5][:2] == (4, 4)  # a frame against itself stays
    else:
        assert not by_overlap and sum(accepted) == len(rows) - len(wrong)
    # the accepted list is a match list: the whole tool's chain reads it back and registers exactly those matches
    back = tmp_path / "back"
    back.mkdir()
    r = subprocess.run([str(base.HOST / "batch_submap_registration"), str(outs[0] / "verified_match_result.txt"), str(tree["root"]), str(half)],
                       cwd=back, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    n_ok = sum(accepted)
    counts = re.search(r"count_success: (\d+), count_failure: (\d+)", r.stdout)
    assert counts and int(counts.group(1)) + int(counts.group(2)) == n_ok and n_ok >= 1


@pytest.mark.parametrize("env", [{"BEV_VERIFY_THRESHOLD": "0"}, {"BEV_VERIFY_THRESHOLD": "-1"}, {"BEV_VERIFY_THRESHOLD": "nan"},
                                 {"BEV_VERIFY_THRESHOLD": "inf"}, {"BEV_VERIFY_THRESHOLD": "0.5x"}, {"BEV_VERIFY_MIN_OVERLAP": "0"},
                                 {"BEV_VERIFY_MIN_OVERLAP": "1.01"}, {"BEV_VERIFY_MIN_OVERLAP": "nan"}, {"BEV_VERIFY_MIN_OVERLAP": "x"}])
def test_refusals_before_any_work(tree, matches_file, tmp_path, env):
    r = _run([matches_file[0], tree["root"], 0], tmp_path, env, ok=False)
    assert r.returncode == 1 and "Usage: batch_verified_registration" in r.stderr and "placeholders" in r.stderr
    assert not (tmp_path / "verification_detail.csv").exists() and not (tmp_path / "verified_match_result.txt").exists()


def test_too_few_arguments(tmp_path):
    r = subprocess.run([str(base.HOST / "batch_verified_registration"), "a", "b"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage: batch_verified_registration" in r.stderr
