"""CPU: scan-to-map registration without a GPU — the invariants of the host plan (csrc/bev_submap_reg_plan.h)
over seeded random calls, checked by the stand-alone tests/submapregcheck, plain and as a second program under the address
and undefined-behaviour sanitizers; the two entry points in the library and the binding; the checker composition
(submap_reg_cases.py) on the mirror-tie map, which must depend on the entry order; and the tool's argument checks."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import submap_reg_cases as sc

DIR = Path(__file__).resolve().parent / "submapregcheck"
CLI = bev_amd.PKG_DIR / "host" / "batch_submap_registration"
INVALID = -1
SANITIZE = "-fsanitize=address,undefined -fno-omit-frame-pointer"


def _build_and_run(program):
    """a fresh build of one of the two programs, its run, and a clean tree"""
    try:
        subprocess.run(["make", "-C", str(DIR), "clean"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        r = subprocess.run(["make", "-C", str(DIR), program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            return r, None
        return r, subprocess.run([str(DIR / program)], capture_output=True, text=True, timeout=300)
    finally:
        subprocess.run(["make", "-C", str(DIR), "clean"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _assert_ok(run):
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert [l for l in lines if l.startswith("ok:")] == lines[-1:], run.stdout
    assert lines[-1].startswith("ok: submapregcheck: 300 plans, "), lines[-1]
    assert "PLAN" not in run.stdout
    words = lines[-1].split()                               # ok: submapregcheck: P plans, G launch groups, K of them ...
    groups, oversize = int(words[4]), int(words[7])
    assert groups > 300 and 0 < oversize < groups          # several groups per plan; single maps above the cap among them


def test_plan_invariants_over_seeded_random_calls():
    built, run = _build_and_run("submapregcheck")
    assert built.returncode == 0, built.stdout
    _assert_ok(run)


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", *SANITIZE.split(), "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + (r.stderr.strip().splitlines() or ["gcc failed"])[-1])
    built, run = _build_and_run("submapregcheck_san")      # a stand-alone host program, run directly
    assert built.returncode == 0, built.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    _assert_ok(run)


def test_entry_points_are_exported_and_refuse_a_null_context():
    lib = bev_amd.load_lib()
    names = {"bev_submap_registration_device_resident", "bev_submap_registration_batch"}
    assert names <= set(bev_amd.ABI_SYMBOLS) and all(hasattr(lib, n) for n in names)
    assert hasattr(bev_amd.BevContext, "submap_registration_device") and hasattr(bev_amd.BevContext, "submap_registration_batch")
    assert lib.bev_abi_version() == 1                      # the change only adds
    assert bev_amd.SUBMAP_REG_MAX_TARGET == sc.REG_MAX_TARGET
    offs = np.array([0, 4], dtype=np.uint64)
    moffs = np.array([0, 1], dtype=np.uint64)
    eframe = np.zeros(1, dtype=np.int32)
    epose = sc.IDENTITY.reshape(1, 12).copy()
    buf = np.zeros(4, dtype=bev_amd.POINT_DTYPE)
    m = sc.matches([(0, 0, 0.0)])
    out = np.full(bev_amd.ICP_RESULT_DTYPE.itemsize, 0xA5, dtype=np.uint8)
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.bev_submap_registration_device_resident(None, 1, buf.ctypes.data, u64(offs), 0.2, 1, u64(moffs), eframe.ctypes.data,
                                                       epose.ctypes.data, 1, m.ctypes.data, None, None, None,
                                                       out.ctypes.data) == INVALID
    VP = C.c_void_p * 1
    n = (C.c_uint32 * 1)(4)
    assert lib.bev_submap_registration_batch(None, 1, VP(buf.ctypes.data), n, 0.2, 1, u64(moffs), eframe.ctypes.data,
                                             epose.ctypes.data, 1, m.ctypes.data, None, out.ctypes.data) == INVALID
    assert (out == 0xA5).all()


def test_the_checker_composition_depends_on_the_entry_order_of_a_mirror_tie():
    fl.build()
    clouds, maps, m = sc.mirror_tie()
    vox = fl.voxel_irct(clouds[0], 0.2)
    assert len(vox) == len(clouds[0])                      # one point per voxel: A is its own voxel cloud
    t0, t1 = sc.target({0: vox}, maps.entries(0)), sc.target({0: vox}, maps.entries(1))
    assert len(t0) == 2 * len(vox) and t0[: len(vox)].tobytes() == t1[len(vox):].tobytes()
    # the tie itself: every source point is exactly as far from both images of its own point, and nothing is nearer
    src = fl.voxel_irct(clouds[1], 0.2)
    xyz = np.c_[src["x"], src["y"], src["z"]]
    i0, d0 = fl.nn(t0, xyz)
    i1, d1 = fl.nn(t1, xyz)
    assert (i0 < len(vox)).all() and (i1 < len(vox)).all() and d0.tobytes() == d1.tobytes()
    assert (d0 == np.float32(0.25 + 1.0 / 64.0)).all()
    assert not np.array_equal(t0[i0]["x"], t1[i1]["x"])    # the lowest index is the other image
    for prm in (fl.params(**fl.WHOLE), fl.params(**fl.FINE)):
        exp = sc.expected(clouds, maps, m, prm, threads=2)
        assert exp[0]["state"] != bev_amd.ICP_NO_CORRESPONDENCES and exp[1]["state"] != bev_amd.ICP_NO_CORRESPONDENCES
        assert exp[0].tobytes() != exp[1].tobytes()
        assert exp[0]["T"][3] > 0.25 and exp[1]["T"][3] < -0.25   # each order pulls the source towards its first entry


def _run(*args, cwd=None):
    return subprocess.run([str(CLI), *[str(a) for a in args]], capture_output=True, text=True, timeout=60, cwd=cwd)


def test_tool_refuses_wrong_arguments_before_it_creates_a_context(tmp_path):
    assert CLI.exists(), "host CLI not built"
    for args in ((), ("m.txt",), ("m.txt", "/nowhere")):
        r = _run(*args, cwd=tmp_path)
        assert r.returncode == 1 and r.stderr.startswith("Usage: batch_submap_registration <match_result_text_file> "), args
    (tmp_path / "non_ground_point_cloud").mkdir()
    (tmp_path / "m.txt").write_text("0 0 0.0\n")
    for window in ("-1", "two", "2x", ""):
        r = _run(tmp_path / "m.txt", tmp_path, window, cwd=tmp_path)
        assert r.returncode == 1 and f"half_window '{window}': expected an integer >= 0" in r.stderr, (window, r.stderr)
    r = _run(tmp_path / "m.txt", tmp_path, 2, 5, cwd=tmp_path)
    assert r.returncode == 1 and "chunk '5': expected an integer >= 2 * half_window + 2" in r.stderr
    r = _run(tmp_path / "m.txt", tmp_path, 1, cwd=tmp_path)                    # no pose file
    assert r.returncode == 1 and "keyframe_pose.csv" in r.stderr
    (tmp_path / "keyframe_pose.csv").write_text(",".join(["0", "1.0", "2.0", "0.0", "0", "0", "0", "1", "0", "0", "0", "1", "0", "0", "0", "1"]) + "\n")
    (tmp_path / "m.txt").write_text("0 3 0.0\n")
    r = _run(tmp_path / "m.txt", tmp_path, 1, cwd=tmp_path)                    # an index outside the (zero) clouds
    assert r.returncode == 1 and "outside the 0 clouds" in r.stderr
    assert "bev_create" not in r.stderr and "HIP" not in r.stderr
