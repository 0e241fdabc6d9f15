"""CPU: the BEVs of submaps without a GPU — the plan of a call (csrc/bev_submap_plan.h) built, checked and run
on the host by tests/submapcheck against the oracle's rasters of the concatenated moved clouds, plain and under the address and
undefined-behaviour sanitizers; the two entry points in the library; and batch_submap_bev_gen's argument and pose-file checks,
which end the tool before it creates a context."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bev_amd

DIR = Path(__file__).resolve().parent / "submapcheck"
CLI = bev_amd.PKG_DIR / "host" / "batch_submap_bev_gen"
INVALID = -1
SANITIZE = "-fsanitize=address,undefined -fno-omit-frame-pointer"


def _build_and_run(*make_args):
    """a fresh build of the program (the object files carry the flags of the build before), its run, and a clean tree"""
    try:
        subprocess.run(["make", "-C", str(DIR), "clean"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        r = subprocess.run(["make", "-C", str(DIR), *make_args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            return r, None
        return r, subprocess.run([str(DIR / "submapcheck")], capture_output=True, text=True, timeout=300)
    finally:
        subprocess.run(["make", "-C", str(DIR), "clean"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _assert_ok(run):
    assert run.returncode == 0, run.stdout + run.stderr
    last = run.stdout.strip().splitlines()[-1]
    # (7 + 5 + 0 + 3 maps) x caps of 1, 3 and "all" x 2 intervals; (7 + 3 + 1) + (5 + 2 + 1) + 0 + (3 + 1 + 1) groups x 2
    assert last.startswith("submapcheck ok: 90 map images in 48 launch groups, "), last
    # the scenario under general matrices: 4 maps x 3 caps x 2 intervals; (4 + 2 + 1) groups x 2
    assert "; under general matrices 24 more in 14, " in last and not last.endswith(", 0"), last
    assert "MISMATCH" not in run.stdout and "PLAN" not in run.stdout


def test_plans_run_on_the_host_equal_the_oracle_composition():
    built, run = _build_and_run()
    assert built.returncode == 0, built.stdout
    _assert_ok(run)


def test_frame_table_rows_closing_row_and_the_limit_of_a_launch():
    """bevsub::frame_table, from offsets alone: frames of 0, 1, 1023, 1024, 1025 records and an empty table; the closing row's
    blk0 is the sum of ceil(n / 1024) and the longest frame is reported; 511 frames of 0xffffffff records (2143289344
    workgroups) are accepted, 512 (2^31) are refused, and so is one workgroup past 2^31 - 1"""
    built, run = _build_and_run()
    assert built.returncode == 0, built.stdout
    assert run.returncode == 0, run.stdout + run.stderr
    assert "frame tables: 11 checked, 0 failed checks" in run.stdout.splitlines(), run.stdout
    assert "PLAN frame table" not in run.stdout


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", *SANITIZE.split(), "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + (r.stderr.strip().splitlines() or ["gcc failed"])[-1])
    built, run = _build_and_run(f"SANITIZE={SANITIZE}")
    assert built.returncode == 0, built.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    _assert_ok(run)


def test_entry_points_are_exported_and_refuse_a_null_context():
    lib = bev_amd.load_lib()
    assert {"bev_submap_bev_device_resident", "bev_submap_bev_batch"} <= set(bev_amd.ABI_SYMBOLS)
    assert hasattr(lib, "bev_submap_bev_device_resident") and hasattr(lib, "bev_submap_bev_batch")
    assert bev_amd.SUBMAP_MAX_ENTRIES == 1 << 20
    assert "#define BEV_SUBMAP_MAX_ENTRIES (1u << 20)" in (bev_amd.REPO_DIR / "include" / "bev_mi355x.h").read_text()
    assert hasattr(bev_amd.BevContext, "submap_bev_device") and hasattr(bev_amd.BevContext, "submap_bev_batch")
    offs = np.array([0, 4], dtype=np.uint64)
    moffs = np.array([0, 1], dtype=np.uint64)
    eframe = np.zeros(1, dtype=np.int32)
    epose = np.eye(3, 4, dtype=np.float32).reshape(1, 12)
    buf = np.zeros(4, dtype=bev_amd.POINT_DTYPE)
    out = np.full(24 * 224 * 224, 0xA5, dtype=np.uint8)
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.bev_submap_bev_device_resident(None, 1, buf.ctypes.data, u64(offs), 1, u64(moffs), eframe.ctypes.data,
                                              epose.ctypes.data, out.ctypes.data, out.ctypes.data) == INVALID
    VP = C.c_void_p * 1
    n = (C.c_uint32 * 1)(4)
    assert lib.bev_submap_bev_batch(None, 1, VP(buf.ctypes.data), n, 1, u64(moffs), eframe.ctypes.data, epose.ctypes.data,
                                    VP(out.ctypes.data), VP(out.ctypes.data)) == INVALID
    assert (out == 0xA5).all()


def _run(*args):
    return subprocess.run([str(CLI), *[str(a) for a in args]], capture_output=True, text=True, timeout=60)


def test_tool_usage_line():
    assert CLI.exists(), "host CLI not built"
    for args in ((), ("/nowhere",), ("/nowhere", "HDL_64E")):
        r = _run(*args)
        assert r.returncode == 1 and r.stdout.startswith("Usage: ") and "[half_window] [stride]" in r.stdout.splitlines()[0], args
        assert "float" in r.stdout and "UTM" in r.stdout          # the inherited limit on large coordinates is stated


def _pose_line(i):
    return ",".join([str(i), "1.0", "2.0", "0.0", "0", "0", "0"] + ["1", "0", "0", "0", "1", "0", "0", "0", "1"])


def _no_trace(root, r):
    assert "bev_create" not in r.stderr and "HIP" not in r.stderr          # ended before the GPU was asked for
    assert not (root / "output_submap_bev").exists()                       # ... and before a directory was touched


def test_tool_refuses_wrong_arguments_before_it_creates_a_context(tmp_path):
    (tmp_path / "non_ground_point_cloud").mkdir()
    (tmp_path / "keyframe_pose.csv").write_text(_pose_line(0) + "\n")
    r = _run(tmp_path, "VLP_16", 2)
    assert r.returncode == 1 and "Unknown sensor type VLP_16" in r.stderr
    _no_trace(tmp_path, r)
    for window in ("-1", "two", "2x", ""):
        r = _run(tmp_path, "HDL_64E", window)
        assert r.returncode == 1 and f"half_window '{window}': expected an integer >= 0" in r.stderr, (window, r.stderr)
        _no_trace(tmp_path, r)
    for stride in ("0", "-3", "x", "1.5"):
        r = _run(tmp_path, "HDL_64E", 2, stride)
        assert r.returncode == 1 and f"stride '{stride}': expected an integer >= 1" in r.stderr, (stride, r.stderr)
        _no_trace(tmp_path, r)


def test_tool_refuses_an_unreadable_or_short_pose_file(tmp_path):
    clouds = tmp_path / "non_ground_point_cloud"
    clouds.mkdir()
    r = _run(tmp_path, "HDL_64E", 1)                                       # no pose file
    assert r.returncode == 1 and f"pose file {tmp_path}/keyframe_pose.csv: can not be read" in r.stderr, r.stderr
    _no_trace(tmp_path, r)
    for i in range(3):
        (clouds / f"{i:06d}.pcd").write_text("placeholder\n")
    (tmp_path / "keyframe_pose.csv").write_text(_pose_line(0) + "\n" + _pose_line(1) + "\n")
    r = _run(tmp_path, "HDL_64E", 1)
    assert r.returncode == 1 and "keyframe_pose.csv: 2 rows for 3 clouds" in r.stderr, r.stderr
    _no_trace(tmp_path, r)
