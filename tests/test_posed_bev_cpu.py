"""CPU: the batched 24-layer / uint8 BEVs under per-frame poses without a GPU — posed_code, the arithmetic of
k_posed_splat, composed on the host by tests/posedcheck against the oracle's transform + rasters; the two entry points in the
library; and batch_posed_bev_gen's argument and pose-file checks, which end the tool before it creates a context."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bev_amd

DIR = Path(__file__).resolve().parent / "posedcheck"
CLI = bev_amd.PKG_DIR / "host" / "batch_posed_bev_gen"
INVALID = -1


def test_posed_code_rasters_equal_the_oracle_composition():
    r = subprocess.run(["make", "-C", str(DIR)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(DIR / "posedcheck")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1]
    # 3 sensors x 2 intervals x 2 clouds x (14 poses + none)
    assert last.startswith("posedcheck ok: 180 cases, "), last
    # ... and 3 sensors x 2 intervals x 2 clouds x 2 general matrices (two entries of raster_world_cases.py's map T)
    assert "; 24 more under general matrices, " in last and not last.endswith(", 0 occupied bytes"), last
    assert "MISMATCH" not in r.stdout


def test_entry_points_are_exported_and_refuse_a_null_context():
    lib = bev_amd.load_lib()
    assert {"bev_posed_bev_device_resident", "bev_posed_bev_batch"} <= set(bev_amd.ABI_SYMBOLS)
    assert hasattr(lib, "bev_posed_bev_device_resident") and hasattr(lib, "bev_posed_bev_batch")
    assert bev_amd.POSED_BEV_MAX_POSES == 64
    assert "#define BEV_POSED_BEV_MAX_POSES 64" in (bev_amd.REPO_DIR / "include" / "bev_mi355x.h").read_text()
    offs = np.array([0, 4], dtype=np.uint64)
    buf = np.zeros(4, dtype=bev_amd.POINT_DTYPE)
    out = np.full(24 * 224 * 224, 0xA5, dtype=np.uint8)
    o = offs.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.bev_posed_bev_device_resident(None, 1, buf.ctypes.data, o, 0, None, out.ctypes.data, out.ctypes.data) == INVALID
    VP = C.c_void_p * 1
    n = (C.c_uint32 * 1)(4)
    assert lib.bev_posed_bev_batch(None, 1, VP(buf.ctypes.data), n, 0, None, VP(out.ctypes.data), VP(out.ctypes.data)) == INVALID
    assert (out == 0xA5).all()


def _run(*args):
    return subprocess.run([str(CLI), *[str(a) for a in args]], capture_output=True, text=True, timeout=60)


def test_tool_usage_line():
    assert CLI.exists(), "host CLI not built"
    for args in ((), ("/nowhere",), ("/nowhere", "HDL_64E")):
        r = _run(*args)
        assert r.returncode == 1 and r.stdout.startswith("Usage: ") and "[poses_file]" in r.stdout.splitlines()[0], args


MALFORMED = {
    "bad_number": ("0 0 0 0\n1.0 2.0 abc 4.0\n", "bad number 'abc'"),
    "trailing_junk_in_a_number": ("1.0 2.0 3.0x 4.0\n", "bad number '3.0x'"),
    "three_fields": ("0 0 0 0\n1 2 3\n", "line 2: 3 fields"),
    "five_fields": ("1 2 3 4 5\n", "line 1: 5 fields"),
    "no_poses": ("# only a comment\n\n   \n", "no poses"),
    "empty_file": ("", "no poses"),
    "too_many": ("".join(f"{i} 0 0 0\n" for i in range(65)), "more than 64 poses"),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_tool_refuses_a_malformed_pose_file_before_it_creates_a_context(tmp_path, case):
    text, why = MALFORMED[case]
    poses = tmp_path / "poses.txt"
    poses.write_text(text)
    (tmp_path / "non_ground_point_cloud").mkdir()
    r = _run(tmp_path, "HDL_64E", poses)
    assert r.returncode == 1, r.stdout + r.stderr
    assert f"pose file {poses}: " in r.stderr and why in r.stderr, r.stderr
    assert "bev_create" not in r.stderr and "HIP" not in r.stderr          # ended before the GPU was asked for
    assert not (tmp_path / "output_posed_bev").exists()                    # ... and before a directory was touched


def test_tool_refuses_an_unknown_sensor_and_an_unreadable_pose_file(tmp_path):
    good = tmp_path / "poses.txt"
    good.write_text("# tx ty tz yaw_deg\n1.5 -2.25 0.125 30\n")
    r = _run(tmp_path, "VLP_16", good)
    assert r.returncode == 1 and "Unknown sensor type VLP_16" in r.stderr
    for missing in (tmp_path / "absent.txt", tmp_path):                    # no such file; a directory
        r = _run(tmp_path, "HDL_64E", missing)
        assert r.returncode == 1 and f"pose file {missing}: can not be read" in r.stderr, r.stderr
    assert not (tmp_path / "output_posed_bev").exists()
