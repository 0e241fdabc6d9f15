"""CPU: the raw-sweep side of batch_multi_bev_gen's raw_format mode — host/RawSweeps.cpp against numpy
on files of exact, capped, partial-record and empty sizes; the host-only size query of the batched projection; and the
new entry points without a GPU: an error, never a fallback."""
import ctypes as C

import numpy as np
import pytest

import bev_amd
import rawsweeps_lib as rs
from rawsweeps_lib import KITTI, MULRAN, OXFORD


def _bytes(n_floats, seed, extra=b""):
    return np.random.default_rng(seed).standard_normal(n_floats).astype("<f4").tobytes() + extra


@pytest.mark.parametrize("fmt", [MULRAN, OXFORD, KITTI])
def test_readers_equal_numpy(tmp_path, fmt):
    cap = rs.CAP.get(fmt)
    sizes = {"exact": 4 * 5000, "one": 4, "empty": 0, "at_cap": 4 * (cap or 70000), "above_cap": 4 * ((cap or 70000) + 37)}
    files = {k: _bytes(v, i) for i, (k, v) in enumerate(sizes.items())}
    files["partial"] = _bytes(4 * 777, 9, extra=b"\x01\x02\x03\x04\x05\x06\x07")       # 7 bytes of a 778th record
    files["only_partial"] = b"\x00" * 15
    files["partial_above_cap"] = _bytes(4 * ((cap or 70000) + 5) + 3, 10)
    for name, data in files.items():
        path = tmp_path / f"{name}.bin"
        path.write_bytes(data)
        got, want = rs.read(fmt, path), rs.expected(fmt, data)
        assert got is not None, name
        assert got.tobytes() == want.tobytes(), (name, len(got), len(want))
        assert int(rs.lib().rs_returns(fmt, len(data))) == len(want) // 4
    n_above = len(rs.expected(fmt, files["above_cap"])) // 4
    assert n_above == (cap if cap else 70037)             # MulRan / KITTI stop at the cap, Oxford takes the whole file
    # Oxford: the planes are n floats apart, n = size / 16 — plane p of a file with a partial record starts at float p * n
    if fmt == OXFORD:
        data = files["partial"]
        planes = rs.read(fmt, tmp_path / "partial.bin").reshape(4, 777)
        assert planes[2].tobytes() == data[2 * 777 * 4:3 * 777 * 4]
    assert rs.read(fmt, tmp_path / "missing.bin") is None  # unreadable: a failed frame, no data
    assert rs.read(fmt, tmp_path) is None                  # (a directory)


def test_format_names_sensors_and_listing(tmp_path):
    L = rs.lib()
    assert [L.rs_parse_format(n) for n in (b"mulran", b"oxford", b"kitti")] == [MULRAN, OXFORD, KITTI]
    assert [L.rs_parse_format(n) for n in (b"", b"Kitti", b"mulran ", b"pcd")] == [-1] * 4
    HDL_32E, HDL_64E, OS1_64, UNKNOWN = range(4)        # host/Utility.h
    fits = {(f, s) for f in (MULRAN, OXFORD, KITTI, -1) for s in (HDL_32E, HDL_64E, OS1_64, UNKNOWN) if L.rs_fits_sensor(f, s)}
    assert fits == {(MULRAN, OS1_64), (OXFORD, HDL_32E), (KITTI, HDL_64E)}
    for name in ("000010.bin", "000002.bin", "a.pcd", "b.bin.txt", "000001.bin", "noext"):
        (tmp_path / name).write_bytes(b"")
    (tmp_path / "sub.bin").mkdir()                       # (the reference's listing does not look at the entry's type either)
    assert rs.listing(tmp_path, "bin") == [f"{tmp_path}/{n}" for n in ("000001.bin", "000002.bin", "000010.bin", "sub.bin")]
    assert rs.listing(str(tmp_path) + "/", "pcd") == [f"{tmp_path}/a.pcd"]


def test_batch_out_points():
    offs = np.array([5, 5, 105, 1105, 1105], dtype=np.uint64)
    assert bev_amd.project_batch_out_points(0, 4, offs) == 1105      # records sit at their returns' offsets
    assert bev_amd.project_batch_out_points(1, 4, offs) == 1105
    assert bev_amd.project_batch_out_points(2, 4, offs) == 4 * 64 * 2083 == 4 * bev_amd.KITTI_SLOTS
    assert bev_amd.project_batch_out_points(2, 0, offs[:1]) == 0
    assert bev_amd.project_batch_out_points(0, 0, offs[:1]) == 5
    assert bev_amd.project_batch_out_points(3, 4, offs) == 0         # unknown kind
    assert bev_amd.project_batch_out_points(-1, 4, offs) == 0
    assert bev_amd.project_batch_out_points(0, 2, np.array([0, 9, 8], dtype=np.uint64)) == 0   # decreasing
    lib = bev_amd.load_lib()
    assert lib.bev_project_batch_out_points(0, 4, None) == 0
    assert lib.bev_project_batch_out_points(0, -1, offs.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
    assert bev_amd.PROJECT_KITTI_GROUP == 16                         # BEV_PROJECT_KITTI_GROUP of the header
    assert "#define BEV_PROJECT_KITTI_GROUP 16" in (bev_amd.REPO_DIR / "include" / "bev_mi355x.h").read_text()


def test_new_entry_points_fail_without_a_context_or_a_gpu():
    """no context can exist without a GPU (bev_create: BEV_ERR_NO_DEVICE, test_abi.py); what is left of the new calls
    without one is an error status — there is nothing behind them that could compute on the host"""
    lib = bev_amd.load_lib()
    offs = np.array([0, 4], dtype=np.uint64)
    raw = np.zeros(16, np.float32)
    o = offs.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.bev_project_device_resident(None, 0, 1, raw.ctypes.data, o, raw.ctypes.data) == -1
    VP = C.c_void_p * 1
    n = (C.c_uint32 * 1)(4)
    assert lib.bev_process_batch_xyzi(None, 0, 1, VP(raw.ctypes.data), n, VP(raw.ctypes.data), None, None, None) == -1
    import torch

    if not torch.cuda.is_available():
        p = bev_amd.params_for_sensor("OS1_64")
        with pytest.raises(bev_amd.BevError, match="no usable HIP device"):
            bev_amd.BevContext(p, device=0, max_batch=1, max_points=1000)
