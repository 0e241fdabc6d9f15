"""CPU: the scan-to-map search grids sized to the map (bev_set_submap_search_grid) without a GPU: the rule of
the grid's size against a Python restatement and the invariants of the host plan with a grid cap (csrc/bev_submap_reg_plan.h),
checked by the stand-alone tests/submapgridcheck, plain and as a second program under the address and undefined-behaviour
sanitizers; the setter's and the hook's refusals that need no device; the two symbols in the header, the library and the
binding; and the tools' refusals of BEV_SUBMAP_SEARCH_GRID."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bev_amd
import pcd_util
import submap_grid_cases as gc

REPO = Path(__file__).resolve().parent.parent
DIR = Path(__file__).resolve().parent / "submapgridcheck"
HOST = bev_amd.PKG_DIR / "host"
TOOLS = ["batch_submap_registration", "batch_submap_top_part_registration"]
USAGE = " <match_result_text_file> <keyframes_root_dir> <half_window> [<chunk> [<map_leaf>]]\n"
INVALID = -1
SANITIZE = "-fsanitize=address,undefined -fno-omit-frame-pointer"
CAPS = (1, 2, 63, 64, 65, 128, 130, 256, 1000, 1024)


def _build_and_run(program, *args):
    """a fresh build of one of the two programs, its run, and a clean tree"""
    try:
        subprocess.run(["make", "-C", str(DIR), "clean"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        r = subprocess.run(["make", "-C", str(DIR), program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            return r, None
        return r, subprocess.run([str(DIR / program), *args], capture_output=True, text=True, timeout=300)
    finally:
        subprocess.run(["make", "-C", str(DIR), "clean"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _assert_ok(run):
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert [l for l in lines if l.startswith("ok:")] == lines[-1:], run.stdout
    assert lines[-1].startswith("ok: submapgridcheck: 12000 plans, "), lines[-1]
    assert "PLAN" not in run.stdout
    words = lines[-1].split()        # ok: submapgridcheck: P plans, G launch groups, K of them single maps above the cap, W grids ...
    groups, oversize, wide = int(words[4]), int(words[7]), int(words[15])
    assert groups > 12000 and 0 < oversize < groups and wide > 1000


def test_the_rule_of_the_grids_size_equals_its_python_restatement():
    built, run = _build_and_run("submapgridcheck", "dims")
    assert built.returncode == 0, built.stdout
    assert run.returncode == 0, run.stderr
    rows = np.array([l.split() for l in run.stdout.splitlines()], np.int64)
    assert len(rows) == len(CAPS) * (3 * 1024 + 2)
    seen = set()
    for n, D, dim in rows.tolist():
        assert dim == gc.grid_dim(n, D), (n, D, dim)
        seen.add((n, D))
    assert all((k * k + d, D) in seen for D in CAPS for k in (1, 2, 64, 128, 135, 1023, 1024) for d in (-1, 0, 1))
    assert gc.grid_dim(18000, 1024) == 135 and gc.grid_dim(5400, 1024) == 74 and gc.grid_dim(1 << 22, 1024) == 1024


def test_plan_invariants_with_a_grid_cap_over_seeded_random_calls():
    built, run = _build_and_run("submapgridcheck")
    assert built.returncode == 0, built.stdout
    _assert_ok(run)


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", *SANITIZE.split(), "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + (r.stderr.strip().splitlines() or ["gcc failed"])[-1])
    built, run = _build_and_run("submapgridcheck_san")      # a stand-alone host program, run directly
    assert built.returncode == 0, built.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    _assert_ok(run)


def test_the_setter_and_the_hook_refuse_without_a_device():
    lib = bev_amd.load_lib()
    out = np.zeros(4, np.uint32)
    for fine, coarse in ((0, 0), (256, 128), (-1, 0), (0, 1025)):
        assert lib.bev_set_submap_search_grid(None, fine, coarse) == INVALID
    assert lib.bev_debug_get_submap_grid(None, 0, 0, 1, out.ctypes.data) == INVALID
    assert lib.bev_debug_get_submap_grid(None, 1, 0, 0, None) == INVALID
    assert not out.any()
    assert bev_amd.SUBMAP_SEARCH_GRID_MAX == 1024


def test_both_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "bev_mi355x.h").read_text(), flags=re.S)
    lib = bev_amd.load_lib()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(bev_amd.LIB_PATH)], capture_output=True, text=True).stdout
    for name in ("bev_set_submap_search_grid", "bev_debug_get_submap_grid"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in the header"
        assert name in bev_amd.ABI_SYMBOLS and hasattr(lib, name)
        assert re.search(r" T " + name + r"$", exported, flags=re.M), f"{name} is not exported with C linkage"
        assert getattr(lib, name).argtypes is not None
    assert re.search(r"#define\s+BEV_SUBMAP_SEARCH_GRID_MAX\s+1024\b", text)
    assert callable(bev_amd.BevContext.set_submap_search_grid) and callable(bev_amd.BevContext.debug_submap_grid)
    assert lib.bev_abi_version() == 1


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("kf")
    pcd = root / "non_ground_point_cloud"
    pcd.mkdir()
    rng = np.random.default_rng(7)
    for i in range(3):
        pts = np.zeros(5, bev_amd.POINT_DTYPE)
        pts["x"], pts["y"], pts["z"] = rng.uniform(-1, 1, (3, 5)).astype(np.float32)
        pcd_util.write_pcd_binary(pcd / f"{i:06d}.pcd", pts)
    pose = lambda i: ",".join([str(i), repr(0.5 * i), "0.0", "0.0", "0", "0", "0", "1.0", "0.0", "0.0", "0.0", "1.0", "0.0", "0.0", "0.0", "1.0"])
    (root / "keyframe_pose.csv").write_text("\n".join(pose(i) for i in range(3)) + "\n")
    (root / "matches.txt").write_text("0 1 0.0\n2 1 5.0\n")
    return root


@pytest.mark.parametrize("tool", TOOLS)
@pytest.mark.parametrize("text", ["abc", "-1", "2000", "1,2,3", "1025", "256,", ",128", " 256", "256,-1", "1e2", "0x10"])
def test_the_tools_refuse_a_wrong_search_grid_before_any_device_work(tool, text, tree, tmp_path):
    env = dict(os.environ, BEV_SUBMAP_SEARCH_GRID=text)
    r = subprocess.run([str(HOST / tool), str(tree / "matches.txt"), str(tree), "1"], cwd=tmp_path, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    assert r.stdout == ""
    assert r.stderr == f"BEV_SUBMAP_SEARCH_GRID '{text}': expected <fine>[,<coarse>], integers 0 ... 1024\nUsage: {tool}{USAGE}"
    assert not list(tmp_path.iterdir())                     # refused before the reports are created
