"""CPU: the pair calls' search grids sized to the cloud (bev_set_pair_search_grid) without a GPU: the two symbols
in the header, the library and the binding; the setter's and the hook's refusals that need no device; the tools' refusals of
BEV_PAIR_SEARCH_GRID; and the byte model and the build groups of csrc/bev_pair_grid_plan.h, printed by the stand-alone
tests/pairgridcheck (plain, and as a second program under the address and undefined-behaviour sanitizers) over seeded target
counts and capacities, against a Python restatement."""
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
DIR = Path(__file__).resolve().parent / "pairgridcheck"
HOST = bev_amd.PKG_DIR / "host"
TOOLS = ["batch_top_part_registration", "batch_whole_registration"]
USAGE = " <match_list> <pcd_dir> [max_frames]\n"
INVALID = -1
SANITIZE = "-fsanitize=address,undefined -fno-omit-frame-pointer"
GROUP, PART_POINTS, PARTS, SCAN_TILE = 256, 2048, 256, 4096   # bevpair::kBuildGroup, kPartPoints; bevsubreg::kGridParts, kGridScanTile


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


def model(targets: int, capacity: int, D: int):
    """bevpair::layout, ::groups and ::cell0 restated: the row tests/pairgridcheck prints behind (targets, capacity, D)"""
    if D == 0 or targets == 0:
        return [0] * 15
    cells = gc.grid_cells(capacity, D)
    words = cells + 1                                       # a target's offsets: 4 (cells + 1) bytes
    group = min(targets, GROUP)
    n_groups = -(-targets // group)
    return [cells, words, group, 4 * words * targets, 4 * words * group, group * PARTS * 16, group * 256 * 4, 32 * targets,
            16 * targets, 8 * targets, min(max(-(-capacity // PART_POINTS), 1), PARTS), -(-cells // SCAN_TILE), n_groups,
            targets - (n_groups - 1) * group, ((targets - 1) % group) * words]


def _assert_model(run, layouts):
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert "PLAN" not in run.stdout
    assert re.fullmatch(rf"ok: pairgridcheck: {layouts} layouts, \d+ build groups", lines[-1]), lines[-1]
    rows = np.array([l.split() for l in lines[:-1]], np.int64)
    assert len(rows) == layouts
    for row in rows.tolist():
        assert row[3:] == model(*row[:3]), (row, model(*row[:3]))
    wide = rows[(rows[:, 2] > 0) & (rows[:, 0] > 0)]
    assert len(wide) > layouts // 2 and (wide[:, 15] > 1).sum() > 100 and (rows[:, 2] == 0).sum() > 100
    assert (wide[:, 5] * (PARTS * 16 + 256 * 4) == wide[:, 8] + wide[:, 9]).all()       # 5 KiB per slot of a build group


def test_the_byte_model_and_the_build_groups_equal_their_python_restatement():
    built, run = _build_and_run("pairgridcheck")
    assert built.returncode == 0, built.stdout
    _assert_model(run, 4000)
    assert model(1000, 130000, 1024)[4] == 4 * (361 * 361 + 1) * 256                    # a group's counters, HDL_64E sweeps
    assert model(5, 18000, 256)[0] == 135 * 135 and model(5, 5400, 256)[0] == 74 * 74
    assert model(7, 18000, 0) == [0] * 15                                               # nothing at D = 0


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", *SANITIZE.split(), "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + (r.stderr.strip().splitlines() or ["gcc failed"])[-1])
    built, run = _build_and_run("pairgridcheck_san", "1500")   # a stand-alone host program, run directly
    assert built.returncode == 0, built.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    _assert_model(run, 1500)


def test_the_setter_and_the_hook_refuse_without_a_device():
    lib = bev_amd.load_lib()
    out = np.zeros(4, np.uint32)
    for fine, coarse in ((0, 0), (256, 128), (-1, 0), (0, 1025), (1025, -1)):
        assert lib.bev_set_pair_search_grid(None, fine, coarse) == INVALID
    assert lib.bev_debug_get_pair_grid(None, 0, 0, 1, out.ctypes.data) == INVALID
    assert lib.bev_debug_get_pair_grid(None, 1, 0, 0, None) == INVALID
    assert not out.any()
    assert bev_amd.PAIR_SEARCH_GRID_MAX == 1024


def test_both_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "bev_mi355x.h").read_text(), flags=re.S)
    lib = bev_amd.load_lib()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(bev_amd.LIB_PATH)], capture_output=True, text=True).stdout
    for name in ("bev_set_pair_search_grid", "bev_debug_get_pair_grid"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in the header"
        assert name in bev_amd.ABI_SYMBOLS and hasattr(lib, name)
        assert re.search(r" T " + name + r"$", exported, flags=re.M), f"{name} is not exported with C linkage"
        assert getattr(lib, name).argtypes is not None
    assert re.search(r"#define\s+BEV_PAIR_SEARCH_GRID_MAX\s+1024\b", text)
    assert callable(bev_amd.BevContext.set_pair_search_grid) and callable(bev_amd.BevContext.debug_pair_grid)
    assert lib.bev_abi_version() == 1


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("pairs")
    pcd = root / "pcd"
    pcd.mkdir()
    rng = np.random.default_rng(7)
    for i in range(3):
        pts = np.zeros(5, bev_amd.POINT_DTYPE)
        pts["x"], pts["y"], pts["z"] = rng.uniform(-1, 1, (3, 5)).astype(np.float32)
        pcd_util.write_pcd_binary(pcd / f"{i:06d}.pcd", pts)
    (root / "matches.txt").write_text("0 1 0.0\n2 1 5.0\n")
    return root


@pytest.mark.parametrize("tool", TOOLS)
@pytest.mark.parametrize("text", ["abc", "-1", "2000", "1,2,3", "1025", "256,", ",128", " 256", "256,-1", "1e2", "0x10"])
def test_the_tools_refuse_a_wrong_search_grid_before_any_device_work(tool, text, tree, tmp_path):
    env = dict(os.environ, BEV_PAIR_SEARCH_GRID=text)
    r = subprocess.run([str(HOST / tool), str(tree / "matches.txt"), str(tree / "pcd")], cwd=tmp_path, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    assert r.stdout == ""
    assert r.stderr == f"BEV_PAIR_SEARCH_GRID '{text}': expected <fine>[,<coarse>], integers 0 ... 1024\nUsage: {tool}{USAGE}"
    assert not list(tmp_path.iterdir())                     # refused before the reports are created
