"""GPU: BEV_SUBMAP_TOP_UNION of batch_submap_top_part_registration end to end, on the tree that
test_cli_submap_pn_leaf_gpu.py builds (parts of one world seen from six exact poses).  Unset, empty and 0 write identical files
and lines, with and without a leaf; 1 with BEV_SUBMAP_PN_LEAF=0.5 at half window 2 equals the checker composition (the front
end's chain as the queries, submap_top_cases.py over the full clouds, submap_reg_cases.py from the coarse table) through the
report arithmetic of fineicp_lib.report_line, at two chunk sizes; 1 without a leaf is refused; batch_submap_registration, which
has no coarse stage, writes the same with and without the variable."""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bev_amd
import fineicp_lib as fl
import icp_lib as il
import regfront_lib as rl
import submap_pn_vox_cases as pv
import submap_reg_cases as sc
import submap_top_cases as tc
import test_cli_submap_top_part_registration_gpu as top
from test_cli_submap_pn_leaf_gpu import _files, tree  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
HOST = Path(bev_amd.PKG_DIR) / "host"
TOOL = "batch_submap_top_part_registration"
THREADS = min(16, os.cpu_count() or 4)
N = top.N
VARS = ("BEV_SUBMAP_PN_LEAF", "BEV_SUBMAP_TOP_UNION")


@pytest.fixture(scope="module", autouse=True)
def _checkers():
    fl.build()
    il.build()
    rl.build()


def _run(tool, args, cwd, union=None, pn_leaf=None, expect=0):
    env = {k: v for k, v in os.environ.items() if k not in VARS}
    if union is not None:
        env["BEV_SUBMAP_TOP_UNION"] = union
    if pn_leaf is not None:
        env["BEV_SUBMAP_PN_LEAF"] = pn_leaf
    r = subprocess.run([str(HOST / tool), *[str(a) for a in args]], cwd=cwd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == expect, r.stdout + r.stderr
    return r


def test_unset_empty_and_zero_write_identical_files(tree, tmp_path):
    for leaf in (None, "0.5"):
        outs = {}
        for name, text in (("unset", None), ("empty", ""), ("zero", "0")):
            d = tmp_path / f"{name}_{leaf}"
            d.mkdir()
            r = _run(TOOL, [tree["root"] / "matches.txt", tree["root"], 2], d, union=text, pn_leaf=leaf)
            outs[name] = (top._stdout_without_times(r), _files(d))
        assert outs["unset"][1]["icp_precision_report.txt"].count(b"\n") >= 5
        assert outs["empty"] == outs["unset"] and outs["zero"] == outs["unset"]


def test_one_with_half_a_metre_at_half_window_2_equals_the_checker_at_two_chunk_sizes(tree, tmp_path):
    root, rows, clouds = tree["root"], tree["rows"], tree["clouds"]
    leaf = 0.5
    maps = sc.Maps()
    for k, (q, t, a) in enumerate(rows):  # one map per match: the window of its key frame, ascending
        maps.add([(j, sc.IDENTITY if j == t else top._relative(t, j)) for j in range(max(0, t - 2), min(N - 1, t + 2) + 1)])
    m = sc.matches([(q, k, a) for k, (q, t, a) in enumerate(rows)])
    pn = tc.queries(clouds)
    coarse, best = tc.expected(pn, clouds, maps, m, leaf, threads=THREADS)
    guesses = [coarse[k, best[k]]["T"].reshape(4, 4).copy() for k in range(len(m))]
    fine = sc.expected(clouds, maps, m, fl.params(**fl.FINE), guesses, threads=THREADS)
    lines = "".join(fl.report_line(fine[k]["T"], guesses[k]) for k in range(len(m)) if not fine[k]["fitness"] > 1.5)
    print(f"coarse states {coarse['state'].tolist()} best {best.tolist()} fine fitness {fine['fitness'].tolist()}")
    assert lines.count("\n") >= 5
    concat = pv.expected(pn, maps, m, leaf, threads=THREADS)
    assert concat[0].tobytes() != coarse.tobytes()                         # another target than the thinned concatenation's
    outs = {}
    for chunk in ("6", None):
        d = tmp_path / f"chunk{chunk}"
        d.mkdir()
        r = _run(TOOL, [root / "matches.txt", root, 2] + ([chunk] if chunk else []), d, union="1", pn_leaf="0.5")
        assert (d / "icp_precision_report.txt").read_text() == lines, chunk
        assert top._summary(fine["fitness"]) in r.stdout
        assert re.search(r"\[TIME\] Avg Tiempo for 1st Stage \(coarse\): ", r.stdout)
        outs[chunk] = (top._stdout_without_times(r), _files(d))
    assert outs["6"] == outs[None]


def test_one_without_a_leaf_is_refused(tree, tmp_path):
    for leaf in (None, "0"):
        r = _run(TOOL, [tree["root"] / "matches.txt", tree["root"], 2], tmp_path, union="1", pn_leaf=leaf, expect=1)
        assert "BEV_SUBMAP_TOP_UNION" in r.stderr and "BEV_SUBMAP_PN_LEAF" in r.stderr and r.stdout == ""
        assert not list(tmp_path.iterdir())


def test_the_whole_tool_ignores_the_variable(tree, tmp_path):
    outs = {}
    for name, text in (("unset", None), ("set", "1"), ("bad", "maybe")):
        d = tmp_path / name
        d.mkdir()
        r = _run("batch_submap_registration", [tree["root"] / "matches.txt", tree["root"], 2], d, union=text)
        outs[name] = (top._stdout_without_times(r), _files(d))
    assert outs["unset"][1]["icp_precision_report_submap.txt"].count(b"\n") >= 5
    assert outs["set"] == outs["unset"] and outs["bad"] == outs["unset"]
