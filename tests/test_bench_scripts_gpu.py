"""Every scripts/bench_*.py script still runs and still prints the line it printed before the fold onto scripts/benchlib.py
(DESIGN.md §6y): each script as a fresh child process at the reduced arguments of tests/bench_script_cases.py.  Nothing here
is about a time."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from bench_script_cases import CASES

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent


def key_paths(x, at=""):
    if isinstance(x, dict):
        return set().union(*[key_paths(v, f"{at}.{k}" if at else k) for k, v in x.items()]) if x else {at}
    if isinstance(x, list) and any(isinstance(v, (dict, list)) for v in x):
        return set().union(*[key_paths(v, at + "[]") for v in x])
    return {at}


@pytest.mark.parametrize("name", list(CASES))
def test_bench_script(name, tmp_path):
    case = CASES[name]
    out = tmp_path / "deeper" / "line.json"
    r = subprocess.run([sys.executable, str(REPO / "scripts" / f"{name}.py"), *case["args"], "--out", str(out)],
                       capture_output=True, text=True, timeout=case["timeout"])
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.count("\n") == 1 and r.stdout.endswith("\n"), r.stdout[-2000:]
    assert out.read_text() == r.stdout
    line = json.loads(r.stdout)
    assert key_paths(line) == set(case["keys"]) | {"library"}
    assert line["library"] == "csrc/libbev_mi355x.so" or "BEV_AMD_LIB" in os.environ
    windows = line.get("windows", {})
    if name in ("bench_submap_registration", "bench_submap_coarse_registration"):
        assert windows["1"]["identical_to_pair_call"] is True
        assert all(w["identical_to_pair_call"] is False for k, w in windows.items() if k != "1")
