"""GPU: scripts/bench_verify.py at reduced arguments, as a fresh child process: one JSON line with the keys the
script documents, written to --out as well, as test_bench_scripts_gpu.py asks of the other scripts; every verify run equal to
the first.  Nothing here is about a time."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from test_bench_scripts_gpu import key_paths

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
ARGS = ["--frames", "8", "--moved", "4", "--sub-batch", "8", "--rounds", "1", "--window-matches", "3:1"]
RECORD = """matches register_ms verify_ms register_median_ms verify_median_ms verify_over_register verify_runs_byte_equal
n_query_mean n_target_mean forward_share_at_0.2.median forward_share_at_0.2.min reverse_share_at_0.2.median
reverse_share_at_0.2.min kernels_ms_per_step.k_fine_voxel.ms_per_step kernels_ms_per_step.k_fine_voxel.launches
kernels_ms_per_step.k_verify_move.ms_per_step kernels_ms_per_step.k_verify_move.launches
kernels_ms_per_step.k_verify_count.ms_per_step kernels_ms_per_step.k_verify_count.launches""".split()
PAIR_ONLY = ["kernels_ms_per_step.k_fine_grid.ms_per_step", "kernels_ms_per_step.k_fine_grid.launches"]
MAP_ONLY = [f"kernels_ms_per_step.k_submap_vox_{k}.{f}" for k in ("move", "keys", "tile", "finish") for f in ("ms_per_step", "launches")]
TOP = "metric sensor frames rounds settings thresholds map_leaf device host library".split()


def test_bench_verify(tmp_path):
    out = tmp_path / "deeper" / "line.json"
    r = subprocess.run([sys.executable, str(REPO / "scripts" / "bench_verify.py"), *ARGS, "--out", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.count("\n") == 1 and r.stdout.endswith("\n"), r.stdout[-2000:]
    assert out.read_text() == r.stdout
    line = json.loads(r.stdout)
    want = set(TOP) | {f"pairs.{k}" for k in RECORD + PAIR_ONLY} | {f"windows.3.{k}" for k in RECORD + MAP_ONLY}
    got = key_paths(line)
    assert got - {"windows.3.kernels_ms_per_step.k_submap_vox_global.ms_per_step",
                  "windows.3.kernels_ms_per_step.k_submap_vox_global.launches"} == want
    assert line["library"] == "csrc/libbev_mi355x.so" or "BEV_AMD_LIB" in os.environ
    assert line["pairs"]["matches"] == 4 and line["windows"]["3"]["matches"] == 1
    assert line["pairs"]["verify_runs_byte_equal"] is True and line["windows"]["3"]["verify_runs_byte_equal"] is True
    # a frame against its moved copy: the motion is found, and nearly every point has its neighbour within 0.2 m
    assert line["pairs"]["forward_share_at_0.2"]["median"] > 0.9
