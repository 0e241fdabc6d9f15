"""GPU: scripts/bench_align.py at reduced arguments, as a fresh child process: one JSON line with the keys the
script documents, written to --out as well, as test_bench_scripts_gpu.py asks of the other scripts.  Nothing here is about a
time."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from test_bench_scripts_gpu import key_paths

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
ARGS = ["--frames", "6", "--hits", "5", "--steps", "1", "--warmup", "0", "--distinct", "2", "--rounds", "1"]
KEYS = """
metric frames hits steps warmup records_per_frame grid cell max_shift yaw_steps yaw_step skip_label0 byte_shift_form device host library
grids.fenced_median_ms grids.fenced_frames_per_s grids.unfenced_mean_ms
grids.kernels_ms_per_step.k_align_grid.ms_per_step grids.kernels_ms_per_step.k_align_grid.launches
grids.kernels_ms_per_step.k_align_finish.ms_per_step grids.kernels_ms_per_step.k_align_finish.launches
hits_call.fenced_median_ms hits_call.fenced_hits_per_s hits_call.unfenced_mean_ms hits_call.unfenced_hits_per_s
hits_call.kernels_ms_per_step.k_align_hit.ms_per_step hits_call.kernels_ms_per_step.k_align_hit.launches
hits_call.kernels_ms_per_step.k_align_pick.ms_per_step hits_call.kernels_ms_per_step.k_align_pick.launches
hits_call.kernel_shares.k_align_hit hits_call.kernel_shares.k_align_pick hits_call.checked_against_the_checker
against_place_match.queries against_place_match.database against_place_match.alternated_hits_ms
against_place_match.alternated_place_match_ms against_place_match.alternated_hits_median_ms
against_place_match.alternated_place_match_median_ms
against_fine.settings against_fine.alternated_hits_ms against_fine.alternated_fine_ms against_fine.alternated_hits_median_ms
against_fine.alternated_fine_median_ms against_fine.stage_share_of_fine
"""


def test_bench_align(tmp_path):
    out = tmp_path / "deeper" / "line.json"
    r = subprocess.run([sys.executable, str(REPO / "scripts" / "bench_align.py"), *ARGS, "--out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.count("\n") == 1 and r.stdout.endswith("\n"), r.stdout[-2000:]
    assert out.read_text() == r.stdout
    line = json.loads(r.stdout)
    assert key_paths(line) == set(KEYS.split())
    assert line["library"] == "csrc/libbev_mi355x.so" or "BEV_AMD_LIB" in os.environ
    assert line["hits_call"]["checked_against_the_checker"] is True
    assert (line["grid"], line["max_shift"], line["yaw_steps"], line["hits"]) == (128, 16, 1, 5)
