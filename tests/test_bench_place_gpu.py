"""GPU: scripts/bench_place_retrieval.py at reduced arguments, as a fresh child process: one JSON line with the
keys the script documents, written to --out as well, as test_bench_scripts_gpu.py asks of the other scripts.  Nothing here is
about a time."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from test_bench_scripts_gpu import key_paths

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
ARGS = ["--frames", "12", "--steps", "1", "--warmup", "0", "--distinct", "2", "--rounds", "1", "--max-square", "24"]
KEYS = """
metric frames steps warmup records_per_frame n_rings n_sectors max_range skip_label0 device host library
descriptor.fenced_median_ms descriptor.fenced_frames_per_s descriptor.unfenced_mean_ms descriptor.unfenced_frames_per_s
descriptor.kernels_ms_per_step.k_place_splat.ms_per_step descriptor.kernels_ms_per_step.k_place_splat.launches
descriptor.kernels_ms_per_step.k_place_finish.ms_per_step descriptor.kernels_ms_per_step.k_place_finish.launches
descriptor.alternated_ms descriptor.alternated_float_bev_ms descriptor.alternated_median_ms
descriptor.alternated_float_bev_median_ms descriptor.checked_against_the_checker
match.queries match.database match.top_k match.fenced_median_ms match.fenced_pairs_per_s match.unfenced_mean_ms
match.unfenced_pairs_per_s match.kernels_ms_per_step.k_place_pairs.ms_per_step match.kernels_ms_per_step.k_place_pairs.launches
match.kernels_ms_per_step.k_place_topk.ms_per_step match.kernels_ms_per_step.k_place_topk.launches
match.squares[].side match.squares[].fenced_median_ms match.squares[].pairs_per_s match.largest_square_side_within_1s
"""


def test_bench_place_retrieval(tmp_path):
    out = tmp_path / "deeper" / "line.json"
    r = subprocess.run([sys.executable, str(REPO / "scripts" / "bench_place_retrieval.py"), *ARGS, "--out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.count("\n") == 1 and r.stdout.endswith("\n"), r.stdout[-2000:]
    assert out.read_text() == r.stdout
    line = json.loads(r.stdout)
    assert key_paths(line) == set(KEYS.split())
    assert line["library"] == "csrc/libbev_mi355x.so" or "BEV_AMD_LIB" in os.environ
    assert line["descriptor"]["checked_against_the_checker"] is True
    assert [s["side"] for s in line["match"]["squares"]] == [12, 24] and line["match"]["largest_square_side_within_1s"] == 24
