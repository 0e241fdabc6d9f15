"""bench.py's command-line contract: `--gpus N` starts its own N ranks (or refuses clearly when the machine has fewer
GPUs), a plain run times its steps and nothing else, `--full` adds `roofline` and `cpu_baseline`, `--dump-outputs`
writes what the last timed step computed, and the single-rank RCCL path works under torch.distributed.run."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
BENCH = str(REPO / "bench.py")


def _device_count():
    import torch
    return torch.cuda.device_count()  # does not initialise the GPU


def test_gpus_beyond_the_machine_is_refused_before_any_gpu_call():
    n = _device_count()
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(max(2, n + 1)), "--no-build"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, r.stdout + r.stderr
    assert f"needs {max(2, n + 1)} visible GPUs, this machine shows {n}" in r.stderr
    assert r.stdout.strip() == ""


def _json_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


# two sub-batches of the default size: the front of one overlaps the back of the other, as in the full run
SMALL = ["--steps", "2", "--warmup", "1", "--frames", "512", "--cpu-sample", "8"]


def test_dump_outputs_writes_a_seeded_sample_under_64_mb(tmp_path):
    import bench
    import bev_amd

    S, L, M, count, first = 1000, 24, 224, 50, 7
    rng = np.random.default_rng(1)
    frames = np.zeros((count, S), bev_amd.POINT_DTYPE)
    for f in bench.ORDERED_FIELDS:
        frames[f] = rng.integers(0, 1000, (count, S))
    multi = rng.integers(0, 256, (count, L * M * M), dtype=np.uint8)
    single = rng.integers(0, 256, (count, M * M), dtype=np.uint8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), first, count, S, L, M, lambda i: (frames[i], multi[i], single[i]))
    names = sorted(f.name for f in (tmp_path / "a").iterdir())
    assert names == ["multi_bev.npy", "ordered_cloud.npy", "sample_frames.npy", "single_bev.npy"]
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 * 2**20
    got = {n: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert got[n].dtype in (np.float32, np.float64)
        assert np.array_equal(got[n], np.load(tmp_path / "b" / n))        # the same sample every run
    pick = got["sample_frames.npy"].astype(np.int64) - first
    assert len(pick) >= 1 and len(set(pick.tolist())) == len(pick) and 0 <= pick.min() and pick.max() < count
    for j, i in enumerate(pick):
        assert np.array_equal(got["ordered_cloud.npy"][j], np.stack([frames[i][f] for f in bench.ORDERED_FIELDS], -1))
        assert np.array_equal(got["multi_bev.npy"][j].reshape(-1), multi[i])
        assert np.array_equal(got["single_bev.npy"][j].reshape(-1), single[i])


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """A plain run: the headline only, `steps` timed steps, and --dump-outputs holds the oracle's outputs for its frames."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--steps", "3", "--warmup", "1", "--frames", "512", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - 512 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["cpu_baseline"] is None and d["roofline"] is None and d["kernels"] == [] and d["ms_per_step_median_fenced"] is None
    import bev_amd
    import oracle_lib as orc
    from bev_amd import synth
    p = bev_amd.params_for_sensor("HDL_64E")
    ordered, multi, single = (np.load(out / f"{n}.npy") for n in ("ordered_cloud", "multi_bev", "single_bev"))
    frames = np.load(out / "sample_frames.npy").astype(np.int64)
    assert ordered.dtype == np.float64 and multi.dtype == single.dtype == np.float32 and len(frames) == len(ordered) >= 1
    for j, fid in enumerate(frames):
        o_ord, _, o_multi, o_single = orc.process_frame(orc.sensor_from_params(p), synth.sweep(p, int(fid), keep=0.98, n_dup=5000))
        want = np.stack([o_ord[f].astype(np.float64) for f in ("x", "y", "z", "intensity", "row", "col", "t", "label")], -1)
        assert ordered[j].tobytes() == want.tobytes()                     # (empty slots hold NaN)
        assert np.array_equal(multi[j], o_multi.astype(np.float32)) and np.array_equal(single[j], o_single.astype(np.float32))


@pytest.mark.gpu
def test_json_line_has_roofline_and_cpu_baseline():
    r = subprocess.run([sys.executable, BENCH, *SMALL, "--full"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["full"] is True and d["ms_per_step_median_fenced"] > 0 and d["routes_last_sub_batch"]
    assert d["n_gpus"] == 1 and d["unit"] == "frames/s" and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["config"]["frames_per_step"] == 512
    rf, cb = d["roofline"], d["cpu_baseline"]
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and 0 < rf["frac"] < 1 and rf["kernel"].startswith("k_")
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9 and 0 < rf["pipeline"]["frac"] < 1
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0 and cb["gpu_output_matches_oracle_on_sampled_frame"] is True
    assert cb["timed_region"]["value"] > 0 and cb["timed_region"]["value"] <= cb["value"] * 1.05
    # the timed region runs fused launches (k_stage: a sub-batch's walk beside the later stages of its neighbours); the
    # one-lane pass behind it runs the same device code as one launch per kernel, which is what the roofline is read from
    assert "k_stage" in {k["name"] for k in d["kernels_pipelined"]}
    assert {"k_walk", "k_cell_sums", "k_ground_resolve", "k_bev_raster", "k_probe"} <= {k["name"] for k in d["kernels"]}
    assert rf["kernel"] == "k_walk"


@pytest.mark.gpu
def test_single_rank_under_torch_distributed_run_goes_through_rccl():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
                        "--master-port", "29617", BENCH, "--gpus", "1", *SMALL, "--no-cpu", "--no-profile"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 1 and d["value"] > 0
    # the line shows by itself what RCCL saw: the world size after init_process_group, the broadcast table, every rank's own figures
    assert d["ranks_seen"] == 1 and d["frame_range_table"] == [[0, 512]]
    assert len(d["per_rank"]) == 1 and d["per_rank"][0]["frames"] == 512 and d["per_rank"][0]["frames_per_s"] > 0


@pytest.mark.gpu
def test_two_ranks_over_rccl_when_the_box_has_two_gpus():
    n = _device_count()
    if n < 2:
        pytest.skip(f"needs 2 GPUs, this box shows {n}; the rank-spawning path is covered up to the launch by "
                    "test_gpus_beyond_the_machine_is_refused_before_any_gpu_call, the collectives by tests/test_distributed_cpu.py (gloo)")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", *SMALL, "--no-cpu"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["config"]["frames_per_step"] == 2 * 512 and d["value"] > 0
    assert d["ranks_seen"] == 2 and d["frame_range_table"] == [[0, 512], [512, 512]]
    assert [r["rank"] for r in d["per_rank"]] == [0, 1] and all(r["frames_per_s"] > 0 for r in d["per_rank"])
