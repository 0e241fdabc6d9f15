"""scripts/benchlib.py against the text the sixteen bench scripts carried inline before they were folded onto it (DESIGN.md
§6y).  Every `_old_*` function below is a literal restatement of that text and stays here as the specification: the scripts'
numbers are comparable with the committed profiles only while the draws come from the generator in this order and the timed
regions fence in this order.  No GPU: the draws are host arithmetic, the protocol runs on a context that records its calls."""
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "scripts"))

import benchlib as bl  # noqa: E402

import bev_amd  # noqa: E402

F0, M, WINDOW_MATCHES = 9, 7, "1:7,3:5,5:9"


def _old_draws():
    """the registration scripts' draws: the world, the pairs, then window after window"""
    rng = np.random.default_rng(2026)
    yaw = rng.uniform(-20, 20, M).astype(np.float32)
    tr = rng.uniform(-1.5, 1.5, (M, 2)).astype(np.float32)
    pairs = np.zeros(M, bev_amd.MATCH_DTYPE)
    pairs["query_idx"] = np.arange(M)
    pairs["match_idx"] = F0 + np.arange(M)
    pairs["angle_guess"] = yaw + rng.uniform(-2, 2, M).astype(np.float32)
    identity = np.eye(3, 4, dtype=np.float32).reshape(12)
    windows = []
    for W, n in [(int(w.split(":")[0]), min(M, int(w.split(":")[1]))) for w in WINDOW_MATCHES.split(",")]:
        half = W // 2
        m_map = pairs[:n].copy()
        m_map["match_idx"] = np.arange(n)
        map_offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(W)
        entry_frame = np.zeros(n * W, np.int32)
        entry_pose = np.zeros((n * W, 12), np.float32)
        for i in range(n):
            for k, d in enumerate(range(-half, half + 1)):
                entry_frame[i * W + k] = F0 + (i + d) % M
                entry_pose[i * W + k] = identity if d == 0 else bev_amd.yaw_translate_matrix(
                    float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.3, 0.3)), 0.0, float(rng.uniform(-1, 1)))
        windows.append((W, n, m_map, map_offs, entry_frame, entry_pose))
    return rng, yaw, tr, pairs, windows


def test_draw_order():
    o_rng, o_yaw, o_tr, o_pairs, o_windows = _old_draws()
    rng, yaw, tr = bl.world_draws(M)
    w = SimpleNamespace(rng=rng, yaw=yaw, F0=F0, M=M)
    pairs = bl.moved_copy_pairs(w)
    assert yaw.tobytes() == o_yaw.tobytes() and tr.tobytes() == o_tr.tobytes()
    assert pairs.dtype == o_pairs.dtype and pairs.tobytes() == o_pairs.tobytes()
    lists = bl.parse_window_matches(WINDOW_MATCHES, M)
    assert lists == [(1, 7), (3, 5), (5, 7)] == [(W, n) for W, n, *_ in o_windows]   # n = 9 > M clips to M
    for (W, n), (_, _, o_map, o_offs, o_frame, o_pose) in zip(lists, o_windows):
        state = json.dumps(rng.bit_generator.state, sort_keys=True)
        m_map = bl.map_matches(pairs, n)
        map_offs, entry_frame, entry_pose = bl.cyclic_windows(rng, F0, M, n, W)
        assert m_map.tobytes() == o_map.tobytes()
        for got, want in ((map_offs, o_offs), (entry_frame, o_frame), (entry_pose, o_pose)):
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), W
        assert (json.dumps(rng.bit_generator.state, sort_keys=True) == state) == (W == 1)   # W = 1 draws nothing
        assert entry_frame.min() >= F0 and entry_frame.max() < F0 + M
    assert {int(f) for f in o_windows[2][4][:5]} == {F0 + 5, F0 + 6, F0, F0 + 1, F0 + 2}    # W = 5 wraps below 0 ...
    assert int(o_windows[1][4][-1]) == F0 + 5 and int(o_windows[2][4][-1]) == F0 + 1        # ... and W = 5 at n = M past M - 1
    assert rng.bit_generator.state == o_rng.bit_generator.state


def test_first_pairs_draw_as_many_as_they_are():
    """bench_pair_search_grid.py draws --matches guesses, not --moved"""
    rng = np.random.default_rng(2026)
    yaw = rng.uniform(-20, 20, M).astype(np.float32)
    rng.uniform(-1.5, 1.5, (M, 2))
    n = 4
    want = yaw[:n] + rng.uniform(-2, 2, n).astype(np.float32)
    g, y, _ = bl.world_draws(M)
    pairs = bl.moved_copy_pairs(SimpleNamespace(rng=g, yaw=y, F0=F0, M=M), n)
    assert len(pairs) == n and pairs["angle_guess"].tobytes() == want.tobytes()
    assert pairs["match_idx"].tolist() == [F0 + i for i in range(n)]
    assert g.bit_generator.state == rng.bit_generator.state


def test_frame_poses_draw_order():
    """bench_manip.py's and bench_posed_bev.py's poses: four draws per pose, frame by frame"""
    F = 3
    rng, o_rng = np.random.default_rng(1), np.random.default_rng(1)
    for n_poses in (0, 1, 8):
        want = None
        if n_poses:
            want = np.stack([np.stack([bev_amd.yaw_translate_matrix(o_rng.uniform(-5, 5), o_rng.uniform(-5, 5), o_rng.uniform(-0.5, 0.5),
                                                                     o_rng.uniform(-180, 180)) for _ in range(n_poses)])
                             for _ in range(F)])
        got = bl.frame_poses(rng, F, n_poses)
        assert (got is None and want is None) or (got.dtype == want.dtype and got.tobytes() == want.tobytes())
    assert rng.bit_generator.state == o_rng.bit_generator.state


@pytest.mark.parametrize("F,W", [(6, 1), (6, 3), (6, 5), (2, 5)])
def test_sliding_windows(F, W):
    h = W // 2
    rel = {d: bev_amd.yaw_translate_matrix(2.0 * d, 0.0, 0.0, 1.0 * d) for d in range(-h, h + 1)}
    windows = [range(max(0, i - h), min(F - 1, i + h) + 1) for i in range(F)]
    map_offs = np.zeros(F + 1, dtype=np.uint64)
    map_offs[1:] = np.cumsum([len(w) for w in windows])
    entry_frame = np.array([j for w in windows for j in w], dtype=np.int32)
    entry_pose = np.stack([rel[j - i] for i, w in enumerate(windows) for j in w])
    got_rel = bl.relative_poses(W)
    assert sorted(got_rel) == sorted(rel) and all(got_rel[d].tobytes() == rel[d].tobytes() for d in rel)
    g_windows, g_offs, g_frame, g_pose = bl.sliding_windows(F, W, got_rel)
    assert g_windows == windows
    for got, want in ((g_offs, map_offs), (g_frame, entry_frame), (g_pose, entry_pose)):
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
    if (F, W) == (2, 5):
        assert [len(w) for w in g_windows] == [2, 2]     # every window clipped on both sides


def test_parse_window_matches():
    assert bl.parse_window_matches("1:500,5:100,21:40", 500) == [(1, 500), (5, 100), (21, 40)]
    assert bl.parse_window_matches("1:500,5:100,21:40", 60) == [(1, 60), (5, 60), (21, 40)]


class _Ctx:
    """records what the protocol does to a context"""

    def __init__(self):
        self.calls = []
        self.stats = [{"name": "k_fine_icp", "total_ms": 2.0, "launches": 3}, {"name": "k_fine_grid", "total_ms": 0.5, "launches": 1},
                      {"name": "k_submap_icp", "total_ms": 4.0, "launches": 2}, {"name": "k_rf_top", "total_ms": 1.0, "launches": 1}]

    def step(self, name="s"):
        return lambda: self.calls.append(name)

    def synchronize(self):
        self.calls.append("Y")

    def profile_reset(self):
        self.calls.append("reset")

    def profile_enable(self, on):
        self.calls.append(("enable", on))

    def profile_get(self):
        self.calls.append("get")
        return self.stats


def test_timed_protocol():
    ctx = _Ctx()
    med, mean = bl.timed(ctx, ctx.step(), 3, 2)
    assert ctx.calls == ["s", "s", "Y"] + ["s", "Y"] * 3 + ["s", "s", "s", "Y"]
    assert med >= 0 and mean >= 0


def test_alternate_protocol(capsys):
    ctx = _Ctx()
    t_a, t_b = bl.alternate(ctx, ctx.step("a"), ctx.step("b"), 2)
    assert ctx.calls == ["a", "Y", "b", "Y"] + ["a", "Y", "b", "Y"] * 2
    assert len(t_a) == 2 and len(t_b) == 2
    err = capsys.readouterr().err.splitlines()
    assert len(err) == 6 and all(l.startswith("  step ") and l.endswith(" ms") for l in err)   # the progress lines
    ctx = _Ctx()
    t_a, t_b = bl.alternate(ctx, ctx.step("a"), ctx.step("b"), 2, warm=False, log=False)   # the search-grid scripts' rounds
    assert ctx.calls == ["a", "Y", "b", "Y"] * 2 and len(t_a) == 2 and len(t_b) == 2
    assert capsys.readouterr().err == ""


def test_kernel_ms_protocol():
    sequence = ["reset", ("enable", True), "s", "Y", "get", ("enable", False)]
    ctx = _Ctx()
    assert bl.kernel_ms(ctx, ctx.step(), "k_fine") == {"k_fine_icp": 2.0, "k_fine_grid": 0.5}
    assert ctx.calls == sequence
    ctx = _Ctx()
    assert bl.kernel_ms(ctx, ctx.step(), ("k_fine", "k_submap")) == {"k_fine_icp": 2.0, "k_fine_grid": 0.5, "k_submap_icp": 4.0}
    assert bl.kernel_ms(ctx, ctx.step()) == {s["name"]: s["total_ms"] for s in ctx.stats}
    ctx = _Ctx()
    got = bl.kernel_ms(ctx, ctx.step(), names=("k_submap_icp", "k_fine_icp", "k_not_launched"))
    assert got == {"k_submap_icp": {"ms_per_step": 4.0, "launches": 2}, "k_fine_icp": {"ms_per_step": 2.0, "launches": 3}}
    assert ctx.calls == sequence


def test_emit(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(bl, "device_name", lambda: "a stand-in device")
    monkeypatch.delenv("BEV_AMD_LIB", raising=False)
    out = tmp_path / "not" / "yet" / "there.json"
    bl.emit({"metric": "m", "runs": [1, 2]}, SimpleNamespace(out=str(out), label=None))
    printed = capsys.readouterr().out
    assert printed.count("\n") == 1 and out.read_bytes() == printed.encode()
    line = json.loads(printed)
    assert set(line) == {"metric", "runs", "device", "host", "library"}
    assert line["device"] == "a stand-in device" and line["library"] == "csrc/libbev_mi355x.so"
    monkeypatch.setenv("BEV_AMD_LIB", "/somewhere/libbev_head.so")
    bl.emit({}, SimpleNamespace(out=None, label=None), machine=("device",))                 # bench_submap_float_bev.py's keys
    assert json.loads(capsys.readouterr().out) == {"device": "a stand-in device", "library": "/somewhere/libbev_head.so"}
    bl.emit({}, SimpleNamespace(out=None, label="head"), machine=())                        # bench_submap_copy_out.py's
    assert json.loads(capsys.readouterr().out) == {"library": "head"}
    bl.emit({"runs": [1]}, SimpleNamespace(out=str(out), label="head"), final=False)         # a partial result on the way
    assert capsys.readouterr().out == "" and json.loads(out.read_text())["runs"] == [1]


def test_std_args():
    import argparse
    ap = argparse.ArgumentParser()
    bl.std_args(ap, frames=12, window_matches="1:2", out="x.json")
    a = ap.parse_args([])
    assert (a.frames, a.window_matches, a.label) == (12, "1:2", None) and a.out == str(bl.REPO / "profiles" / "x.json")
    a = ap.parse_args(["--frames", "3", "--label", "head", "--out", "y"])
    assert (a.frames, a.label, a.out) == (3, "head", "y")
    ap = argparse.ArgumentParser()
    bl.std_args(ap, out=None)
    assert ap.parse_args([]).out is None
