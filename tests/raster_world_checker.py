"""The checker's side of the world tests: the oracle's composition — transform_cloud per entry, concatenate,
then multi_bev / single_bev / float_bev — on the frames and float32 matrices of raster_world_cases.py, and the mutants of that
construction that test_raster_world_cpu.py shows the float64 reference to catch.  Tests only."""
from __future__ import annotations

import numpy as np

import bev_amd
import oracle_lib as orc
import raster_world_cases as rw
from bev_amd import POINT_DTYPE

F32, F64 = np.float32, np.float64


def params(c: rw.Case):
    """the sensor's bev_params_t at the configuration's interval"""
    p = bev_amd.params_for_sensor(c.sensor)
    assert p.height_res == c.height_res and p.max_range == rw.R_MAIN and p.n_layers == rw.N_LAYERS and p.lidar_to_ground == rw.LIDAR_TO_GROUND
    p.interval = c.interval
    assert p.mat_size == c.M
    return p


def moved(frames, entries) -> np.ndarray:
    parts = [orc.transform_cloud(np.ascontiguousarray(frames[f]), m) for f, m in entries]
    return np.concatenate(parts) if parts else np.empty(0, POINT_DTYPE)


def composition(c: rw.Case, entries, frames=None):
    """{"multi", "single", "float1" (label 0 skipped), "float0"}: the oracle's images of one map"""
    p = params(c)
    cloud = moved(c.frames if frames is None else frames, entries)
    return {"multi": orc.multi_bev(orc.sensor_from_params(p), cloud, p.interval), "single": orc.single_bev(cloud, p.interval),
            "float1": orc.float_bev(cloud, c.interval, True), "float0": orc.float_bev(cloud, c.interval, False)}


def reference(c: rw.Case, name):
    multi, single = c.reference(name)
    return {"multi": multi, "single": single, "float1": c.reference_float(name, True), "float0": c.reference_float(name, False)}


def compare(got, want, tol, what) -> float:
    """the images `got` (any of the four keys) against the float64 reference's: bytes, or occupancy and tol; returns the
    largest distance of a float grid"""
    worst = 0.0
    for key, g in got.items():
        if key.startswith("float"):
            worst = max(worst, rw.compare_float(g, want[key], tol, f"{what}, {key}"))
        else:
            rw.compare_bytes(g, want[key], f"{what}, {key}")
    return worst


# ---- mutants: (name, the images they can change, maps they cannot change, how) ---------------------------------------------------
ALL = ("multi", "single", "float1", "float0")


def _rt(m):
    m = np.asarray(m, F64).reshape(3, 4)
    return m[:, :3], m[:, 3]


def _m12(R, t):
    return np.c_[R, t].astype(F32).reshape(12)


def _each(fn):
    return lambda entries: [(f, fn(m)) for f, m in entries]


def _inverse(m):
    R, t = _rt(m)
    Ri = np.linalg.inv(R)
    return _m12(Ri, -Ri @ t)


def _swap89(m):
    m = np.array(m, F32)
    m[[8, 9]] = m[[9, 8]]
    return m


def _next(entries):
    return [(f, entries[(e + 1) % len(entries)][1]) for e, (f, _) in enumerate(entries)]


def _ignore_one(entries):
    e = next(e for e, (_, m) in enumerate(entries) if not np.array_equal(m, rw.IDENTITY12))
    return [(f, rw.IDENTITY12 if i == e else m) for i, (f, m) in enumerate(entries)]


MATRIX_MUTANTS = {
    "rotation transposed": (_each(lambda m: _m12(_rt(m)[0].T, _rt(m)[1])), ALL, ()),
    "P_j^-1 P_o": (_each(_inverse), ALL, ()),
    "entry e under entry e + 1's matrix": (_next, ALL, ("D",)),          # D names one frame twice: swapping its matrices is D
    "one entry's matrix ignored": (_ignore_one, ALL, ()),
    "m[8] and m[9] swapped": (_each(_swap89), ALL, ()),
    "translation rotated by the transpose": (_each(lambda m: _m12(_rt(m)[0], _rt(m)[0].T @ _rt(m)[1])), ALL, ()),
    "the last entry alone": (lambda entries: entries[-1:], ALL, ()),
}


def _shift_one_bin(img):
    """what a bin without its + 1 gives: every cell one row and one column lower, bin 0 lost"""
    out = np.zeros_like(img)
    out[..., :-1, :-1] = img[..., 1:, 1:]
    return out


def _matrix_mutant(mutant):
    def run(c, name):
        fn, keys, not_on = MATRIX_MUTANTS[mutant]
        if name in not_on:
            return None
        got = composition(c, fn(c.entries(name)))
        return {k: got[k] for k in keys}
    return run


def _floor_layer(c, name):
    # floor(v) = round(v - 0.5) away from ties: half a layer lower, in the multi-layer image only
    lower = [(f, m + np.array([0] * 11 + [-0.5 * c.height_res], F32)) for f, m in c.entries(name)]
    return {"multi": composition(c, lower)["multi"]}


def _labels_kept(c, name):
    kept = []
    for f in c.frames:
        f = f.copy()
        f["label"] = 1
        kept.append(f)
    got = composition(c, c.entries(name), kept)
    return {k: got[k] for k in ("multi", "single", "float1")}


# mutant -> (case, map) -> {image key: mutated image} for the images it can change, or None where it cannot change the map
MUTANTS = {m: _matrix_mutant(m) for m in MATRIX_MUTANTS}
MUTANTS["image indexed [y, x]"] = lambda c, name: {k: np.ascontiguousarray(np.swapaxes(v, -1, -2))
                                                   for k, v in composition(c, c.entries(name)).items()}
MUTANTS["bin without the + 1"] = lambda c, name: {k: _shift_one_bin(v) for k, v in composition(c, c.entries(name)).items()}
MUTANTS["layer from floor"] = _floor_layer
MUTANTS["label-0 records kept"] = _labels_kept
assert len(MUTANTS) == 11
