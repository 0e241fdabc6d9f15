"""GPU: the polar descriptors and unit records of bev_place_descriptor_device_resident, byte for byte against
the sequential checker (tests/place/place_oracle.c), over frames and over maps."""
import functools

import numpy as np
import pytest
import torch

import bev_amd
import ground_truth_cases as gt
import oracle_lib as orc
import place_lib
from bev_amd import POINT_DTYPE, place_params, synth
from packed_cases import _p
from place_gpu_lib import descriptors, guarded, handles, HB

pytestmark = pytest.mark.gpu
SHAPES = [(20, 60, 80.0), (4, 8, 10.5), (32, 64, 37.25)]
L2G = 2.0  # bev_params_for_sensor's lidar_to_ground


@pytest.fixture(scope="module")
def ctx():
    c = bev_amd.BevContext(_p(), device=0, max_batch=4)
    yield c
    c.close()


def _seeded(rng, n, max_range):
    """points over 1.2 x the range, heights from below 0 to above the 127 clamp, a fifth of the labels 0"""
    c = np.zeros(n, POINT_DTYPE)
    c["x"], c["y"] = rng.uniform(-1.2 * max_range, 1.2 * max_range, (2, n)).astype(np.float32)
    c["z"] = rng.uniform(-6.0, 40.0, n).astype(np.float32)
    c["label"] = rng.uniform(size=n) >= 0.2
    return c


def _on_r2(target):
    """(x, y) float32 with x * x + y * y == target in float, searched near (0.8, 0.6) sqrt(target); None if there is none"""
    t = np.float32(target)
    x0, y0 = np.float32(0.8 * np.sqrt(float(t))), np.float32(0.6 * np.sqrt(float(t)))
    xs, ys = [x0], [y0]
    for _ in range(12):
        xs += [np.nextafter(xs[-1], np.float32(np.inf))]
        ys += [np.nextafter(ys[-1], np.float32(np.inf))]
    for k in range(12):
        xs += [np.nextafter(min(xs), np.float32(0))]
        ys += [np.nextafter(min(ys), np.float32(0))]
    X, Y = np.meshgrid(np.array(xs, np.float32), np.array(ys, np.float32))
    hit = np.argwhere(X * X + Y * Y == t)
    return (X[tuple(hit[0])], Y[tuple(hit[0])]) if len(hit) else None


def _edges(R, C, max_range):
    """points exactly on ring edges and one ulp to either side, at azimuth 0 and +-180, on sector edges, at the origin, with
    NaN, inf and -0.0 coordinates: POINT_DTYPE records of label 1 (every third 0), heights 1 .. 9"""
    edge2 = np.array([np.float32((np.float64(np.float32(max_range)) * k / R) ** 2) for k in range(R + 1)], np.float32)
    xy, found = [], 0
    for k in range(1, R + 1):
        for t in (np.nextafter(edge2[k], np.float32(0)), edge2[k], np.nextafter(edge2[k], np.float32(np.inf))):
            p = _on_r2(t)
            if p is not None:
                found += 1
                xy += [p, (-p[1], p[0]), (-p[0], -p[1])]
    assert found >= 2 * R, "the search finds most ring edges exactly"
    r = np.float32(0.37 * max_range)
    nz, inf, nan = np.float32(-0.0), np.float32(np.inf), np.float32(np.nan)
    xy += [(r, 0.0), (r, nz), (-r, 0.0), (-r, nz), (0.0, r), (nz, r), (0.0, -r), (nz, -r), (r, r), (-r, r), (r, -r), (-r, -r)]
    for s in range(C):  # a sector's lower edge as float rounding leaves it, and a hair to either side
        for da in (0.0, 1e-5, -1e-5):
            a = np.deg2rad(s * 360.0 / C + da)
            xy.append((np.float32(r * np.cos(a)), np.float32(r * np.sin(a))))
    xy += [(0.0, 0.0), (nz, nz), (nz, 0.0), (nan, r), (r, nan), (inf, r), (r, -inf), (inf, inf), (nan, nan),
           (np.float32(1e-30), 0.0), (np.float32(1e-23), np.float32(1e-23)), (np.float32(3e38), 1.0)]
    c = np.zeros(len(xy) + 4, POINT_DTYPE)
    c["x"][: len(xy)], c["y"][: len(xy)] = np.array(xy, np.float32).T
    c["z"] = 1.0 + (np.arange(len(c)) % 9) * 0.25
    c["label"] = np.arange(len(c)) % 3 != 0
    c["x"][len(xy):], c["y"][len(xy):] = r, r            # one cell: NaN, inf, negative and clamped heights
    c["z"][len(xy):] = [nan, inf, -5.0, 1000.0]
    c["label"][len(xy):] = 1
    return c


@functools.lru_cache(maxsize=None)
def _frames(R, C, max_range):
    rng = np.random.default_rng([11, R, C])
    return [_seeded(rng, n, max_range) for n in (0, 1, 255, 256, 257, 5000, 1025)] + [_edges(R, C, max_range)]


def _rigid(roll, pitch, yaw, t):
    return gt.pose(roll, pitch, yaw, t)[:3].astype(np.float32).reshape(12)


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("R,C,max_range", SHAPES)
def test_frames_against_the_checker(ctx, R, C, max_range, skip):
    prm = place_params(R, C, max_range, skip)
    frames = _frames(R, C, max_range)
    assert bev_amd.place_descriptor_bytes(prm) == R * C and bev_amd.place_desc_handle_bytes(prm) == HB
    desc, units = descriptors(ctx, frames, prm)
    want = np.stack([place_lib.descriptor([(f, None)], prm, L2G) for f in frames])
    assert want[5].any() and want[7].any() and not want[0].any()
    assert desc.tobytes() == want.tobytes()
    assert units.tobytes() == handles(want).tobytes()
    only_units = descriptors(ctx, frames, prm, want_desc=False)[1]
    only_desc = descriptors(ctx, frames, prm, want_units=False)[0]
    assert only_units.tobytes() == units.tobytes() and only_desc.tobytes() == desc.tobytes()


@pytest.mark.parametrize("R,C,max_range", SHAPES)
def test_maps_against_the_checker_and_the_concatenation(ctx, R, C, max_range):
    prm = place_params(R, C, max_range, True)
    frames = _frames(R, C, max_range)
    mats = [_rigid(1.5, -2.0, 33.0, [0.3 * max_range, -0.1 * max_range, 0.4]), _rigid(-3.0, 0.5, -120.0, [-2.0, 1.0, -0.3]),
            _rigid(0.0, 0.0, 180.0, [0.0, 0.0, 0.0]), _rigid(10.0, 10.0, 77.0, [0.05 * max_range, 0.3 * max_range, 2.0]),
            np.eye(3, 4, dtype=np.float32).reshape(12)]
    maps = [[(5, mats[0])], [], [(7, mats[1]), (5, mats[2]), (4, mats[3])],
            [(6, mats[0]), (0, mats[1]), (7, mats[4]), (2, mats[3]), (6, mats[2])]]  # frame 5 in two maps, frame 6 twice in one
    offs = np.cumsum([0] + [len(m) for m in maps]).astype(np.uint64)
    ef = np.array([f for m in maps for f, _ in m], np.int32)
    ep = np.array([mat for m in maps for _, mat in m], np.float32).reshape(-1, 12)
    desc, units = descriptors(ctx, frames, prm, maps=(offs, ef, ep))
    want = np.stack([place_lib.descriptor([(frames[f], mat) for f, mat in m], prm, L2G) for m in maps])
    assert not want[1].any() and want[0].any() and want[3].any()
    assert desc.tobytes() == want.tobytes() and units.tobytes() == handles(want).tobytes()
    for g, m in enumerate(maps):  # the descriptor of the concatenated bev_transform_cloud outputs
        moved = [orc.transform_cloud(np.ascontiguousarray(frames[f]), mat) for f, mat in m]
        cat = np.concatenate(moved) if moved else np.empty(0, POINT_DTYPE)
        assert desc[g].tobytes() == place_lib.descriptor([(cat, None)], prm, L2G).tobytes(), g


def test_statuses(ctx):
    frames = _frames(20, 60, 80.0)[:3]
    for bad in (place_params(3, 60), place_params(33, 60), place_params(20, 7), place_params(20, 65),
                place_params(20, 60, 0.0), place_params(20, 60, float("inf")), place_params(20, 60, float("nan"))):
        assert bev_amd.place_descriptor_bytes(bad) == 0 and bev_amd.place_desc_handle_bytes(bad) == 0
        with pytest.raises(bev_amd.BevError):
            descriptors(ctx, frames, bad)
    with pytest.raises(bev_amd.BevError):
        descriptors(ctx, frames, place_params(), want_desc=False, want_units=False)
    with pytest.raises(bev_amd.BevError):  # an entry frame outside the call
        descriptors(ctx, frames, place_params(), maps=(np.array([0, 1], np.uint64), np.array([3], np.int32), np.zeros((1, 12), np.float32)))


def test_d_ordered_straight_from_the_bev_path(ctx):
    """process_device, then the descriptor call on its d_ordered with nothing between them"""
    p = _p()
    sp = orc.sensor_from_params(p)
    S, dev = p.slots, torch.device("cuda:0")
    clouds = [synth.sweep(p, 40), synth.sweep(p, 41)[:70000]]
    nf = len(clouds)
    want_ordered = [orc.mark_ground(sp, orc.order_cloud(sp, c))[0] for c in clouds]
    offs_in = np.cumsum([0] + [len(c) for c in clouds]).astype(np.uint64)
    offs_s = np.arange(nf + 1, dtype=np.uint64) * np.uint64(S)
    prm = place_params()
    src = torch.from_numpy(np.concatenate(clouds).view(np.uint8).reshape(-1).copy()).to(dev)
    d_ordered = torch.zeros(nf * S * 32, dtype=torch.uint8, device=dev)
    d_multi = torch.zeros(nf * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    d_single = torch.zeros(nf * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    d_desc, d_units = guarded(nf * 1200), guarded(nf * HB)
    torch.cuda.synchronize()
    ctx.process_device(nf, src.data_ptr(), offs_in, d_ordered.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
    ctx.place_descriptor_device(nf, d_ordered.data_ptr(), offs_s, d_desc.data_ptr(), d_units.data_ptr(), prm)
    ctx.synchronize()
    want = np.stack([place_lib.descriptor([(c, None)], prm, L2G) for c in want_ordered])
    assert want.any()
    assert d_desc[: nf * 1200].cpu().numpy().tobytes() == want.tobytes()
    assert d_units[: nf * HB].cpu().numpy().tobytes() == handles(want).tobytes()
