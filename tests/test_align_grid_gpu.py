"""GPU: the candidate height grids and their sums of squares of bev_align_grid_device_resident, byte for byte
against the sequential checker (tests/align/align_oracle.c), over frames and over maps."""
import functools

import numpy as np
import pytest
import torch

import align_cases as ac
import bev_amd
import oracle_lib as orc
from align_gpu_lib import checker_grids, grids, guarded
from bev_amd import align_params, synth
from packed_cases import _p

pytestmark = pytest.mark.gpu
SHAPES = [(16, 2.0), (64, 0.5), (128, 0.5)]


@pytest.fixture(scope="module")
def ctx():
    c = bev_amd.BevContext(_p(), device=0, max_batch=4)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _frames(G, cell):
    rng = np.random.default_rng([41, G])
    return [ac.seeded(rng, n, G, cell) for n in (0, 1, 255, 256, 257, 5000, 1025)] + [ac.edge_frame(G, cell)]


def _energy(g):
    return (g.reshape(len(g), -1).astype(np.int64) ** 2).sum(axis=1).astype(np.uint32)


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("G,cell", SHAPES)
def test_frames_against_the_checker(ctx, G, cell, skip):
    prm = align_params(G, cell, 4, 1, 2.0, skip)
    frames = _frames(G, cell)
    assert bev_amd.align_grid_bytes(prm) == G * G
    got, energy = grids(ctx, frames, prm)
    want = checker_grids(frames, prm)
    assert want[5].any() and want[7].any() and not want[0].any()
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(energy, _energy(want))


@pytest.mark.parametrize("G,cell", SHAPES)
def test_maps_against_the_checker(ctx, G, cell):
    prm = align_params(G, cell, 4, 1, 2.0, True)
    frames = _frames(G, cell)
    ext = G * cell
    mats = [ac.rigid12(1.5, -2.0, 33.0, [0.15 * ext, -0.05 * ext, 0.4]), ac.rigid12(-3.0, 0.5, -120.0, [-2.0, 1.0, -0.3]),
            ac.rigid12(0.0, 0.0, 180.0, [0.0, 0.0, 0.0]), ac.rigid12(10.0, 10.0, 77.0, [0.02 * ext, 0.15 * ext, 2.0]),
            np.eye(3, 4, dtype=np.float32).reshape(12)]
    maps = [[(5, mats[0])], [], [(7, mats[1]), (5, mats[2]), (4, mats[3])],
            [(6, mats[0]), (0, mats[1]), (7, mats[4]), (2, mats[3]), (6, mats[2])]]  # frame 5 in two maps, frame 6 twice in one
    offs = np.cumsum([0] + [len(m) for m in maps]).astype(np.uint64)
    ef = np.array([f for m in maps for f, _ in m], np.int32)
    ep = np.array([mat for m in maps for _, mat in m], np.float32).reshape(-1, 12)
    got, energy = grids(ctx, frames, prm, maps=(offs, ef, ep))
    want = checker_grids(frames, prm, maps=(offs, ef, ep))
    assert not want[1].any() and want[0].any() and want[3].any()
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(energy, _energy(want))


def test_statuses(ctx):
    frames = _frames(16, 2.0)[:3]
    for bad in (align_params(14), align_params(130), align_params(33), align_params(cell=0.0), align_params(cell=float("nan")),
                align_params(max_shift=0), align_params(max_shift=17), align_params(32, 1.0, 9), align_params(yaw_steps=4),
                align_params(yaw_step=-1.0), align_params(yaw_step=float("inf"))):
        assert bev_amd.align_grid_bytes(bad) == 0
        with pytest.raises(bev_amd.BevError):
            grids(ctx, frames, bad)
    with pytest.raises(bev_amd.BevError):  # an entry frame outside the call
        grids(ctx, frames, align_params(), maps=(np.array([0, 1], np.uint64), np.array([3], np.int32), np.zeros((1, 12), np.float32)))
    offs = np.array([0, 0, 1, 256], np.uint64)
    d = guarded(64)
    with pytest.raises(bev_amd.BevError):  # no output
        ctx.align_grid_device(3, d.data_ptr(), offs, 0, d.data_ptr(), align_params())
    with pytest.raises(bev_amd.BevError):
        ctx.align_grid_device(3, d.data_ptr(), offs, d.data_ptr(), 0, align_params())
    with pytest.raises(bev_amd.BevError):  # records to read and no clouds
        ctx.align_grid_device(3, 0, offs, d.data_ptr(), d.data_ptr(), align_params())
    ctx.align_grid_device(0, 0, np.zeros(1, np.uint64), 0, 0, align_params())  # nothing to make


def test_d_ordered_straight_from_the_bev_path(ctx):
    """process_device, then the grid call on its d_ordered with nothing between them"""
    p = _p()
    sp = orc.sensor_from_params(p)
    S, dev = p.slots, torch.device("cuda:0")
    clouds = [synth.sweep(p, 40), synth.sweep(p, 41)[:70000]]
    nf = len(clouds)
    want_ordered = [orc.mark_ground(sp, orc.order_cloud(sp, c))[0] for c in clouds]
    offs_in = np.cumsum([0] + [len(c) for c in clouds]).astype(np.uint64)
    offs_s = np.arange(nf + 1, dtype=np.uint64) * np.uint64(S)
    prm = align_params()
    cells = prm.grid * prm.grid
    src = torch.from_numpy(np.concatenate(clouds).view(np.uint8).reshape(-1).copy()).to(dev)
    d_ordered = torch.zeros(nf * S * 32, dtype=torch.uint8, device=dev)
    d_multi = torch.zeros(nf * p.n_layers * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    d_single = torch.zeros(nf * p.mat_size ** 2, dtype=torch.uint8, device=dev)
    d_grids, d_energy = guarded(nf * cells), guarded(nf * 4)
    torch.cuda.synchronize()
    ctx.process_device(nf, src.data_ptr(), offs_in, d_ordered.data_ptr(), d_multi.data_ptr(), d_single.data_ptr())
    ctx.align_grid_device(nf, d_ordered.data_ptr(), offs_s, d_grids.data_ptr(), d_energy.data_ptr(), prm)
    ctx.synchronize()
    want = checker_grids(want_ordered, prm)
    assert want.any()
    assert d_grids[: nf * cells].cpu().numpy().tobytes() == want.tobytes()
    assert np.array_equal(d_energy[: nf * 4].cpu().numpy().view(np.uint32), _energy(want))
