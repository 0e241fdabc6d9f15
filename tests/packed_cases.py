"""What the GPU tests of the calls over packed frames share (tests/test_float_bev_batch_gpu.py, test_posed_bev_gpu.py,
test_submap_bev_gpu.py): the source clouds, the packing of frames into one device buffer, the poses,
the guarded outputs of a device call and the status codes.  Each cloud is computed once per session and is read-only.  Test
infrastructure only."""
import functools

import numpy as np
import torch

import bev_amd
import oracle_lib as orc
from bev_amd import POINT_DTYPE, synth

GUARD = 1 << 16       # bytes behind each output
PATTERN = 0xA5
# test_transform_cloud's poses (tx, ty, tz, yaw), and one that pushes most points off the grid
POSES = [(0, 0, 0, 0), (1.5, -2.25, 0.125, 30), (-3, 4, 1, -45.5), (10, 20, -1, 180), (0.1, 0.2, 0.3, 359.9)]
FAR = (150, 0, 0, 10)
# a general rigid matrix, every entry far from 0 and 1: frame 1 of raster_world_cases.py's map T (12 deg of roll, -9 of pitch)
GENERAL = np.array([0.9024916887283325, 0.41009873151779175, 0.13163472712039948, -12.794914245605469,
                    -0.4304434359073639, 0.8694769144058228, 0.24233940243721008, 4.982234001159668,
                    -0.015070266090333462, -0.27537062764167786, 0.9612199664115906, 1.820896863937378], dtype=np.float32)
INVALID, UNSUPPORTED, TOO_LARGE = -1, -5, -6


@functools.lru_cache(maxsize=None)
def _p(sensor="HDL_64E"):
    return bev_amd.params_for_sensor(sensor)


@functools.lru_cache(maxsize=None)
def _marked(frame_id=21, sensor="HDL_64E"):
    """a full sweep, ordered and ground-marked: S records, labels 0 among them"""
    sp = orc.sensor_from_params(_p(sensor))
    cloud = orc.mark_ground(sp, orc.order_cloud(sp, synth.sweep(_p(sensor), frame_id)))[0]
    assert (cloud["label"] == 0).any() and (cloud["label"] != 0).any()
    cloud.setflags(write=False)
    return cloud


@functools.lru_cache(maxsize=None)
def _adversarial(n=60000, seed=3):
    cloud = synth.adversarial(_p(), n, seed, nonfinite=True)
    assert (cloud["label"] == 0).any() and not np.isfinite(cloud["z"]).all()
    cloud.setflags(write=False)
    return cloud


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(torch.device("cuda:0"))


def _pack(frames):
    offs = np.zeros(len(frames) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    flat = np.concatenate([np.ascontiguousarray(f, dtype=POINT_DTYPE) for f in frames] + [np.zeros(1, POINT_DTYPE)])
    return offs, flat


def _matrix(pose):
    return orc.yaw_translate_matrix(*[float(v) for v in pose])


def _one_cell(zs, labels=1):
    cloud = np.zeros(len(zs), dtype=POINT_DTYPE)
    cloud["x"], cloud["y"], cloud["z"], cloud["label"] = 0.3, -7.2, zs, labels
    return cloud


def _ragged_frames(n_large, n_frames, more_small=()):
    """frames of 0, 1, 255 ... 4097 points (and of more_small's counts behind them), n_large frames of 3000 ... 40000, the
    full sweep and two empty frames: n_frames in all"""
    adv, marked = _adversarial(), _marked()
    small = [0, 0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 4097, *more_small]
    frames = [adv[41 * i:41 * i + n] for i, n in enumerate(small)]
    rng = np.random.default_rng(11)
    for i, n in enumerate(rng.integers(3000, 40001, n_large)):
        src = adv if i % 2 else marked
        frames.append(src[1000 * i:1000 * i + int(n)])
    frames += [marked, adv[:0], adv[:0]]
    assert len(frames) == n_frames and len(marked) == 133312
    return frames


class _Out:
    """both outputs of a device call with guard bytes behind them"""

    def __init__(self, p, n_grids, multi=True, single=True):
        dev = torch.device("cuda:0")
        self.n, self.L, self.M = n_grids, p.n_layers, p.mat_size
        self.mb, self.sb = n_grids * self.L * self.M ** 2, n_grids * self.M ** 2
        self.multi = torch.full((self.mb + GUARD,), PATTERN, dtype=torch.uint8, device=dev) if multi else None
        self.single = torch.full((self.sb + GUARD,), PATTERN, dtype=torch.uint8, device=dev) if single else None

    def ptrs(self):
        return (self.multi.data_ptr() if self.multi is not None else None,
                self.single.data_ptr() if self.single is not None else None)

    def images(self):
        m = self.multi[:self.mb].cpu().numpy().reshape(self.n, self.L, self.M, self.M) if self.multi is not None else None
        s = self.single[:self.sb].cpu().numpy().reshape(self.n, self.M, self.M) if self.single is not None else None
        return m, s

    def guards_ok(self):
        return all(bool((t[b:] == PATTERN).all()) for t, b in ((self.multi, self.mb), (self.single, self.sb)) if t is not None)

    def untouched(self):
        return all(bool((t == PATTERN).all()) for t in (self.multi, self.single) if t is not None)
