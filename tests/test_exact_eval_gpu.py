"""GPU: the shared host/device arithmetic one function at a time — bev_debug_exact_eval (k_exact_eval: the dispatch of
csrc/bev_exact_eval.h on the device) against the host build of the same dispatch (tests/exacteval), bit for bit, on the
inputs of tests/exact_eval_cases.py, which tests/test_exact_eval_cpu.py has checked against plain references and shown to be
sharp against contraction to FMA and flush-to-zero.  Then frames made of the same edge inputs through the projection
kernels that inline these functions, against the oracle."""
import ctypes as C

import numpy as np
import pytest

import bev_amd
import exact_eval_cases as cs
import exacteval_lib as ee
import oracle_lib as orc

pytestmark = pytest.mark.gpu
U32 = np.uint32


@pytest.fixture(scope="module")
def ctx():
    ee.build()
    c = bev_amd.BevContext(bev_amd.params_for_sensor("HDL_64E"), device=0, max_batch=2, max_points=600000)
    yield c
    c.close()


def _compare(name, set_name, dev, host, inputs):
    """integers by bits; floats by bits, except that NaN matches NaN — as many pairs as the reference has NaNs"""
    assert dev.shape == host.shape and dev.dtype == host.dtype
    ia = dev.view({4: U32, 8: np.uint64}[dev.itemsize])
    differ = ia != host.view(ia.dtype)
    if dev.dtype.kind == "f":
        pairs = np.isnan(dev) & np.isnan(host)
        assert int(pairs.sum()) == int(np.isnan(host).sum()), (name, set_name, "a NaN of the host is a number on the device")
        differ &= ~pairs
    if differ.any():
        k = int(np.flatnonzero(differ.reshape(len(differ), -1).any(1))[0])
        raise AssertionError(f"{name} / {set_name}: {int(differ.sum())} of {differ.size} differ; first at element {k}: inputs "
                             f"{[a[k].tobytes().hex() for a in inputs]} device {dev[k].tobytes().hex()} host {host[k].tobytes().hex()}")


@pytest.mark.parametrize("name", bev_amd.EXACT_EVAL_NAMES)
def test_device_equals_host(ctx, name):
    for set_name, arrs, prm in cs.sets(name):
        _compare(name, set_name, ctx.exact_eval(name, *arrs, params=prm), ee.eval(name, *arrs, params=prm), arrs)


def test_one_element_and_a_ragged_tail(ctx):
    y, x = cs.column_edges()
    for n in (1, 255, 257, 1000):
        _compare("fd_atan2f", n, ctx.exact_eval("fd_atan2f", y[:n], x[:n]), ee.eval("fd_atan2f", y[:n], x[:n]), (y[:n], x[:n]))
    d = cs.f64_sweep()[:777]
    _compare("fd_sin", 777, ctx.exact_eval("fd_sin", d), ee.eval("fd_sin", d), (d,))
    t = [a[:513] for a in cs.triples()]
    m = np.array(cs.TRANSFORMS[2], np.float32)
    _compare("transform_xyz", 513, ctx.exact_eval("transform_xyz", *t, params=m), ee.eval("transform_xyz", *t, params=m), t)
    assert len(ctx.exact_eval("fd_atanf", np.empty(0, np.float32))) == 0


def test_refusals_leave_the_output_untouched(ctx):
    lib, h = ctx.lib, ctx._h
    x = np.ones(16, np.float32)
    out = np.full(48, 0xA5A5A5A5, U32)
    before = out.copy()
    px, po, null = C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data), None
    one = bev_amd.EXACT_EVAL_NAMES.index("fd_atanf")
    two = bev_amd.EXACT_EVAL_NAMES.index("fd_atan2f")
    xf = bev_amd.EXACT_EVAL_NAMES.index("transform_xyz")
    INVALID = -1  # BEV_ERR_INVALID_ARG
    calls = [
        (None, one, 16, px, null, null, null, null, po),               # no context
        (h, one, 16, null, null, null, null, null, po),                # the array the id reads
        (h, two, 16, px, null, null, null, null, po),                     # its second array
        (h, one, 16, px, null, null, null, null, null),                # no output
        (h, -1, 16, px, px, px, px, px, po),                              # unknown ids
        (h, len(bev_amd.EXACT_EVAL_NAMES), 16, px, px, px, px, px, po),
        (h, xf, 16, px, px, px, null, null, po),                          # the matrix
        (h, one, bev_amd.EXACT_EVAL_MAX_N + 1, px, null, null, null, null, po),  # too many (refused before anything is read)
    ]
    for args in calls:
        assert lib.bev_debug_exact_eval(*args) == INVALID, args[1:3]
        assert np.array_equal(out, before)
    assert lib.bev_debug_exact_eval(h, one, 0, px, null, null, null, null, po) == 0 and np.array_equal(out, before)
    assert lib.bev_debug_exact_eval(h, one, 16, px, null, null, null, null, po) == 0
    assert np.array_equal(out[:16].view(np.float32), ee.eval("fd_atanf", x)) and np.array_equal(out[16:], before[16:])


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_edge_frames_through_the_projection_kernels(ctx, kind):
    """MulRan, Oxford and KITTI frames made of the column-, row-edge and subnormal inputs: the product kernels that inline
    these functions give the records the oracle gives, and the columns the per-function hook gives"""
    xyzi = (cs.mulran_edge_frame, cs.oxford_edge_frame, cs.kitti_edge_frame)[kind]()
    got, want = ctx.project_xyzi(kind, xyzi), orc.project(kind, xyzi)
    assert got.tobytes() == want.tobytes(), np.flatnonzero((got["col"] != want["col"]) | (got["row"] != want["row"]))[:8]
    if kind == 0:
        word = ctx.exact_eval("project_mulran", np.arange(len(xyzi), dtype=U32), xyzi[:, 0], xyzi[:, 1])
        assert np.array_equal(word, got["row"].astype(U32) | got["col"].astype(U32) << 16)
    elif kind == 1:
        word = ctx.exact_eval("project_oxford", -xyzi[0], xyzi[1], -xyzi[2])
        assert np.array_equal(word, got["row"].astype(U32) | got["col"].astype(U32) << 16)
    else:
        filled = got["label"] != 0
        assert filled.reshape(64, 2083).any(1).sum() >= 60  # the rings were told apart
        col = ctx.exact_eval("kitti_col_xy", got["x"][filled], got["y"][filled])
        assert np.array_equal(col, got["col"][filled].astype(np.int32))
