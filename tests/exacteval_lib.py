"""ctypes loader for tests/exacteval: the host build of csrc/bev_exact_eval.h, the dispatch that the device hook
bev_debug_exact_eval (BevContext.exact_eval) runs.  eval(name, *arrays) is what the device must equal bit for bit;
eval(..., mode="ftz") is the same under flush-to-zero / denormals-are-zero, and mode="fma" the contracted build of the same
source — the two mutants of the sharpness test, used by nothing else.  Tests only."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from bev_amd import EXACT_EVAL, EXACT_EVAL_NAMES

DIR = Path(__file__).resolve().parent / "exacteval"
_libs = {}
_IN = {"f": np.float32, "u": np.uint32, "d": np.float64}
_OUT = {"f": np.float32, "i": np.int32, "u": np.uint32, "d": np.float64, "f3": np.float32}


def build() -> None:
    r = subprocess.run(["make", "-C", str(DIR)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"make -C {DIR} failed:\n{r.stdout}")


def lib(fma: bool = False):
    name = "libexacteval_fma.so" if fma else "libexacteval.so"
    if name not in _libs:
        l = C.CDLL(str(DIR / name))
        for f in (l.ee_eval, l.ee_eval_ftz):
            f.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]
        l.ee_sig.argtypes = [C.c_int, C.c_void_p]
        _libs[name] = l
    return _libs[name]


def cpu_has_fma() -> bool:
    return bool(lib().ee_cpu_has_fma())


def libm_atanf(x) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    lib().ee_libm_atanf(C.c_size_t(len(x)), C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data))
    return out


def libm_atan2f(y, x) -> np.ndarray:
    y, x = np.ascontiguousarray(y, np.float32), np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    lib().ee_libm_atan2f(C.c_size_t(len(x)), C.c_void_p(y.ctypes.data), C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data))
    return out


def signature(fn_id: int):
    """(input kinds, 32-bit words per element, params) as the C++ dispatch states them; None for an unknown id"""
    out = np.zeros(6, np.uint8)
    if not lib().ee_sig(fn_id, out.ctypes.data):
        return None
    return "".join(" fud"[k] for k in out[:4]).strip(), int(out[4]), int(out[5])


def eval(name: str, *inputs, params=None, mode: str = "plain") -> np.ndarray:
    kinds, out_kind, n_params = EXACT_EVAL[name]
    assert len(inputs) == len(kinds), name
    arrs = [np.ascontiguousarray(a, dtype=_IN[k]) for a, k in zip(inputs, kinds)]
    n = arrs[0].shape[0]
    assert all(a.shape == (n,) for a in arrs), name
    prm = np.zeros(12, np.float32)
    if n_params:
        prm[:n_params] = np.asarray(params, np.float32).reshape(n_params)
    out = np.zeros((n, 3) if out_kind == "f3" else n, dtype=_OUT[out_kind])
    ptrs = (C.c_void_p * 4)(*[a.ctypes.data for a in arrs] + [None] * (4 - len(arrs)))
    l = lib(fma=(mode == "fma"))
    f = l.ee_eval_ftz if mode == "ftz" else l.ee_eval
    rc = f(EXACT_EVAL_NAMES.index(name), n, ptrs, prm.ctypes.data, out.ctypes.data)
    assert rc == 0, (name, rc)
    return out
