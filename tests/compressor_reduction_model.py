"""ctypes binding of tests/compressor_reduction_model.c, the CPU reference of DynamicsCompressorNode.reduction() for
tests/test_compressor_reduction.py.  Built like tests/compressor_model.py builds its C file: once per test session with the system
compiler into a temporary directory — `-O2 -ffp-contract=off -fno-fast-math`, like oracle/Makefile — and loaded from there; nothing
is written into the repository.  `params` and `live` are compressor_model's (param_rows, a byte per quantum)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

RQ = 128
HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="compressor_reduction_model_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libcompressor_reduction_model.so")
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-fPIC", "-std=gnu11", "-Wall", "-Wextra", "-fno-fast-math",
                               "-ffp-contract=off", "-shared", "-o", so, os.path.join(HERE, "compressor_reduction_model.c"), "-lm"])
        l = C.CDLL(so)
        fp, dp, u8p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        l.reduction_f32.argtypes = [fp, C.c_uint32, C.c_uint64, fp, u8p, C.c_float, fp, fp]
        l.reduction_f64.argtypes = [fp, C.c_uint32, C.c_uint64, fp, u8p, C.c_float, dp, dp]
        l.reduction_f32.restype = l.reduction_f64.restype = None
        _lib = l
    return _lib


def _run(fn, dtype, x, rows, sample_rate, live):
    x = np.ascontiguousarray(x, np.float32)
    assert x.ndim == 2 and x.shape[0] in (1, 2) and x.shape[1] % RQ == 0, x.shape
    nq = x.shape[1] // RQ
    rows = np.ascontiguousarray(rows, np.float32)
    assert rows.shape == (nq, 5), (rows.shape, nq)
    lv = None
    if live is not None:
        lv = np.ascontiguousarray(live, np.uint8)
        assert lv.shape == (nq,)
    red, makeup = np.empty(nq, dtype), np.empty(nq, dtype)
    fp = C.POINTER(C.c_float)
    op = C.POINTER(C.c_float if dtype == np.float32 else C.c_double)
    fn(x.ctypes.data_as(fp), x.shape[0], x.shape[1], rows.ctypes.data_as(fp),
       None if lv is None else lv.ctypes.data_as(C.POINTER(C.c_uint8)), float(np.float32(sample_rate)), red.ctypes.data_as(op),
       makeup.ctypes.data_as(op))
    return red, makeup


def reduction_f32(x, rows, sample_rate, live=None):
    """the reference's arithmetic: x [channels, frames] -> (red [n_quanta] f32, makeup [n_quanta] f32)"""
    return _run(lib().reduction_f32, np.float32, x, rows, sample_rate, live)


def reduction_f64(x, rows, sample_rate, live=None):
    """the same algorithm in f64 -> (red [n_quanta] f64, makeup [n_quanta] f64)"""
    return _run(lib().reduction_f64, np.float64, x, rows, sample_rate, live)
