"""ctypes binding of tests/compressor_model.c, the CPU reference of DynamicsCompressorNode for tests/test_compressor.py (the
oracle renders the node kind as silence and does not change here).  The C file is built once per test session with the system
compiler into a temporary directory — `-O2 -ffp-contract=off -fno-fast-math`, like oracle/Makefile — and loaded from there:
nothing is written into the repository."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

RQ = 128
HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULTS = dict(threshold=-24.0, knee=30.0, ratio=12.0, attack=0.003, release=0.25)  # dynamics_compressor.rs:48-63
ORDER = ("threshold", "knee", "ratio", "attack", "release")                         # WAA_PARAM_COMPRESSOR_*
RANGES = dict(threshold=(-100.0, 0.0), knee=(0.0, 40.0), ratio=(1.0, 20.0), attack=(0.0, 1.0), release=(0.0, 1.0))
_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="compressor_model_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libcompressor_model.so")
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-fPIC", "-std=gnu11", "-Wall", "-Wextra", "-fno-fast-math",
                               "-ffp-contract=off", "-shared", "-o", so, os.path.join(HERE, "compressor_model.c"), "-lm"])
        l = C.CDLL(so)
        fp, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        for name in ("model_f32", "model_f64"):
            f = getattr(l, name)
            f.argtypes = [fp, C.c_uint32, C.c_uint64, fp, u8p, C.c_float, fp]
            f.restype = None
        for name in ("model_db_to_lin", "model_lin_to_db"):
            getattr(l, name).argtypes = [C.c_float]
            getattr(l, name).restype = C.c_float
        l.model_ring_size.argtypes = [C.c_float]
        l.model_ring_size.restype = C.c_uint32
        _lib = l
    return _lib


def delay_quanta(sample_rate):
    """D: the output is the input of D quanta ago (ring - 1, dynamics_compressor.rs:253-254, 452-461)"""
    return int(lib().model_ring_size(float(sample_rate))) - 1


def param_rows(n_quanta, **kw):
    """[n_quanta, 5] f32 rows (threshold, knee, ratio, attack, release), each a scalar or an [n_quanta] array, clamped to the
    param's range like AudioParamProcessor does (param.rs:739-797)"""
    rows = np.empty((n_quanta, 5), np.float32)
    for k, name in enumerate(ORDER):
        v = np.asarray(kw.get(name, DEFAULTS[name]), np.float32)
        rows[:, k] = np.clip(v, np.float32(RANGES[name][0]), np.float32(RANGES[name][1]))
    return rows


def _run(fn, x, rows, sample_rate, live):
    x = np.ascontiguousarray(x, np.float32)
    assert x.ndim == 2 and x.shape[0] in (1, 2) and x.shape[1] % RQ == 0, x.shape
    nq = x.shape[1] // RQ
    rows = np.ascontiguousarray(rows, np.float32)
    assert rows.shape == (nq, 5), (rows.shape, nq)
    out = np.empty_like(x)
    lv = None
    if live is not None:
        lv = np.ascontiguousarray(live, np.uint8)
        assert lv.shape == (nq,)
    fp = C.POINTER(C.c_float)
    fn(x.ctypes.data_as(fp), x.shape[0], x.shape[1], rows.ctypes.data_as(fp),
       None if lv is None else lv.ctypes.data_as(C.POINTER(C.c_uint8)), float(np.float32(sample_rate)), out.ctypes.data_as(fp))
    return out


def model_f32(x, rows, sample_rate, live=None):
    """the reference's arithmetic: x [channels, frames] -> output [channels, frames]"""
    return _run(lib().model_f32, x, rows, sample_rate, live)


def model_f64(x, rows, sample_rate, live=None):
    """the same algorithm in f64 (output rounded to f32 once)"""
    return _run(lib().model_f64, x, rows, sample_rate, live)
