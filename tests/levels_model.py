"""numpy model of the output levels (waa_output_levels / waa_output_level_series, include/waa_hip_device.h), written from the
definitions and not from the kernels; tests/test_output_levels.py compares the device with it bit for bit.

A row is one (instance, output channel) of L samples in n_q = ceil(L / 128) quanta.  Everything is decided on the sample's 32
bits: a = bits & 0x7fffffff, e = a >> 23; e == 255 is non-finite, e == 0 zero or denormal.

  p_q   the f32 whose bits are the unsigned maximum of `a` over the quantum's frames with e != 255 (0 when there is none)
  e_q   f64: s_j = (double)x_j * (double)x_j where 1 <= e <= 254, +0.0 otherwise (past the end, non-finite, zero, denormal), summed by
        the adjacent-pairs tree in index order — t0[k] = s[2k] + s[2k+1], t1[k] = t0[2k] + t0[2k+1], ... seven levels
  peak  max p_q
  sum_sq   blocks of 64 consecutive quanta (a missing quantum is +0.0), b_m = the same tree over the block's 64 e_q (six levels),
           sum_sq = (...((0.0 + b_0) + b_1) + ...)
  n_nonfinite / first_nonfinite   the frames with e == 255 and the smallest of them (UINT64_MAX: none)
  n_clipped   frames with e != 255 whose f32 product v = x * 32768 has v > 32767 or v < -32768

The trees are explicit halvings (a[..., 0::2] + a[..., 1::2]); np.sum, whose order is its own, appears nowhere.  A denormal never
reaches an f32 operation whose result could depend on flushing: it is +0.0 for the energy, its own bits for the peak, and its
product with 32768 is far from a clamp edge flushed or not.
"""
import numpy as np

RQ = 128
BLOCK = 64
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)

STATS_DTYPE = np.dtype([("sum_sq", np.float64), ("n_nonfinite", np.uint64), ("first_nonfinite", np.uint64), ("n_clipped", np.uint64),
                        ("peak", np.float32)])


def pair_tree(a):
    """root of the adjacent-pairs tree over the last axis (a power of two long)"""
    a = np.asarray(a, np.float64)
    assert a.shape[-1] & (a.shape[-1] - 1) == 0 and a.shape[-1] > 0
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def butterfly(a):
    """what every lane of an xor-butterfly (masks 1, 2, 4, ...) over the last axis ends with: v[l] = v[l] + v[l ^ m]"""
    v = np.array(a, np.float64)
    n = v.shape[-1]
    lanes = np.arange(n)
    m = 1
    while m < n:
        v = v + v[..., lanes ^ m]
        m <<= 1
    return v


def _padded(rows, multiple):
    """rows [..., L] padded with +0.0 to a multiple (bits: +0.0 has e == 0 and adds nothing anywhere)"""
    L = rows.shape[-1]
    n = -(-L // multiple) * multiple
    out = np.zeros(rows.shape[:-1] + (n,), rows.dtype)
    out[..., :L] = rows
    return out


def series(rows):
    """rows float32 [..., L] -> (p_q float32 [..., n_q], e_q float64 [..., n_q])"""
    rows = np.ascontiguousarray(rows, np.float32)
    x = _padded(rows, RQ)
    x = x.reshape(x.shape[:-1] + (x.shape[-1] // RQ, RQ))
    a = x.view(np.uint32) & np.uint32(0x7FFFFFFF)
    e = a >> np.uint32(23)
    p = np.where(e != 255, a, np.uint32(0)).max(axis=-1).astype(np.uint32).view(np.float32)
    xd = x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.where((e >= 1) & (e <= 254), xd * xd, 0.0)
    return p, pair_tree(s)


def clipped(rows):
    """bool [..., L]: the samples the packer's clamp changes"""
    rows = np.ascontiguousarray(rows, np.float32)
    e = (rows.view(np.uint32) & np.uint32(0x7FFFFFFF)) >> np.uint32(23)
    with np.errstate(invalid="ignore", over="ignore"):
        v = rows * np.float32(32768.0)
        assert v.dtype == np.float32
        return (e != 255) & ((v > np.float32(32767.0)) | (v < np.float32(-32768.0)))


def stats(rows):
    """rows float32 [..., L] -> STATS_DTYPE [...]"""
    rows = np.ascontiguousarray(rows, np.float32)
    L = rows.shape[-1]
    out = np.zeros(rows.shape[:-1], STATS_DTYPE)
    out["first_nonfinite"] = NONE
    if L == 0:
        return out
    p, e_q = series(rows)
    out["peak"] = p.view(np.uint32).max(axis=-1).astype(np.uint32).view(np.float32)
    eb = _padded(e_q, BLOCK)
    b = pair_tree(eb.reshape(eb.shape[:-1] + (eb.shape[-1] // BLOCK, BLOCK)))
    total = np.zeros(rows.shape[:-1], np.float64)
    for m in range(b.shape[-1]):  # ascending and sequential
        total = total + b[..., m]
    out["sum_sq"] = total
    nonfinite = ((rows.view(np.uint32) & np.uint32(0x7FFFFFFF)) >> np.uint32(23)) == 255
    out["n_nonfinite"] = np.count_nonzero(nonfinite, axis=-1)
    first = np.argmax(nonfinite, axis=-1).astype(np.uint64)
    out["first_nonfinite"] = np.where(nonfinite.any(axis=-1), first, NONE)
    out["n_clipped"] = np.count_nonzero(clipped(rows), axis=-1)
    return out


def normalize_gains(peak, target):
    """gain[i] = float32(target) / max_c peak[i, c] (an f32 division), 1 where that peak is 0"""
    top = np.asarray(peak, np.float32).max(axis=1)
    gain = np.ones(top.shape, np.float32)
    np.divide(np.float32(target), top, out=gain, where=top > 0)
    return gain
