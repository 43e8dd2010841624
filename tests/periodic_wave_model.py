"""A numpy model of PeriodicWave::new's table, written from the reference's src/periodic_wave.rs:164-189 alone, and the bound a
table computed in f32 is held to (tests/test_periodic_wave_per_instance.py).

    for i in 0 .. 8192:  phase = 2 pi * i / 8192 (f32);  sample = 0
        for j in 1 .. n:  rad = phase * j;  sample += re[j] * cos(rad) + im[j] * sin(rad)      (every operation rounded to f32)
    unless disable_normalization:  max = max |sample|;  if max > 0: every sample *= 1 / max

`table_f32` is that, in the reference's order, with numpy's f32 cos / sin standing for the host's.  `table_f64` takes the SAME
f32 phase and rad values, widened, and does everything else in f64: cos / sin, the products, the sum, the maximum and the
scaling.  It is what an f32 table is an approximation OF, so the bound below covers only what f32 arithmetic adds.

The bound, derived and not measured.  S = sum over j >= 1 of |re_j| + |im_j|, n the (padded) number of coefficients.  An
un-normalised entry computed in f32 lies within

    B(c) = S * (c * 2^-23 + (n + 2) * 2^-24)

of table_f64's: c ulp of a value <= 1 (2^-23 at most) for each cos / sin, scaled by its coefficient; one rounding (2^-24 relative)
per product, of a value <= |coefficient|; one for the term's sum, <= |re_j| + |im_j|; one per accumulation, of a partial sum <= S,
n - 1 of them.  Summed: S * (c 2^-23 + 2^-24 + 2^-24 + (n - 1) 2^-24) <= B(c), second-order terms aside.  c = 1 for a libm that
rounds to one ulp, c = 4 for the device: the OpenCL full-profile limit for sin and cos, which the ROCm device library meets.
Zero padding adds terms that are exactly +0, so a padded set's table is the unpadded one's; its bound takes the padded n.

With M = max |table_f64| and eps = B / M, the f32 maximum lies within B of M, its reciprocal within eps (1 + eps) relatively, and a
normalised entry (|entry / M| <= 1) within  eps + eps (1 + eps) + 2^-24 (the reciprocal's rounding) + 2^-24 (the product's)
<= 2 eps (1 + eps) + 2^-22  of table_f64's.  The linearisation wants eps small: the tests assert eps <= 1e-3 for their sets."""
import numpy as np

LEN = 8192
F32 = np.float32


def _coefs(real, imag):
    if real is None and imag is None:
        raise ValueError("real and imag are both None")
    n = len(real if real is not None else imag)
    re = np.zeros(n, F32) if real is None else np.asarray(real, F32)
    im = np.zeros(n, F32) if imag is None else np.asarray(imag, F32)
    assert re.shape == im.shape == (n,) and n >= 2
    return re, im


def _phase():
    pi_2 = F32(2.0) * F32(3.14159265358979323846)
    return (pi_2 * np.arange(LEN, dtype=F32)) / F32(LEN)


def table_f32(real, imag, normalize=True):
    """the reference's table in its f32 order of operations"""
    re, im = _coefs(real, imag)
    phase = _phase()
    sample = np.zeros(LEN, F32)
    for j in range(1, re.size):
        rad = phase * F32(j)
        contrib = re[j] * np.cos(rad) + im[j] * np.sin(rad)
        sample = sample + contrib
    assert sample.dtype == F32
    if normalize:
        peak = F32(np.abs(sample).max())
        if peak > 0:
            sample = sample * (F32(1.0) / peak)
    return sample


def table_f64(real, imag, normalize=True):
    """the same f32 phase and rad values, everything behind them in f64"""
    re, im = _coefs(real, imag)
    phase = _phase()
    sample = np.zeros(LEN, np.float64)
    for j in range(1, re.size):
        rad = (phase * F32(j)).astype(np.float64)
        sample += np.float64(re[j]) * np.cos(rad) + np.float64(im[j]) * np.sin(rad)
    if normalize:
        peak = np.abs(sample).max()
        if peak > 0:
            sample = sample * (1.0 / peak)
    return sample


def coefficient_sum(real, imag):
    re, im = _coefs(real, imag)
    return float(np.abs(re[1:].astype(np.float64)).sum() + np.abs(im[1:].astype(np.float64)).sum())


def raw_bound(real, imag, c, n=None):
    """B(c) for an un-normalised entry; n: the padded coefficient count (default: the set's own)"""
    re, _ = _coefs(real, imag)
    n = re.size if n is None else n
    assert n >= re.size
    return coefficient_sum(real, imag) * (c * 2.0 ** -23 + (n + 2) * 2.0 ** -24)


def epsilon(real, imag, c, n=None):
    """B(c) / max |table_f64| (0 for an all-zero set)"""
    peak = float(np.abs(table_f64(real, imag, normalize=False)).max())
    return raw_bound(real, imag, c, n) / peak if peak > 0 else 0.0


def bound(real, imag, normalize, c, n=None):
    """what an entry of a table computed in f32 may differ from table_f64(real, imag, normalize) by"""
    if not normalize:
        return raw_bound(real, imag, c, n)
    eps = epsilon(real, imag, c, n)
    if eps == 0.0:
        return 0.0  # an all-zero set: a table of zeros, not scaled
    return 2.0 * eps * (1.0 + eps) + 2.0 ** -22
