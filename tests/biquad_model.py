"""numpy model of the reference's a-rate BiquadFilterNode for tests/test_biquad_a_rate_types.py, written from
src/node/biquad_filter.rs (get_computed_freq :367-373, calculate_coefs :343-364 with the eight get_*_coefs :40-341, the
render loop :817-896) — a third leg next to the device's biquad_coef_kernel and the oracle's C restatement, sharing no
text with either.

Inputs are the values `AudioParamValues::get` hands the renderer: per param a constant, or a constant plus ONE value
block `(quantum0, values)` with values of shape (nq,) (single-valued slices) or (nq, 128) (128-value slices).  Nothing
of the automation timeline is restated; the one step of AudioParamProcessor that value blocks still go through is the
clamp to the param's range (param.rs:755-761), which only `frequency` (0 ... sample_rate / 2, biquad_filter.rs:575-581)
can reach with finite values.

The slice-length rule of :834-855: the first frame's coefficients fill the quantum, and as soon as one of the four
slices has 128 values every frame gets its own set, single-valued slices repeating their value (`iter().cycle()`).
Expanding every param to one value per frame gives exactly that — a quantum whose four slices are single-valued has
128 equal sets — so the model computes one set per frame throughout."""
import numpy as np

RQ = 128
TYPES = ("lowpass", "highpass", "bandpass", "notch", "allpass", "peaking", "lowshelf", "highshelf")  # biquad_filter.rs:377-402
DEFAULTS = dict(frequency=350.0, detune=0.0, q=1.0, gain=0.0)  # :439-450
F64_MIN_NORMAL = np.finfo(np.float64).tiny


def per_frame(param, n_quanta, default):
    """one f32 value per frame, [n_quanta * 128], of a param given as a constant or as (constant, quantum0, block)"""
    if np.isscalar(param) or param is None:
        return np.full(n_quanta * RQ, default if param is None else param, np.float32)
    const, q0, block = param
    block = np.asarray(block, np.float32)
    v = np.full((n_quanta, RQ), const, np.float32)
    n = min(block.shape[0], n_quanta - q0)
    v[q0:q0 + n] = block[:n] if block.ndim == 2 else block[:n, None]
    return v.reshape(-1)


def computed_freq(frequency, detune, ulps=0, pinned=(0.0,)):
    """get_computed_freq, f32 throughout: f * 2^(detune / 1200) where detune != 0, else f.  `ulps` = +1 / -1 moves every
    result to the next f32 above / below (the input cap of the tests: what an exp2f that is one ulp off would deliver, and
    2^29 times what an f64 ulp of sin / cos / pow does to a coefficient).  `pinned` lists the values that stay: the two
    limits of the frequency param's clamp, 0 and sample_rate / 2.  A frame that sits exactly on one of them got there by
    the clamp, which every implementation computes exactly, and then either detune == 0 and nothing was evaluated, or
    0 * 2^x is 0 whatever exp2f returns; the hardwired `f == 0` / `f == 1` sets those frames select are not continuous
    with the formulas next to them, so moving them would measure the reference's branch, not an implementation's error."""
    f, d = np.asarray(frequency, np.float32), np.asarray(detune, np.float32)
    with np.errstate(over="ignore"):
        cf = np.where(d != 0, f * np.exp2(d / np.float32(1200.0)), f).astype(np.float32)
    if ulps:
        moved = np.nextafter(cf, np.float32(np.inf if ulps > 0 else -np.inf))
        cf = np.where(np.isin(cf, np.asarray(pinned, np.float32)), cf, moved).astype(np.float32)
    return cf


def coefficients(type_, sample_rate, cf, gain, q):
    """calculate_coefs per frame: [n, 5] f64 rows (b0, b1, b2, a1, a2), from the f32 computed frequency, gain and Q"""
    assert type_ in TYPES, type_
    f0, g, q = (np.asarray(a, np.float32).astype(np.float64) for a in (cf, gain, q))
    freq = np.clip(f0 / (float(sample_rate) / 2.0), 0.0, 1.0)  # :351-352
    n = freq.shape[0]
    one, zero = np.ones(n), np.zeros(n)

    def raw(b0):  # the hardwired sets: b0 only
        return np.stack([b0 * one, zero, zero, zero, zero], axis=1)

    def norm(b0, b1, b2, a0, a1, a2):  # normalize_coefs :28-38
        scale = 1.0 / a0
        return np.stack([b0 * scale * one, b1 * scale * one, b2 * scale * one, a1 * scale, a2 * scale], axis=1)

    def pick(*branches):
        """branches: (mask, rows) in the order of the reference's if / else if chain, the last mask None"""
        out = branches[-1][1]
        for mask, rows in reversed(branches[:-1]):
            out = np.where(mask[:, None], rows, out)
        return out

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w0 = np.pi * freq
        sin_w0, cos_w0 = np.sin(w0), np.cos(w0)
        inside = (freq > 0.0) & (freq < 1.0)
        if type_ in ("lowpass", "highpass"):
            alpha = sin_w0 / (2.0 * np.power(10.0, q / 20.0))  # Q in dB for these two
            if type_ == "lowpass":  # :40-66
                beta = (1.0 - cos_w0) / 2.0
                return pick((freq == 1.0, raw(1.0)),
                            (None, norm(beta, 2.0 * beta, beta, 1.0 + alpha, -2.0 * cos_w0, 1.0 - alpha)))
            beta = (1.0 + cos_w0) / 2.0  # :68-104
            return pick((freq == 1.0, raw(0.0)), (freq == 0.0, raw(1.0)),
                        (None, norm(beta, -2.0 * beta, beta, 1.0 + alpha, -2.0 * cos_w0, 1.0 - alpha)))
        if type_ in ("bandpass", "notch", "allpass", "peaking"):
            alpha = sin_w0 / (2.0 * q)
            a0, a1, a2 = 1.0 + alpha, -2.0 * cos_w0, 1.0 - alpha
            if type_ == "bandpass":  # :106-143
                return pick((~inside, raw(0.0)), (~(q > 0.0), raw(1.0)), (None, norm(alpha, zero, -alpha, a0, a1, a2)))
            if type_ == "notch":  # :145-181
                return pick((~inside, raw(1.0)), (~(q > 0.0), raw(0.0)), (None, norm(one, -2.0 * cos_w0, one, a0, a1, a2)))
            if type_ == "allpass":  # :183-217
                return pick((~inside, raw(1.0)), (~(q > 0.0), raw(-1.0)),
                            (None, norm(1.0 - alpha, -2.0 * cos_w0, 1.0 + alpha, a0, a1, a2)))
            big_a = np.power(10.0, g / 40.0)  # peaking :219-259
            return pick((~inside, raw(1.0)), (~(q > 0.0), raw(big_a * big_a)),
                        (None, norm(1.0 + alpha * big_a, -2.0 * cos_w0, 1.0 - alpha * big_a,
                                    1.0 + alpha / big_a, -2.0 * cos_w0, 1.0 - alpha / big_a)))
        big_a = np.power(10.0, g / 40.0)
        alpha_s = sin_w0 / 2.0 * np.sqrt(2.0)
        k = 2.0 * alpha_s * np.sqrt(big_a)
        ap, am = big_a + 1.0, big_a - 1.0
        if type_ == "lowshelf":  # :261-300
            return pick((freq == 1.0, raw(big_a * big_a)), (freq == 0.0, raw(1.0)),
                        (None, norm(big_a * (ap - am * cos_w0 + k), 2.0 * big_a * (am - ap * cos_w0),
                                    big_a * (ap - am * cos_w0 - k),
                                    ap + am * cos_w0 + k, -2.0 * (am + ap * cos_w0), ap + am * cos_w0 - k)))
        return pick((freq == 1.0, raw(1.0)),  # highshelf :302-341
                    (freq > 0.0, norm(big_a * (ap + am * cos_w0 + k), -2.0 * big_a * (am + ap * cos_w0),
                                      big_a * (ap + am * cos_w0 - k),
                                      ap - am * cos_w0 + k, 2.0 * (am - ap * cos_w0), ap - am * cos_w0 - k)),
                    (None, raw(big_a * big_a)))


def recurrence(x, coefs):
    """:857-896 — x [streams, frames] f32, coefs [>= frames, 5] f64 shared by the streams; y = b0 x + b1 x1 + b2 x2 -
    a1 y1 - a2 y2 in f64 in that order, anything that is not a normal number flushed to 0, the output rounded to f32"""
    x = np.asarray(x, np.float32).astype(np.float64)
    n_streams, frames = x.shape
    out = np.empty((n_streams, frames), np.float32)
    x1 = x2 = y1 = y2 = np.zeros(n_streams)
    c = np.asarray(coefs, np.float64)
    for i in range(frames):
        b0, b1, b2, a1, a2 = c[i]
        xi = x[:, i]
        y = b0 * xi + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        y = np.where(np.isfinite(y) & (np.abs(y) >= F64_MIN_NORMAL), y, 0.0)  # !y.is_normal() -> 0
        x2, x1, y2, y1 = x1, xi, y1, y
        out[:, i] = y
    return out


def render(type_, sample_rate, x, frequency=None, detune=None, q=None, gain=None, ulps=0):
    """x [streams, frames] f32 through one BiquadFilterNode whose params are the same for every stream"""
    frames = x.shape[-1]
    nq = (frames + RQ - 1) // RQ
    f = per_frame(frequency, nq, DEFAULTS["frequency"])
    f = np.clip(f, np.float32(0.0), np.float32(sample_rate / 2.0))  # AudioParamProcessor's clamp (see the module docstring)
    cf = computed_freq(f, per_frame(detune, nq, DEFAULTS["detune"]), ulps, pinned=(0.0, sample_rate / 2.0))
    co = coefficients(type_, sample_rate, cf, per_frame(gain, nq, DEFAULTS["gain"]), per_frame(q, nq, DEFAULTS["q"]))
    return recurrence(x, co)
