"""numpy model of the reference's OscillatorNode for tests/test_oscillator_kernels.py, written from src/node/oscillator.rs
alone (process and generate_sample :364-558, the five generate_* :571-637, poly_blep :647-659 with is_test = false, both
unroll_phase forms :661-675, the sine table :16-28, get_computed_freq :30-32) — a third leg next to the device's three
oscillator kernels and the oracle's C restatement, sharing no text with either.

Inputs are what `AudioParamValues::get` hands the renderer, expanded to one f32 per frame: a quantum whose slices are
single-valued takes the scalar branch of process (:426-446), whose arithmetic per frame is that of the per-frame branch
(:447-459; generate_sample with every frame inside [start, stop) is the two lines of the fast path), so one loop serves
both.  The loop runs over frames and is vectorised over contexts: 67 contexts cost what one does.

Where the model is deliberately not the reference's arithmetic: table interpolation is evaluated in f64 from the f32
`k` and rounded once (the reference: f32 `1 - k`, an f32 product and one f32 fma), and `t.mul_add(t, t)` is t * t + t.
Both stay below the rounding term U of the tests' bound.  The sine table is built as :25 builds it — the argument in
f32 arithmetic — with the sine of that f32 argument taken in f64 and rounded, so an entry may sit one ulp from a libm
sinf.

Hazard (reported as Result.phase_one, asserted empty by the tests): the single wrap :662-670 maps a phase in
[-2^-54, 0) to exactly 1.0 (phase + 1. rounds up), and the table forms then index one past the table (the reference
panics).  It takes |phase + incr| < 2^-54 with the sum negative."""
from dataclasses import dataclass

import numpy as np

RQ = 128
TYPES = ("sine", "square", "sawtooth", "triangle", "custom")
SINE_LEN, CUSTOM_LEN = 2048, 8192


def sine_table():
    x = np.arange(SINE_LEN, dtype=np.float32)
    arg = x * np.float32(2.0) * np.float32(np.pi) * (np.float32(1.0) / np.float32(SINE_LEN))  # f32 products, left to right
    assert arg.dtype == np.float32
    return np.sin(arg.astype(np.float64)).astype(np.float32)


def unroll_phase(p):  # :662-670
    return np.where(p >= 1.0, p - 1.0, np.where(p < 0.0, p + 1.0, p))


def unroll_phase_unbounded(p):  # f64::rem_euclid(1.): r = p % 1 (sign of p); r < 0 -> r + 1
    r = np.fmod(p, 1.0)
    return np.where(r < 0.0, r + 1.0, r)


def poly_blep(t, dt):  # :647-659, is_test = false
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lo = t / dt
        lo = lo + lo - lo * lo - 1.0
        hi = (t - 1.0) / dt
        hi = (hi * hi + hi) + hi + 1.0
    return np.where(t < dt, lo, np.where(t > 1.0 - dt, hi, 0.0))


def _table(table, phase):
    n = table.shape[0]
    position = phase * float(n)
    floored = np.floor(position)
    prev = floored.astype(np.int64)
    nxt = np.where(prev + 1 == n, 0, prev + 1)
    k = (position - floored).astype(np.float32).astype(np.float64)
    t = table.astype(np.float64)
    return t[prev % n] * (1.0 - k) + t[nxt % n] * k  # (% n: see `phase_one`; never taken in a checked case)


def waveform(type_, table, phase, incr):
    """generate_waveform_sample :561-637 in f64, before the cast to f32"""
    if type_ in ("sine", "custom"):
        return _table(table, phase)
    if type_ == "sawtooth":
        ph = unroll_phase(phase + 0.5)
        return 2.0 * ph - 1.0 - poly_blep(ph, incr)
    if type_ == "square":
        s = np.where(phase < 0.5, 1.0, -1.0) + poly_blep(phase, incr)
        return s - poly_blep(unroll_phase(phase + 0.5), incr)
    assert type_ == "triangle", type_
    s = -4.0 * phase + 2.0
    return np.where(s > 1.0, 2.0 - s, np.where(s < -1.0, -2.0 - s, s))


@dataclass
class Result:
    samples64: np.ndarray  # [n_ctx, frames] f64, the sample before `as f32` (0 where silent)
    samples: np.ndarray    # [n_ctx, frames] f32
    audible: np.ndarray    # [n_ctx, frames] bool: inside [start, stop) on the renderer's clock and inside Nyquist
    active: np.ndarray     # [n_ctx, frames] bool: inside [start, stop) (the phase advances)
    phase: np.ndarray      # [n_ctx, frames] f64: the serial phase the sample was taken at (NaN where not active)
    incr: np.ndarray       # [n_ctx, frames] f64: computed_freq / sample_rate
    lipschitz: np.ndarray  # [n_ctx, frames] f64: L_f, |d sample / d phase| at that frame's increment
    near_edge: np.ndarray  # [n_ctx, frames] bool
    phase_one: np.ndarray  # [n_ctx, frames] bool: audible frames whose phase is exactly 1.0 (see the module docstring)
    first: np.ndarray      # [n_ctx] first active frame, -1 if never
    ratio: np.ndarray      # [n_ctx] (time of that frame - start) / dt, 0 when it starts on the frame
    dphi: float            # 8 * frames * 2^-53


def render(type_, sample_rate, length, frequency, detune, start, stop, table=None):
    """frequency, detune: [n_ctx, n_quanta * 128] f32; start, stop: [n_ctx] seconds (f64::MAX: never).  `table`: the
    finished 8192-point table of `custom`."""
    assert type_ in TYPES, type_
    f32, d32 = np.asarray(frequency), np.asarray(detune)
    assert f32.dtype == np.float32 and d32.dtype == np.float32 and f32.shape == d32.shape
    n_ctx, padded = f32.shape
    nq = (length + RQ - 1) // RQ
    assert padded == nq * RQ
    if type_ == "custom":
        table = np.asarray(table)
        assert table.dtype == np.float32 and table.shape == (CUSTOM_LEN,)
    else:
        table = sine_table() if type_ == "sine" else None
    sr = float(sample_rate)
    dt = 1.0 / sr
    nyquist = sr / 2.0
    computed = f32.astype(np.float64) * np.exp2(d32.astype(np.float64) / 1200.0)  # get_computed_freq
    incr_all = computed / sr
    outside_all = np.abs(computed) >= nyquist
    start_time = np.array(start, np.float64)
    stop_time = np.array(stop, np.float64)
    assert start_time.shape == stop_time.shape == (n_ctx,)
    phase = np.zeros(n_ctx)
    started = np.zeros(n_ctx, bool)
    s64 = np.zeros((n_ctx, padded))
    act = np.zeros((n_ctx, padded), bool)
    ph_at = np.full((n_ctx, padded), np.nan)
    first_at = np.full(n_ctx, -1, np.int64)
    ratio_at = np.zeros(n_ctx)
    on_frame = np.zeros((n_ctx, padded), bool)  # the first active frame of a context that starts on a frame
    for q in range(nq):
        block_time = float(q * RQ) / sr  # render/thread.rs: current_frame as f64 / sample_rate as f64
        next_block_time = block_time + dt * float(RQ)
        live = ~((stop_time <= block_time) | (start_time >= next_block_time))  # :382-406
        if not live.any():
            continue
        past = live & ~started & (start_time < block_time)  # :419-421
        start_time = np.where(past, block_time, start_time)
        current_time = block_time
        for k in range(RQ):
            f = q * RQ + k
            incr, outside = incr_all[:, f], outside_all[:, f]
            active = live & ~((current_time < start_time) | (current_time >= stop_time))  # :521-524
            begins = active & ~started
            late = begins & (current_time > start_time)  # :530-537
            ratio = (current_time - start_time) / dt
            p0 = incr * ratio
            phase = np.where(late, np.where(outside, unroll_phase_unbounded(p0), unroll_phase(p0)), phase)
            first_at = np.where(begins, f, first_at)
            ratio_at = np.where(late, ratio, ratio_at)
            on_frame[:, f] = begins & ~late
            started = started | begins
            act[:, f] = active
            ph_at[:, f] = np.where(active, phase, np.nan)
            s64[:, f] = np.where(active & ~outside, waveform(type_, table, phase, incr), 0.0)  # :542-549
            nxt = phase + incr
            phase = np.where(active, np.where(outside, unroll_phase_unbounded(nxt), unroll_phase(nxt)), phase)  # :551-555
            current_time = current_time + dt
    audible = act & ~outside_all
    dphi = 8.0 * float(length) * 2.0 ** -53
    with np.errstate(divide="ignore"):
        if type_ == "triangle":
            lip = np.full_like(incr_all, 4.0)
        elif type_ == "sawtooth":
            lip = 2.0 + 2.0 / np.abs(incr_all)
        elif type_ == "square":
            lip = np.where(incr_all > 0.0, 4.0 / np.abs(incr_all), 0.0)
        else:
            step = np.abs(np.diff(np.concatenate([table, table[:1]]).astype(np.float64))).max()
            lip = np.full_like(incr_all, float(table.shape[0]) * step)
    edges = {"sawtooth": (0.5,), "square": (0.0, 0.5, 1.0)}.get(type_, ())
    near = np.zeros_like(audible)
    with np.errstate(invalid="ignore"):
        for e in edges:
            near |= audible & (incr_all <= 0.0) & (np.abs(ph_at - e) <= 64.0 * dphi)
    near &= ~on_frame
    out = s64[:, :length]
    cut = lambda a: a[:, :length]
    return Result(samples64=out, samples=out.astype(np.float32), audible=cut(audible), active=cut(act), phase=cut(ph_at),
                  incr=cut(incr_all), lipschitz=cut(lip), near_edge=cut(near),
                  phase_one=cut(audible & (ph_at == 1.0)), first=first_at, ratio=ratio_at, dphi=dphi)


def gain_upmix(samples, gains, channels=2):
    """GainNode (gain.rs:160-188, one value per quantum: mute at |g| <= 1e-6, pass-through at |1 - g| <= 1e-6, else the f32
    product) and the mono -> `channels` up-mix of the destination (speakers: the mono signal in every channel);
    samples [n_ctx, frames] f32, gains [n_ctx] f32 -> [n_ctx, channels, frames] f32"""
    x, g = np.asarray(samples, np.float32), np.asarray(gains, np.float32)[:, None]
    thr = np.float32(1e-6)
    y = np.where(np.abs(g) <= thr, np.float32(0.0), np.where(np.abs(np.float32(1.0) - g) <= thr, x, x * g)).astype(np.float32)
    return np.repeat(y[:, None, :], channels, axis=1)
