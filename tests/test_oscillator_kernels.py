"""The three phase constructions of the OscillatorNode on the device — osc_par_kernel (closed-form phase from the host's
replay), osc_scan_kernel<0/1> (prefix sum over 8 time segments) and osc_kernel (the serial accumulator, WAA_OSC_EXACT=1) —
and the oracle, against tests/oscillator_model.py: a numpy model written from the reference's src/node/oscillator.rs alone.
Three legs: oracle against model (CPU), device against model and device against oracle (GPU), every plan line asserted.
Per-frame and per-quantum values are value blocks (AudioParam.set_block, 2-D and 1-D), so all legs are handed the same f32
values and none restates automation.

Bound per frame, device or oracle against the model's f32 sample:  |diff| <= U + L_f * dphi, with
  dphi = 8 * frames * 2^-53   (one rounded addition per frame in the reference's sum, one in the device's whatever its
                               order, up to three ulp of exp2 on each side scaled by |incr| <= 0.5; the rest is margin),
  L_f  the Lipschitz constant of the sample in the phase at that frame's increment: triangle 4, sawtooth 2 + 2 / |incr|,
       square 4 / |incr| for incr > 0 and 0 otherwise, a table len * max |table[i + 1] - table[i]|,
  U    = 2^-23 * max(1, |model|) for square, sawtooth and triangle (one f32 ulp: an implementation may contract
       t + t - t * t - 1 into an fma), 3 * 2^-24 * peak(table) for sine and custom (the table entry's ulp plus the
       roundings of the interpolation).
Where the model is silent — before the start, after the stop, at and outside Nyquist — device and oracle are exactly 0.
Device against oracle: the same bound doubled.  No frame is left out of any comparison.  Behind a GainNode (post_ops) the
bound is |g| times the above plus 2^-24 (the f32 product's rounding on both sides, values below 1); a muted context is 0.

Input conditions, asserted on the model alone for every case (test_input_conditions): `near_edge` is empty (no audible
frame with incr <= 0 within 64 * dphi of a hard step: sawtooth at phase 0.5, square at 0, 0.5 and 1; for dt <= 0 the
reference's polyBLEP is inert; a first frame that starts on a frame is exempt, its phase is exactly 0 in every form);
L_f * dphi <= U at every audible frame; no audible frame has 0 < |incr| < 1e-9 — there the bound says nothing, and at
|phase + incr| < 2^-54 the reference's single wrap yields a phase of exactly 1.0 and indexes past its table (it panics;
oscillator_model's Result.phase_one, asserted empty).  One condition more: apart from inputs that are
exactly +-Nyquist with a detune of 0 (2^0 is exact everywhere), no computed frequency lies within 1e-9 of Nyquist, relatively
— there one ulp of exp2 would decide between a sample and silence.  Sign changes of the frequency happen between two frames.

What the conditions moved:
 * `const`, context 2: 0 Hz for sine, triangle and custom; -5 Hz for square and sawtooth.  At incr = 0 the sawtooth's L_f is
   infinite as stated, and the square sits on its hard step at phase 0 on every frame, not only on the first.
 * `freq_a_rate` / `freq_a_rate_d_k_rate` / `both_a_rate`: the floor of the per-frame frequency is 5 Hz where the context's detune is >= 0, and 8 Hz
   under -1200 cents / under a detune that changes (5 Hz * 2^-1 = 2.5 Hz: square L_f * dphi = 1.4 U at 2441 frames).
 * `per_quantum`: the detune block steps to 2401 and 2500 cents, not to 2400 (6 kHz * 2^2 is Nyquist only if exp2 is exact).

Segment geometry.  The kernels run over the PADDED length (a multiple of the 2048-frame tile, read from the plan's first
line in test_plans), so the scan kernel always sees 8 * tiles groups of 256 frames: per_seg = tiles groups, every segment is
full, and "fewer groups than segments", a short or empty last segment and g_begin past the end cannot be planned.  What
remains, and is covered: segments that hold only padding, or lie wholly before the start or after the stop (all their
increments inactive, `seg_phase` 0):
  640 frames  -> 2048 padded, 1 group per segment:  segment 2 holds the end, segments 3 - 7 only padding;
  2441 frames -> 4096 padded, 2 groups per segment: segment 4 holds the end, segments 5 - 7 only padding;
  4225 frames -> 6144 padded, 3 groups per segment: segment 5 holds the end, segments 6 - 7 only padding.

WAA_WRITE_PROFILES=1 makes the GPU session write profiles/oscillator_parity.json: per case, waveform and kernel the worst
|diff| / bound of both device legs and the share of frames that are bit-identical to the oracle (reported, not asserted)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import oscillator_model as om
import web_audio_api_rs_amd as waa
from graphs import assert_all_finite, assert_le

RQ = 128
SR = 48000.0
NYQ = SR / 2.0
NEVER = float(np.finfo(np.float64).max)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PADDED = {640: 2048, 2441: 4096, 4225: 6144}  # render length -> padded length (see the module docstring)
PLAN_LINE = {"par": "time-parallel, closed-form phase", "scan": "prefix-sum phase", "exact": "lane per instance, serial phase"}
MODE = {"const": "const", "k": "k-rate", "a": "a-rate"}
ALL5 = om.TYPES
_FIGURES = {}


def _pl(n, knots):
    """piecewise linear through (frame, value) knots, one f32 per frame, the last value held"""
    return np.interp(np.arange(n), [k[0] for k in knots], [k[1] for k in knots]).astype(np.float32)


_TABLE = []


def custom_table():
    """a finished 8192-point table: three harmonics plus white noise (so that neighbouring entries differ), peak 1"""
    if not _TABLE:
        i = np.arange(om.CUSTOM_LEN, dtype=np.float64) / om.CUSTOM_LEN
        t = np.sin(2 * np.pi * i) + 0.4 * np.cos(6 * np.pi * i) + 0.2 * np.sin(14 * np.pi * i + 1.0)
        t += 0.05 * np.random.default_rng(0x05C).uniform(-1.0, 1.0, om.CUSTOM_LEN)
        t = (t / np.abs(t).max()).astype(np.float32)
        t.setflags(write=False)
        _TABLE.append(t)
    return _TABLE[0]


def _freq_block(n, floor):
    """+900 -> -700 Hz in one step, through -2 kHz and +2 kHz (the signs change between two frames), down to `floor`, up to 4 kHz"""
    return _pl(n, [(0, 900.0), (400, 1200.0), (401, -700.0), (800, -2000.0), (1100, -300.0), (1101, 2000.0), (1500, floor),
                   (1900, floor), (2440, 4000.0)])


def _detune_next_group(n):
    """6 kHz out through Nyquist (2400 cents) in group 1, back in group 2; out in group 5, back in group 6"""
    return _pl(n, [(0, 0.0), (200, 1200.0), (300, 2613.0), (520, 2613.0), (560, 1807.0), (900, -1200.0), (1250, 0.0), (1300, 2517.0),
                   (1540, 2517.0), (1600, 600.0), (2440, -300.0)])


def _detune_segments_later(n):
    """out in segment 0 (frames 0 - 511) and up to 6 kHz * 2^4.5 = 136 kHz (muted increments of 2.8: rem_euclid, not the single
    wrap), back in segment 3; out again in segment 3, back in segment 4"""
    return _pl(n, [(0, 0.0), (200, 1200.0), (300, 5413.0), (1690, 5413.0), (1710, 1500.0), (1900, 1500.0), (1950, 3011.0),
                   (2300, 3011.0), (2330, 100.0), (2440, 0.0)])


def _per_quantum_frequency():
    nq = np.float32(NYQ)
    below = np.nextafter(nq, np.float32(0.0))
    v = [300.0] * 3 + [23999.0] * 2 + [-700.0] * 3 + [nq, below] + [5.0] * 2 + [-nq, -below] + [300.0] * 6
    return np.asarray(v, np.float32)


def _per_quantum_detune():
    """6 kHz up to 24 kHz * 2^(1/12) (2500 cents) and back"""
    return np.asarray([0.0] * 4 + [1200.0, 2401.0] + [2500.0] * 3 + [2399.0, 1200.0] + [0.0] * 9, np.float32)


CASES = {  # name -> (length, waveforms, kernels)
    "const_on_frame": (640, ALL5, ("par", "exact")),
    "const_sub_sample": (640, ALL5, ("par", "exact")),
    "const_in_one_quantum": (640, ALL5, ("par", "exact")),
    "per_quantum": (2441, ALL5, ("par", "exact")),
    "freq_a_rate": (2441, ALL5, ("scan", "exact")),
    "freq_a_rate_d_k_rate": (2441, ALL5, ("scan", "exact")),
    "detune_a_rate_f_const": (2441, ALL5, ("scan", "exact")),
    "detune_a_rate_f_k_rate": (2441, ALL5, ("scan", "exact")),
    "both_a_rate": (2441, ALL5, ("scan", "exact")),
    "segments": (4225, ("sawtooth", "custom"), ("scan",)),
    "many_contexts": (640, ("sine", "square"), ("exact", "par")),
    "post_ops_par": (640, ("triangle",), ("par",)),
    "post_ops_scan": (640, ("triangle",), ("scan",)),
}
CASE_TYPES = [(c, t) for c, (_, types, _k) in CASES.items() for t in types]
DEVICE_CASES = [(k, c, t) for c, (_, types, kernels) in CASES.items() for t in types for k in kernels]


def case_spec(case, type_):
    """length, n_ctx, frequency / detune as (kind, one entry per context) with kind const (a float), k (one f32 per quantum)
    or a (one f32 per frame of the quanta), start / stop in seconds per context (stop None: never), gains (post_ops) or None"""
    length = CASES[case][0]
    nq = (length + RQ - 1) // RQ
    n = nq * RQ
    at = lambda frame: frame / SR
    s = SimpleNamespace(length=length, gains=None)
    if case.startswith("const_"):
        # contexts 3 and 4 equal context 0 in start, stop, frequency and detune: they share its replay row (tq_row)
        third = -5.0 if type_ in ("square", "sawtooth") else 0.0
        s.frequency = ("const", [441.0, -333.3, third, 441.0, 441.0])
        s.detune = ("const", [0.0, 50.0, 0.0, 0.0, 0.0])
        start, stop = {"const_on_frame": (at(256.0), None), "const_sub_sample": (at(300.5), None),
                       "const_in_one_quantum": (at(130.37), at(190.2))}[case]
        s.start, s.stop = [start] * 5, [stop] * 5
    elif case == "per_quantum":
        f, d = _per_quantum_frequency(), _per_quantum_detune()
        assert f.size == d.size == nq
        s.frequency = ("k", [f, np.full(nq, 6000.0, np.float32), f[::-1].copy()])
        d2 = np.where(np.arange(nq) % 3 == 1, 3.5, -300.0)
        d2[[2, 5]] = 9600.0  # 300 Hz * 2^8 = 76.8 kHz: a muted increment of 1.6, where rem_euclid and the single wrap differ
        s.detune = ("k", [np.zeros(nq, np.float32), d, d2.astype(np.float32)])
        s.start, s.stop = [at(130.37)] * 3, [at(2000.5)] * 3
    elif case == "freq_a_rate":
        f0 = _freq_block(n, 5.0)  # context 0 (detune exactly 0): four frames at Nyquist, one ulp inside it, and the same below 0
        below = np.nextafter(np.float32(NYQ), np.float32(0.0))
        f0[1950:1954] = [NYQ, below, -NYQ, -below]
        s.frequency = ("a", [f0, _freq_block(n, 5.0), _freq_block(n, 8.0)])
        s.detune = ("const", [0.0, 700.0, -1200.0])  # the det_mul path
        s.start, s.stop = [at(130.37)] * 3, [at(2300.5)] * 3
    elif case == "freq_a_rate_d_k_rate":  # the reverse of detune_a_rate_f_k_rate: one detune value per quantum under a per-frame frequency
        q = np.arange(nq)
        d = (100.0 * ((q * 7) % 13 - 6)).astype(np.float32)  # -600 ... 600 cents, a new value every quantum
        out = d.copy()
        out[17:19] = 3300.0  # 2 - 4 kHz * 2^2.75: out through Nyquist inside quantum 18
        s.frequency = ("a", [_freq_block(n, 8.0)] * 3)
        s.detune = ("k", [d, d[::-1].copy(), out])
        s.start, s.stop = [at(130.37)] * 3, [at(2420.5)] * 3
    elif case.startswith("detune_a_rate"):
        if case.endswith("f_const"):
            s.frequency = ("const", [6000.0] * 3)
        else:  # one value per quantum around 6 kHz, two quanta at -6 kHz
            q = np.arange(nq)
            f = np.where((q == 7) | (q == 8), -6000.0, 6000.0 + 250.0 * (q % 5 - 2)).astype(np.float32)
            s.frequency = ("k", [f, f, f[::-1].copy()])
        d0 = _detune_next_group(n)
        s.detune = ("a", [d0, _detune_segments_later(n), d0[::-1].copy()])
        s.start, s.stop = [at(130.37)] * 3, [at(2420.5)] * 3
    elif case == "both_a_rate":
        f = _freq_block(n, 8.0)
        d = _pl(n, [(0, 0.0), (600, 1200.0), (1200, -1200.0), (1800, 0.0), (2150, 4500.0), (2300, 4500.0), (2350, 0.0)])
        s.frequency = ("a", [f, f[::-1].copy(), f])  # context 1 holds both blocks reversed in time, context 2 the detune alone
        s.detune = ("a", [d, d[::-1].copy(), d[::-1].copy()])
        s.start, s.stop = [at(130.37)] * 3, [at(2420.5)] * 3
    elif case == "segments":
        # 768-frame segments.  Context 0 starts in segment 5 (3840 ...) at a fractional frame: first frame 3901, lane 15 of its
        # group; 1 stops in segment 0; 2 start == stop, 3 stop before start, 4 starts past the end (never active); 5 never stops
        f = _pl(n, [(0, 200.0), (1500, 3000.0), (1501, -1500.0), (2600, -400.0), (2601, 700.0), (4224, 2500.0)])
        s.frequency = ("a", [f] * 6)
        s.detune = ("const", [0.0, 100.0, 0.0, 0.0, 0.0, -700.0])
        s.start = [at(3900.37), 0.0, at(1000.25), at(2000.0), at(5000.0), 0.0]
        s.stop = [None, at(500.5), at(1000.25), at(1000.0), None, None]
    elif case == "many_contexts":
        i = np.arange(67)
        f = (100.0 + 37.7 * i) * np.where(i % 5 == 3, -1.0, 1.0)
        s.frequency = ("const", [float(np.float32(v)) for v in f])
        s.detune = ("const", [float(np.float32(3.0 * k - 100.0)) for k in i])
        s.start, s.stop = [at(0.1 + 3.37 * k) for k in i], [None] * 67
    else:
        assert case in ("post_ops_par", "post_ops_scan"), case
        s.frequency = ("const", [441.0, -333.3, 1234.5]) if case == "post_ops_par" else ("a", [_pl(n, [(0, 300.0), (639, 2500.0)])] * 3)
        s.detune = ("const", [0.0, 50.0, -300.0])
        s.start, s.stop = [at(130.37)] * 3, [at(600.5)] * 3
        s.gains = [0.5, 1.0 + 5e-7, 5e-7]  # the product, pass-through, mute (gain.rs:163-179)
    s.n_ctx = len(s.start)
    return s


def _per_frame(param, nq):
    kind, vals = param
    rows = []
    for v in vals:
        if kind == "const":
            rows.append(np.full(nq * RQ, v, np.float32))
        elif kind == "k":
            rows.append(np.repeat(np.asarray(v, np.float32), RQ))
        else:
            rows.append(np.asarray(v, np.float32))
    return np.stack(rows)


_MODEL = {}


def model(case, type_):
    """oscillator_model.Result of a case, once"""
    key = (case, type_)
    if key not in _MODEL:
        s = case_spec(case, type_)
        nq = (s.length + RQ - 1) // RQ
        stop = [NEVER if t is None else t for t in s.stop]
        m = om.render(type_, SR, s.length, _per_frame(s.frequency, nq), _per_frame(s.detune, nq), s.start, stop,
                      table=custom_table() if type_ == "custom" else None)
        assert_all_finite(m.samples, f"model {key}")
        for a in (m.samples, m.samples64):
            a.setflags(write=False)
        _MODEL[key] = m
    return _MODEL[key]


def rounding_term(case, type_):
    """U per frame"""
    m = model(case, type_)
    if type_ in ("sine", "custom"):
        table = custom_table() if type_ == "custom" else om.sine_table()
        return np.full(m.samples64.shape, 3.0 * 2.0 ** -24 * float(np.abs(table).max()))
    return 2.0 ** -23 * np.maximum(1.0, np.abs(m.samples64))


def expected(case, type_):
    """(the model's f32 output as the context delivers it [n_ctx, channels, length], the bound per sample; 0 = silent)"""
    m, s = model(case, type_), case_spec(case, type_)
    with np.errstate(invalid="ignore"):
        bound = np.where(m.audible, rounding_term(case, type_) + m.lipschitz * m.dphi, 0.0)
    if s.gains is None:
        return m.samples[:, None, :], bound[:, None, :]
    g = np.asarray(s.gains, np.float32)
    mute, unity = np.abs(g) <= np.float32(1e-6), np.abs(np.float32(1.0) - g) <= np.float32(1e-6)
    scale = np.where(mute, 0.0, np.where(unity, 1.0, np.abs(g.astype(np.float64))))[:, None]
    extra = np.where(mute | unity, 0.0, 2.0 ** -24)[:, None]
    bound = np.where(bound > 0.0, bound * scale + extra, 0.0) * (scale > 0.0)
    return om.gain_upmix(m.samples, g), np.repeat(bound[:, None, :], 2, axis=1)


def render(be, case, type_, plan_only=False):
    """Oscillator [-> Gain] -> destination on a binding; (output [n_ctx, channels, length], plan description or None)"""
    s = case_spec(case, type_)
    kw = dict(device=waa.PLAN_ONLY) if plan_only else {}
    ctx = waa.OfflineAudioContext(1 if s.gains is None else 2, s.length, SR, n_instances=s.n_ctx, binding=be, **kw)
    kw = dict(periodic_wave=waa.PeriodicWave.from_wavetable(custom_table())) if type_ == "custom" else dict(type_=type_)
    osc = ctx.create_oscillator(**kw)
    for name in ("frequency", "detune"):
        kind, vals = getattr(s, name)
        param = getattr(osc, name)
        for i, v in enumerate(vals):
            if kind == "const":
                param.set_value(v, instance=i)
            else:
                param.set_block(0, v if kind == "k" else v.reshape(-1, RQ), instance=i)
    head = osc
    if s.gains is not None:
        gain = ctx.create_gain(gain=1.0)
        for i, g in enumerate(s.gains):
            gain.gain.set_value(g, instance=i)
        head = osc.connect(gain)
    head.connect(ctx.destination())
    for i in range(s.n_ctx):
        osc.start_at(s.start[i], instance=i)
        if s.stop[i] is not None:
            osc.stop_at(s.stop[i], instance=i)
    plan = ctx.plan_describe() if be.prefix == "waa_" else None
    out = None if plan_only else ctx.start_rendering_sync().data
    ctx.close()
    return out, plan


def check_plan(plan, case, type_, kernel):
    s = case_spec(case, type_)
    tiles = PADDED[s.length] // 2048
    assert f"x {s.length} frames ({(s.length + RQ - 1) // RQ} quanta, {tiles} tiles of 2048)" in plan, plan
    line = f"{'custom' if type_ == 'custom' else type_} ({PLAN_LINE[kernel]}) frequency={MODE[s.frequency[0]]} detune={MODE[s.detune[0]]}"
    assert line in plan, (line, plan)
    if s.gains is not None:
        assert "renders 1 gain(s) and the up-mix 1 -> 2" in plan, plan


_ORACLE = {}


def oracle(orc, case, type_):
    key = (case, type_)
    if key not in _ORACLE:
        out = render(orc, case, type_)[0]
        out.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def compare(name, got, want, bound, factor=1.0):
    """(worst |diff| / bound over the samples with a bound, the number of samples that must be exactly 0 and are not)"""
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    assert_all_finite(got, name)
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    silent = bound == 0.0
    loud = int(np.count_nonzero(got[silent]))
    worst = float((diff[~silent] / (factor * bound[~silent])).max()) if (~silent).any() else 0.0
    k = np.unravel_index(int(np.argmax(np.where(silent, 0.0, diff / np.where(silent, 1.0, factor * bound)))), diff.shape)
    print(f"{name}: worst |diff| / bound {worst:.3e} at {tuple(int(i) for i in k)}; {loud} non-zero samples where the model is silent")
    return worst, loud


@pytest.fixture(scope="module", autouse=True)
def _write_parity_profile():
    yield
    if os.environ.get("WAA_WRITE_PROFILES") and _FIGURES:
        doc = {"rule": "per sample |diff| <= U + L_f * dphi against the model (doubled: device against oracle), exactly 0 where the "
                       "model is silent (tests/test_oscillator_kernels.py); the figures are the worst |diff| / bound of a render. "
                       "bit_identical_to_oracle: share of all samples, reported only",
               "worst_fraction_of_bound": max(max(v["device_vs_model"], v["device_vs_oracle"]) for v in _FIGURES.values()),
               "cases": _FIGURES}
        with open(os.path.join(ROOT, "profiles", "oscillator_parity.json"), "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


# ---- CPU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,type_", CASE_TYPES)
def test_input_conditions(case, type_):
    """the conditions under which the bound means something (module docstring), on the model alone"""
    m, s = model(case, type_), case_spec(case, type_)
    assert m.dphi == 8.0 * s.length * 2.0 ** -53
    assert not m.near_edge.any(), np.argwhere(m.near_edge)[:8]
    assert not m.phase_one.any(), np.argwhere(m.phase_one)[:8]
    a = m.audible
    with np.errstate(invalid="ignore"):
        share = float((m.lipschitz * m.dphi / rounding_term(case, type_))[a].max()) if a.any() else 0.0
    print(f"{case}/{type_}: {int(a.sum())} audible frames, worst L_f * dphi / U = {share:.3e}")
    assert_le(share, 1.0, "L_f * dphi / U")
    tiny = a & (m.incr != 0.0) & (np.abs(m.incr) < 1e-9)
    assert not tiny.any(), np.argwhere(tiny)[:8]
    nq = (s.length + RQ - 1) // RQ
    f, d = _per_frame(s.frequency, nq)[:, :s.length], _per_frame(s.detune, nq)[:, :s.length]
    cf = np.abs(m.incr) * SR
    exact = (np.abs(f) == np.float32(NYQ)) & (d == 0.0)
    close = m.active & ~exact & (np.abs(cf - NYQ) <= 1e-9 * NYQ)
    assert not close.any(), np.argwhere(close)[:8]
    assert np.all(np.abs(f) <= np.float32(NYQ)) and np.all(np.abs(d) <= 153600.0)  # inside the params' ranges: no clamp acts
    assert np.all((m.incr == 0.0) == (f == 0.0))


def _runs(mask):
    """(first, end) of every run of True"""
    edge = np.flatnonzero(np.diff(np.concatenate([[False], mask, [False]]).astype(np.int8)))
    return list(zip(edge[::2].tolist(), edge[1::2].tolist()))


def test_cases_reach_the_branches_they_name():
    # const: sub-sample start, start and stop inside one quantum, zero and negative increments
    m = model("const_sub_sample", "sine")
    assert m.first.tolist() == [301] * 5 and np.allclose(m.ratio, 0.5) and np.all(m.incr[2] == 0.0) and np.all(m.incr[1] < 0.0)
    assert np.array_equal(m.samples[0], m.samples[3]) and np.array_equal(m.samples[0], m.samples[4])
    assert np.all(model("const_on_frame", "square").ratio == 0.0) and np.all(model("const_on_frame", "square").incr[2] < 0.0)
    m = model("const_in_one_quantum", "triangle")
    assert _runs(m.audible[0]) == [(131, 191)] and abs(m.ratio[0] - 0.63) < 1e-6
    # per_quantum: exactly +-Nyquist is silent, one ulp inside is not; frames muted by Nyquist keep advancing the phase
    m = model("per_quantum", "square")
    f = _per_quantum_frequency()
    for q in range(20):
        if q * RQ >= 131 and (q + 1) * RQ <= 2000:
            assert bool(m.audible[0, q * RQ:(q + 1) * RQ].all()) == (abs(float(f[q])) < NYQ), q
    assert np.isclose(np.abs(m.incr[0, 9 * RQ]), 0.5, rtol=0, atol=1e-7) and np.abs(m.incr[0, 9 * RQ]) < 0.5
    assert m.active[0, 8 * RQ] and not m.audible[0, 8 * RQ] and m.first[0] == 131 and _runs(m.active[0])[-1][1] == 2001
    assert len(_runs(m.audible[1])) == 2  # 6 kHz under the detune block: out and back
    # freq_a_rate: both signs, a sign change inside a group and inside a lane's four frames
    m = model("freq_a_rate", "sawtooth")
    flips = np.flatnonzero(np.sign(m.incr[0, 1:]) != np.sign(m.incr[0, :-1])) + 1
    assert flips.tolist() == [401, 1101, 1952, 1954] and all(k % 256 for k in flips) and any(k % 4 for k in flips)
    assert m.audible[0, 1949:1955].tolist() == [True, False, True, False, True, True] and m.active[0, 1949:1955].all()
    m = model("freq_a_rate_d_k_rate", "sine")  # a new detune every quantum; context 2 leaves Nyquist inside a quantum
    assert len(_runs(m.active[2] & ~m.audible[2])) == 1 and _runs(m.active[2] & ~m.audible[2])[0][0] % RQ
    # detune_a_rate: re-entry in the group after the exit / several 512-frame segments later, twice each
    for case in ("detune_a_rate_f_const", "detune_a_rate_f_k_rate"):
        m = model(case, "sine")
        muted = [_runs(m.active[i] & ~m.audible[i]) for i in range(3)]
        assert len(muted[0]) == len(muted[1]) == len(muted[2]) == 2, muted
        for first, end in muted[0]:
            assert end // 256 == first // 256 + 1, muted[0]
        assert muted[1][0][1] // 512 - muted[1][0][0] // 512 >= 3 and muted[1][1][1] // 512 > muted[1][1][0] // 512, muted[1]
    assert np.any(model("detune_a_rate_f_k_rate", "sine").incr[0] < 0.0)
    for case, i in (("per_quantum", 2), ("detune_a_rate_f_const", 1), ("detune_a_rate_f_k_rate", 1)):  # muted increments beyond 1
        m = model(case, "sine")
        assert np.any(m.active[i] & ~m.audible[i] & (np.abs(m.incr[i]) > 1.5)), case
    m = model("both_a_rate", "custom")
    assert all(len(_runs(m.active[i] & ~m.audible[i])) == 1 for i in (0, 1))  # out through Nyquist and back
    # segments (768 frames each at this length)
    m = model("segments", "sawtooth")
    assert m.first.tolist() == [3901, 0, -1, -1, -1, 0] and (3901 % 256) // 4 == 15 and 3901 // 768 == 5
    assert abs(m.ratio[0] - 0.63) < 1e-6 and _runs(m.active[1]) == [(0, 501)] and _runs(m.active[5]) == [(0, 4225)]
    # many_contexts: a second block of osc_kernel with 3 lanes; distinct constants and sub-sample starts
    m = model("many_contexts", "square")
    assert m.incr.shape[0] == 67 == 64 + 3 and np.unique(m.incr[:, 0]).size == 67 and np.unique(np.round(m.ratio, 6)).size > 60
    assert np.any(m.incr[:, 0] < 0.0) and m.first.max() < 640
    for case, type_ in CASE_TYPES:  # every context the case means to sound does
        m = model(case, type_)
        never = {"segments": (2, 3, 4)}.get(case, ())
        for i in range(m.audible.shape[0]):
            assert (m.audible[i].sum() >= 40) == (i not in never), (case, type_, i)


def test_model_sine_table_is_within_an_ulp_of_sinf():
    t = om.sine_table()
    x = np.arange(2048, dtype=np.float32) * np.float32(2.0) * np.float32(np.pi) * (np.float32(1.0) / np.float32(2048.0))
    assert np.all(np.abs(t.astype(np.float64) - np.sin(x.astype(np.float64))) <= np.spacing(np.abs(t)).astype(np.float64))
    assert t[0] == 0.0 and t[512] == 1.0


@pytest.mark.parametrize("kernel,case,type_", DEVICE_CASES)
def test_plans(hip, monkeypatch, kernel, case, type_):
    """the kernel every device case means to run, the param modes and the padded length, from a plan-only context"""
    if kernel == "exact":
        monkeypatch.setenv("WAA_OSC_EXACT", "1")
    check_plan(render(hip, case, type_, plan_only=True)[1], case, type_, kernel)


@pytest.mark.parametrize("case,type_", CASE_TYPES)
def test_oracle_against_model(orc, case, type_):
    want, bound = expected(case, type_)
    worst, loud = compare(f"{case}/{type_}: oracle vs model", oracle(orc, case, type_), want, bound)
    assert loud == 0
    assert_le(worst, 1.0, "|diff| / (U + L_f * dphi)")


# ---- GPU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kernel,case,type_", DEVICE_CASES)
def test_device_against_model_and_oracle(hip, orc, monkeypatch, kernel, case, type_):
    if kernel == "exact":
        monkeypatch.setenv("WAA_OSC_EXACT", "1")
    got, plan = render(hip, case, type_)
    check_plan(plan, case, type_, kernel)
    want, bound = expected(case, type_)
    ref = oracle(orc, case, type_)
    name = f"{case}/{type_}/{kernel}"
    vs_model, loud = compare(f"{name}: device vs model", got, want, bound)
    vs_oracle, _ = compare(f"{name}: device vs oracle", got, ref, bound, factor=2.0)
    same = float(np.mean(got.view(np.uint32) == ref.view(np.uint32)))
    print(f"{name}: {same:.4f} of the samples are bit-identical to the oracle's")
    _FIGURES[name] = dict(device_vs_model=vs_model, device_vs_oracle=vs_oracle, bit_identical_to_oracle=same)
    assert loud == 0 and int(np.count_nonzero(ref[bound == 0.0])) == 0
    assert_le(vs_model, 1.0, "device vs model, |diff| / (U + L_f * dphi)")
    assert_le(vs_oracle, 1.0, "device vs oracle, |diff| / (2 * (U + L_f * dphi))")
