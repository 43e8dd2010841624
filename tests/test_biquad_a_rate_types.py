"""Every branch of the a-rate Biquad's coefficient formulas, on the device (biquad_coef_kernel in waa_kernels.hip and the
three kernels that consume its table) and in the oracle, against tests/biquad_model.py — a numpy model written from the
reference's src/node/biquad_filter.rs alone.

All eight types are rendered with per-frame `frequency` (a sweep; and a block that runs from below 0 Hz through the
audible range to above Nyquist, so that the hardwired `f == 0` / `f == 1` sets and the normalised ones alternate inside a
2048-frame tile), per-frame `Q` through 0, per-frame `gain` over a k-rate `frequency`, and per-frame `detune` with a run
at exactly 0 (the `detune != 0` split of get_computed_freq).  The inputs are value blocks, so the three legs are handed
the same f32 per-frame values and none of them restates automation.

Bounds (those of test_c1_a_rate_biquad / test_c1a_edges_every_instance_rerendered): per (context, channel)
RMS <= 1e-6 and max |diff| <= 2e-6 * max(1, peak(model)), for device against model, device against oracle and oracle
against model.  Input cap, checked on the CPU: the device's exp2f / sin / cos / pow may be 1-2 ulp off numpy's, so for
every case the model is evaluated again with every computed frequency one f32 ulp up, and one down — far more than an
f64 ulp of sin / cos / pow moves a coefficient — and the output may move by at most a quarter of the max-|diff| bound.
Frames that sit exactly on a limit of the frequency param's clamp (0 and Nyquist) are not moved: every leg computes the
clamp exactly, and the hardwired sets they select are not continuous with the formulas (biquad_model.computed_freq).
What the cap made of the cases: the sweep runs with Q = 1 (Q = 1.5 moved the allpass by 0.28 of the bound), and the
`edges` block crosses Nyquist in one step from 12 kHz instead of gliding through the last Hz below it (_edges_block).

No case feeds non-finite values.  WAA_WRITE_PROFILES=1 makes the GPU session write the measured fractions of the bounds
into the "biquad" section of profiles/param_kernels_parity.json."""
import json
import os

import numpy as np
import pytest

import biquad_model as bm
import web_audio_api_rs_amd as waa
from graphs import assert_all_finite, assert_le, rms_err, white_noise

RQ = 128
TOL = 1e-6
MAX_TOL = 2e-6  # times max(1, peak(model))
SR, N_CTX, N_CH = 48000.0, 3, 2
FRAMES = 2 * 2048 + 3 * RQ + 9  # two full 2048-frame tiles, a partial third (the table's padded tail), a last partial quantum
NQ = (FRAMES + RQ - 1) // RQ
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAIN_TYPES = ("peaking", "lowshelf", "highshelf")
Q_TYPES = ("bandpass", "notch", "allpass", "peaking")
CASE_TYPES = dict(sweep=bm.TYPES, edges=bm.TYPES, q_through_zero=Q_TYPES, gain_a_rate=GAIN_TYPES, detune_a_rate=bm.TYPES)
CASES = [(c, t) for c, types in CASE_TYPES.items() for t in types]
PLAN_LINE = {"shared": "biquad_lanes(a-rate, shared table", "per-instance": "biquad_stream(a-rate, per-instance table)",
             "stream": "biquad_stream(a-rate, shared table)"}
_FIGURES = {}  # "case/type/route" -> fractions of the bounds


def _edges_block():
    """frequency per frame for quanta 1 ... 34: below 0 Hz at the start, up into the audible range, down through 0 again,
    up and past Nyquist, back down through the whole range and below 0, and past Nyquist to the end.  Nyquist is crossed in
    one step from / to 12 kHz: one f32 ulp of a frequency f moves sin(pi f / Nyquist) by ulp / (Nyquist - f) of itself, so a
    frame a few Hz below Nyquist fails the input cap (0 Hz has no such neighbourhood: there the ulp shrinks with f)"""
    knots = [(128, -400.0), (500, 3000.0), (900, -200.0), (1100, -200.0), (2433, 12000.0), (2434, 26000.0), (3000, 26000.0),
             (3001, 12000.0), (3400, 5000.0), (3900, -100.0), (4190, 12000.0), (4191, 30000.0), (4479, 30000.0)]
    t = np.arange(RQ, 35 * RQ)
    return np.interp(t, [k[0] for k in knots], [k[1] for k in knots]).astype(np.float32).reshape(34, RQ)


def _q_block():
    """Q per frame for quanta 2 ... 31: 3 down to -1 and back in steps of 1/480, both passes exactly through 0"""
    down = np.arange(1440, -481, -1)
    k = np.concatenate([down, down[-2:0:-1]])
    assert k.size == 30 * RQ
    return (k.astype(np.float64) / 480.0).astype(np.float32).reshape(30, RQ)


def _detune_block():
    """detune per frame for quanta 2 ... 33: -1200 cents up to -1, 300 frames at exactly 0.0, then 1 up to 1200"""
    v = np.concatenate([np.linspace(-1200.0, -1.0, 1800), np.zeros(300), np.linspace(1.0, 1200.0, 32 * RQ - 2100)])
    return v.astype(np.float32).reshape(32, RQ)


def case_params(case, type_):
    """(params, own): the four params as biquad_model.per_frame takes them (a constant, or (constant, quantum0, block)), and
    the name of the a-rate one — the per-instance route gives context 1 that block reversed in time"""
    gain = 6.0 if type_ in GAIN_TYPES else 0.0
    if case == "sweep":
        f = np.geomspace(60.0, 20000.0, NQ * RQ).astype(np.float32).reshape(NQ, RQ)
        return dict(frequency=(350.0, 0, f), detune=0.0, q=1.0, gain=gain), "frequency"
    if case == "edges":
        return dict(frequency=(1000.0, 1, _edges_block()), detune=0.0, q=1.5, gain=gain), "frequency"
    if case == "q_through_zero":
        return dict(frequency=1200.0, detune=0.0, q=(1.0, 2, _q_block()), gain=gain), "q"
    if case == "gain_a_rate":
        g = np.linspace(-18.0, 18.0, 12 * RQ).astype(np.float32).reshape(12, RQ)
        return dict(frequency=(800.0, 4, np.geomspace(300.0, 5000.0, 27).astype(np.float32)), detune=0.0, q=1.5, gain=(6.0, 10, g)), "gain"
    assert case == "detune_a_rate"
    return dict(frequency=1000.0, detune=(0.0, 2, _detune_block()), q=4.0, gain=gain), "detune"


def own_params(case, type_):
    params, own = case_params(case, type_)
    const, q0, block = params[own]
    params[own] = (const, q0, np.ascontiguousarray(block.reshape(-1)[::-1]).reshape(block.shape))
    return params


_NOISE = []


def noise():
    if not _NOISE:
        _NOISE.append(white_noise(N_CTX, N_CH, FRAMES))
        _NOISE[0].setflags(write=False)
    return _NOISE[0]


_MODEL = {}


def model(case, type_, table, ulps=0):
    """the model's render [N_CTX, N_CH, FRAMES], once per (case, type, table, ulps)"""
    key = (case, type_, table, ulps)
    if key not in _MODEL:
        x = noise()
        out = bm.render(type_, SR, x.reshape(-1, FRAMES), ulps=ulps, **case_params(case, type_)[0]).reshape(x.shape)
        if table == "per-instance":
            out[1] = bm.render(type_, SR, x[1], ulps=ulps, **own_params(case, type_))
        assert_all_finite(out, f"model {key}")
        out.setflags(write=False)
        _MODEL[key] = out
    return _MODEL[key]


def render(be, case, type_, table):
    """source -> BiquadFilterNode -> destination on a binding; (output, plan description or None)"""
    params, own = case_params(case, type_)
    x = noise()
    ctx = waa.OfflineAudioContext(N_CH, FRAMES, SR, n_instances=N_CTX, binding=be)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(x, SR)
    const = {k: (v if np.isscalar(v) else v[0]) for k, v in params.items()}
    bq = ctx.create_biquad_filter(type_=type_, **const)
    for name, v in params.items():
        if not np.isscalar(v):
            getattr(bq, name).set_block(v[1], v[2])
    if table == "per-instance":
        _, q0, block = own_params(case, type_)[own]
        getattr(bq, own).set_block(q0, block, instance=1)
    src.connect(bq).connect(ctx.destination())
    src.start()
    plan = ctx.plan_describe() if be.prefix == "waa_" else None
    out = ctx.start_rendering_sync().data
    ctx.close()
    return out, plan


_ORACLE = {}


def oracle(orc, case, type_, table):
    key = (case, type_, table)
    if key not in _ORACLE:
        out = render(orc, case, type_, table)[0]
        out.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def fractions(got, want, peak_of):
    """(worst RMS / TOL, worst max |diff| / its bound) of two renders; the max-|diff| bound scales with the MODEL's peak"""
    max_bound = MAX_TOL * max(1.0, float(np.abs(peak_of).max()))
    return float(rms_err(got, want).max()) / TOL, float(np.abs(got.astype(np.float64) - want).max()) / max_bound


def check(name, got, want, peak_of, figures):
    assert got.shape == want.shape == (N_CTX, N_CH, FRAMES)
    assert_all_finite(got, name)
    r, m = fractions(got, want, peak_of)
    print(f"{name}: RMS {r:.3e} of its bound, max |diff| {m:.3e} of its bound")
    figures[name.split(": ")[1]] = dict(rms=r, max_abs=m)
    return r, m


def input_cap(case, type_):
    """how far one f32 ulp of every computed frequency moves the model's output, as a fraction of the max-|diff| bound"""
    base = model(case, type_, "shared")
    bound = MAX_TOL * max(1.0, float(np.abs(base).max()))
    return max(float(np.abs(model(case, type_, "shared", u).astype(np.float64) - base).max()) for u in (1, -1)) / bound


@pytest.fixture(scope="module", autouse=True)
def _write_parity_profile():
    yield
    if os.environ.get("WAA_WRITE_PROFILES") and _FIGURES:
        path = os.path.join(ROOT, "profiles", "param_kernels_parity.json")
        doc = {}
        if os.path.exists(path):
            with open(path) as f:
                doc = json.load(f)
        worst = {k: max(v[leg][k] for v in _FIGURES.values() for leg in v) for k in ("rms", "max_abs")}
        doc["biquad"] = {
            "rule": "per (context, channel): RMS <= 1e-6 and max |diff| <= 2e-6 * max(1, peak(model)); the figures are fractions of those "
                    "bounds.  input_cap: the model's move under one f32 ulp of every computed frequency, as a fraction of the "
                    "max-|diff| bound (asserted <= 0.25)",
            "worst_fraction_of_bound": worst, "cases": _FIGURES,
            "input_cap": {f"{c}/{t}": input_cap(c, t) for c, t in CASES}}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def _span_starts(mask):
    return np.flatnonzero(mask & ~np.concatenate([[False], mask[:-1]]))


def test_cases_reach_the_branches_they_name():
    """the blocks themselves: spans of f == 0, of normal frequencies and of f == 1 that begin inside a quantum and inside
    a tile, both kinds of coefficient set inside one tile; Q at exactly 0 and below; a run of detune == 0.0 inside a
    quantum; quanta with only single-valued slices, with mixed lengths, and both transitions"""
    f = bm.per_frame(case_params("edges", "lowpass")[0]["frequency"], NQ, 0.0)
    zero, one = f <= 0.0, f >= SR / 2
    for name, mask in (("f == 0", zero), ("f == 1", one), ("normal", ~zero & ~one)):
        inside = [s for s in _span_starts(mask) if s % RQ and s % 2048]
        assert len(inside) >= 1, (name, _span_starts(mask))
    assert f[0] == 1000.0 and f[RQ] < 0.0 and f[35 * RQ - 1] > SR / 2  # the block starts below 0 Hz and ends above Nyquist
    t0, t1 = slice(0, 2048), slice(2048, 4096)
    assert zero[t0].any() and (~zero & ~one)[t0].any()
    assert zero[t1].any() and one[t1].any() and (~zero & ~one)[t1].any()
    assert not np.any((f > 12000.0) & (f < SR / 2))  # (see _edges_block)
    q = bm.per_frame(case_params("q_through_zero", "notch")[0]["q"], NQ, 0.0)
    assert (q == 0.0).sum() == 2 and q.min() == -1.0 and q.max() == 3.0 and all(s % RQ for s in np.flatnonzero(q == 0.0))
    d = bm.per_frame(case_params("detune_a_rate", "notch")[0]["detune"], NQ, 0.0)
    run = np.flatnonzero(d[2 * RQ:34 * RQ] == 0.0) + 2 * RQ
    assert run.size == 300 and run[0] % RQ and d.min() == -1200.0 and d.max() == 1200.0
    p = case_params("gain_a_rate", "peaking")[0]
    assert (p["gain"][1], p["gain"][2].shape, p["frequency"][1], p["frequency"][2].shape) == (10, (12, RQ), 4, (27,))
    for case, type_ in CASES:  # no case feeds a non-finite value
        for v in case_params(case, type_)[0].values():
            assert np.all(np.isfinite(v if np.isscalar(v) else v[2]))


@pytest.mark.parametrize("table", ["shared", "per-instance"])
@pytest.mark.parametrize("case,type_", CASES)
def test_oracle_against_model(orc, case, type_, table):
    got, want = oracle(orc, case, type_, table), model(case, type_, table)
    r, m = check(f"{case}/{type_}/{table}: oracle vs model", got, want, want, {})
    assert float(np.abs(want).max()) > 1e-3
    assert_le(r, 1.0, "RMS, fraction of 1e-6")
    assert_le(m, 1.0, "max |diff|, fraction of 2e-6 * max(1, peak)")


@pytest.mark.parametrize("case,type_", CASES)
def test_input_cap(case, type_):
    """one f32 ulp of every computed frequency moves the output by at most a quarter of the max-|diff| bound"""
    cap = input_cap(case, type_)
    print(f"{case}/{type_}: one ulp of the computed frequency moves the output by {cap:.3e} of the max-|diff| bound")
    assert_le(cap, 0.25, "fraction of the max-|diff| bound")


# ---- GPU --------------------------------------------------------------------------------------------------------------------
def _device_case(hip, orc, case, type_, route):
    table = "per-instance" if route == "per-instance" else "shared"
    got, plan = render(hip, case, type_, table)
    assert PLAN_LINE[route] in plan, plan
    want, ref = model(case, type_, table), oracle(orc, case, type_, table)
    figures = _FIGURES.setdefault(f"{case}/{type_}/{route}", {})
    results = [check(f"{case}/{type_}/{route}: device vs model", got, want, want, figures),
               check(f"{case}/{type_}/{route}: device vs oracle", got, ref, want, figures)]
    for r, m in results:  # (after both legs' figures have been printed)
        assert_le(r, 1.0, "RMS, fraction of 1e-6")
        assert_le(m, 1.0, "max |diff|, fraction of 2e-6 * max(1, peak)")


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["shared", "per-instance"])
@pytest.mark.parametrize("case,type_", CASES)
def test_device_against_model_and_oracle(hip, orc, case, type_, route):
    """biquad_coef_kernel's table read by the lane kernel (one table for the batch) and, lane-major, by the streaming kernel
    (context 1 has a block of its own)"""
    _device_case(hip, orc, case, type_, route)


@pytest.mark.gpu
@pytest.mark.measure
@pytest.mark.parametrize("case,type_", [(c, t) for c, t in CASES if c in ("sweep", "edges")])
def test_device_shared_table_streamed(hip, orc, monkeypatch, case, type_):
    """the shared table read by the streaming kernel, with the tile digests of biquad_hp_kernel (WAA_ARATE_STREAM=1)"""
    monkeypatch.setenv("WAA_ARATE_STREAM", "1")
    _device_case(hip, orc, case, type_, "stream")
