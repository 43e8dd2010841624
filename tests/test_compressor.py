"""DynamicsCompressorNode (the reference's src/node/dynamics_compressor.rs) on the device: waa_compressor.hip behind the C ABI's
WAA_NODE_DYNAMICS_COMPRESSOR and api.py's DynamicsCompressorNode.

The reference of every comparison is tests/compressor_model.c (compressor_model.py): `model_f32` is the reference's own f32
arithmetic (glibc log10f / powf / expf, unfused, FTZ + DAZ), `model_f64` the same algorithm in f64.

Tolerance.  Bit equality is not on offer: the device's log10 / pow are not glibc's and the detector feeds every rounding back for
thousands of samples.  With rel(a, b) = rms(a - b) / rms(b) per context,

    E_ref = rel(model_f32, model_f64)                    # how far the reference's own f32 arithmetic strays from the mathematics
    assert rel(gpu, model_f32) <= max(2 * E_ref, 1e-6)

Why 2: device and reference are two f32 evaluations of the same exact recurrence; by the triangle inequality their distance is at
most the sum of their distances to the f64 result.  Why the floor: where nothing is compressed E_ref is a few ulp, and 1e-6 is the
project's usual f32 parity bound (tests/test_iir.py).  Every context of every batch is checked, and a non-finite sample anywhere
in the device's output or the model's fails the case (test_a_nan_fails_the_comparison shows it does).

WAA_WRITE_PROFILES=1 makes the GPU session write rel(gpu, model_f32) / E_ref of every case to profiles/compressor_parity.json."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import compressor_model as cm
import web_audio_api_rs_amd as waa
from graphs import white_noise
from rearm import assert_differs, assert_same_bits, refill_from, render_again
from test_automation import LIN, SET, TARGET, TL

RQ = 128
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM_SETS = {
    "defaults": dict(cm.DEFAULTS),
    "hard-knee-slow-release": dict(threshold=-40.0, knee=0.0, ratio=20.0, attack=0.001, release=1.0),
    "gentle-fast": dict(threshold=-10.0, knee=10.0, ratio=4.0, attack=0.05, release=0.05),
    "wide-knee-low-threshold": dict(threshold=-60.0, knee=40.0, ratio=2.0, attack=0.0005, release=0.5),
}
SIGNALS = ("white", "gated", "sweep")
_RATIOS = {}  # case -> worst rel(gpu, model_f32) / E_ref of its contexts (and the figures behind it)


# ---- signals, graph, comparison ---------------------------------------------------------------------------------------------
def signal(kind, n_ch, frames, sr, seed):
    """white noise; noise gated between full scale and -40 dB every 0.5 s; noise with a 3 Hz amplitude sweep"""
    x = np.random.default_rng(seed).uniform(-1.0, 1.0, (n_ch, frames)).astype(np.float32)
    t = np.arange(frames, dtype=np.float64) / sr
    if kind == "gated":
        x *= np.where((t // 0.5) % 2 == 0, 1.0, 0.01).astype(np.float32)
    elif kind == "sweep":
        x *= (0.5 + 0.5 * np.sin(2 * np.pi * 3.0 * t)).astype(np.float32)
    else:
        assert kind == "white"
    return x


def comp_graph(be, audio, sr, length=None, device=-1, **params):
    """source (one AudioBuffer per context, audio [n_inst, channels, frames]) -> compressor -> destination"""
    n_inst, n_ch, frames = audio.shape
    ctx = waa.OfflineAudioContext(n_ch, length or frames, sr, n_instances=n_inst, binding=be, device=device)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(audio, sr)
    comp = ctx.create_dynamics_compressor(**params)
    src.connect(comp).connect(ctx.destination())
    src.start()
    return ctx, comp


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))


def rel(a, b):
    return rms(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / rms(b)


def compare(gpu, x, rows, sr, live=None):
    """one context: (rel(gpu, model_f32), E_ref, bound); a non-finite sample on either side fails"""
    assert gpu.shape == x.shape and gpu.dtype == np.float32, (gpu.shape, x.shape, gpu.dtype)
    want, exact = cm.model_f32(x, rows, sr, live), cm.model_f64(x, rows, sr, live)
    for name, a in (("the device's output", gpu), ("model_f32", want), ("model_f64", exact)):
        bad = ~np.isfinite(a)
        assert not bad.any(), f"{name} holds {int(bad.sum())} non-finite sample(s), the first at {tuple(int(v) for v in np.argwhere(bad)[0])}"
    assert rms(want) > 0.0, "the model's output is all zeros: nothing to compare against"
    e_ref = rel(want, exact)
    return rel(gpu, want), e_ref, max(2.0 * e_ref, 1e-6)


def check_batch(case, gpu, audio, rows_of, sr, live_of=None):
    """every context of a batch against its own model run; rows_of(i) -> [n_quanta, 5]"""
    assert gpu.shape == audio.shape, (gpu.shape, audio.shape)
    worst = None
    for i in range(audio.shape[0]):
        got, e_ref, bound = compare(gpu[i], audio[i], rows_of(i), sr, None if live_of is None else live_of(i))
        print(f"{case} context {i}: rel(gpu, model_f32) = {got:.3e}, E_ref = {e_ref:.3e}, bound = {bound:.3e}, ratio = {got / max(e_ref, 1e-300):.3f}")
        if worst is None or got / bound > worst[0] / worst[2]:
            worst = (got, e_ref, bound, i)
    _RATIOS[case] = dict(rel_gpu_f32=worst[0], e_ref=worst[1], bound=worst[2], ratio_to_e_ref=worst[0] / max(worst[1], 1e-300), context=worst[3],
                         contexts=int(audio.shape[0]))
    for i in range(audio.shape[0]):  # (after the figures of ALL contexts have been printed)
        got, e_ref, bound = compare(gpu[i], audio[i], rows_of(i), sr, None if live_of is None else live_of(i))
        assert got <= bound, f"{case}, context {i}: rel(gpu, model_f32) = {got:.3e} > max(2 * E_ref, 1e-6) = {bound:.3e} (E_ref = {e_ref:.3e})"


@pytest.fixture(scope="module", autouse=True)
def _write_parity_profile():
    yield
    if os.environ.get("WAA_WRITE_PROFILES") and _RATIOS:
        path = os.path.join(ROOT, "profiles", "compressor_parity.json")
        worst = max(_RATIOS.values(), key=lambda r: r["rel_gpu_f32"] / r["bound"])
        with open(path, "w") as f:
            json.dump({"rule": "rel(gpu, model_f32) <= max(2 * E_ref, 1e-6), E_ref = rel(model_f32, model_f64), rel = rms(a - b) / rms(b) per context",
                       "worst_ratio_to_e_ref_above_floor": max([r["ratio_to_e_ref"] for r in _RATIOS.values() if 2 * r["e_ref"] > 1e-6], default=None),
                       "worst_fraction_of_bound": worst["rel_gpu_f32"] / worst["bound"], "cases": _RATIOS}, f, indent=1, sort_keys=True)
            f.write("\n")


# ---- CPU: the reference's unit tests against model_f32 (dynamics_compressor.rs:524-580) ---------------------------------------
def test_model_inner_delay():
    sr = 44100.0
    non_zero_index = int(np.ceil(np.float32(0.006) * np.float32(sr) / np.float32(RQ))) * RQ
    assert non_zero_index == 384 and cm.delay_quanta(sr) == 3
    x = np.zeros((1, RQ * 8), np.float32)
    x[0, :RQ * 5] = 1.0
    live = np.array([1] * 5 + [0] * 3, np.uint8)  # (the source ends after five quanta: silent quanta from there on)
    for model in (cm.model_f32, cm.model_f64):
        out = model(x, cm.param_rows(8), sr, live)[0]
        assert (out[:non_zero_index] == 0.0).all()
        assert (out[non_zero_index:] != 0.0).all()


def test_model_db_to_lin():
    f = cm.lib().model_db_to_lin
    assert f(0.0) == 1.0
    for db, lin in ((-20.0, 0.1), (-40.0, 0.01), (-60.0, 0.001)):
        assert abs(f(db) - lin) <= 1e-8


def test_model_lin_to_db():
    f = cm.lib().model_lin_to_db
    for lin, db in ((1.0, 0.0), (0.1, -20.0), (0.01, -40.0), (0.001, -60.0), (0.0, -1000.0)):
        assert f(lin) == db


def test_model_delay_by_sample_rate():
    assert [cm.delay_quanta(sr) for sr in (8000.0, 44100.0, 48000.0, 96000.0)] == [1, 3, 3, 5]


def test_a_nan_fails_the_comparison():
    """the negative test of the NaN-proof comparison: one non-finite sample in an otherwise perfect output fails the case"""
    sr, x = 48000.0, signal("white", 1, RQ * 40, 48000.0, 5)
    rows = cm.param_rows(40)
    good = cm.model_f32(x, rows, sr)
    got, e_ref, bound = compare(good, x, rows, sr)
    assert got == 0.0 and e_ref > 0.0 and bound >= 1e-6
    for poison in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[0, 3000] = poison
        with pytest.raises(AssertionError, match="non-finite"):
            compare(bad, x, rows, sr)
    with pytest.raises(AssertionError, match="non-finite"):  # ... and in the INPUT (then the models hold it)
        xb = x.copy()
        xb[0, 100] = np.nan
        compare(good, xb, rows, sr)
    off = good.copy()
    off[0, RQ * 3:] *= np.float32(1.001)  # a wrong gain does not pass either
    with pytest.raises(AssertionError):
        check_batch("negative", off[None], x[None], lambda i: rows, sr)
    _RATIOS.pop("negative", None)


# ---- CPU: the mirror and the C ABI (fail on a library without the node) -------------------------------------------------------
def test_constructor_default(hip):
    ctx = waa.OfflineAudioContext(1, 1, 44100.0, binding=hip, device=waa.PLAN_ONLY)
    c = ctx.create_dynamics_compressor()
    assert (c.attack.value, c.knee.value, c.ratio.value, c.release.value, c.threshold.value) == (0.003, 30.0, 12.0, 0.25, -24.0)
    assert (c.channel_count, c.channel_count_mode, c.channel_interpretation) == (2, "clamped-max", "speakers")
    assert c.params == [c.threshold, c.knee, c.ratio, c.attack, c.release]
    assert waa.NODE_DYNAMICS_COMPRESSOR == 13 and c.kind == 13


def test_constructor_non_default(hip):
    ctx = waa.OfflineAudioContext(1, 1, 44100.0, binding=hip, device=waa.PLAN_ONLY)
    c = waa.DynamicsCompressorNode(ctx, attack=0.5, knee=12.0, ratio=1.0, release=0.75, threshold=-60.0)
    assert (c.attack.value, c.knee.value, c.ratio.value, c.release.value, c.threshold.value) == (0.5, 12.0, 1.0, 0.75, -60.0)


def test_channel_config_errors_in_the_mirror(hip):
    ctx = waa.OfflineAudioContext(2, RQ, 48000.0, binding=hip, device=waa.PLAN_ONLY)
    c = ctx.create_dynamics_compressor()
    with pytest.raises(waa.WaaError, match="NotSupportedError - DynamicsCompressorNode channel count cannot be greater than two") as e:
        c.set_channel_count(3)
    assert e.value.status == 2
    with pytest.raises(waa.WaaError, match="NotSupportedError - DynamicsCompressorNode channel count mode cannot be set to max") as e:
        c.set_channel_count_mode("max")
    assert e.value.status == 2
    with pytest.raises(waa.WaaError, match="cannot be greater than two"):
        ctx.create_dynamics_compressor(channel_count=4)
    with pytest.raises(waa.WaaError, match="cannot be set to max"):
        ctx.create_dynamics_compressor(channel_count_mode="max")
    c.set_channel_count(1)
    c.set_channel_count_mode("explicit")
    assert (c.channel_count, c.channel_count_mode) == (1, "explicit")


@pytest.mark.parametrize("setter, value, message", [
    ("set_channel_count", 3, "NotSupportedError - DynamicsCompressorNode channel count cannot be greater than two"),
    ("set_channel_count_mode", "max", "NotSupportedError - DynamicsCompressorNode channel count mode cannot be set to max")])
def test_channel_config_errors_in_batch_create(hip, setter, value, message):
    """the same two constraints behind the C ABI: the mirror's own check is bypassed, waa_batch_create answers"""
    ctx = waa.OfflineAudioContext(2, RQ, 48000.0, binding=hip, device=waa.PLAN_ONLY)
    c = ctx.create_dynamics_compressor()
    c.connect(ctx.destination())
    getattr(waa.AudioNode, setter)(c, value)
    with pytest.raises(waa.WaaError) as e:
        ctx.prepare()
    assert e.value.status == 2 and message in str(e.value)


def plan_lines(ctx):
    return ctx.plan_describe().splitlines()


def test_params_are_clamped_like_any_audio_param(hip):
    audio = white_noise(1, 1, RQ * 16)
    ctx, _ = comp_graph(hip, audio, 48000.0, device=waa.PLAN_ONLY, threshold=5.0, knee=-3.0, ratio=50.0, attack=2.0, release=-1.0)
    line = [l for l in plan_lines(ctx) if l.startswith("compressor node")]
    assert len(line) == 1 and "first row: threshold=0 knee=0 ratio=20 attack=1 release=0" in line[0], line
    ctx, _ = comp_graph(hip, audio, 48000.0, device=waa.PLAN_ONLY, threshold=-150.0, knee=41.0, ratio=0.5)
    line = [l for l in plan_lines(ctx) if l.startswith("compressor node")]
    assert "first row: threshold=-100 knee=40 ratio=1 attack=0.003 release=0.25" in line[0], line


def test_plan_names_the_compressor_launches(hip):
    audio = white_noise(3, 2, RQ * 64)
    ctx, comp = comp_graph(hip, audio, 48000.0, device=waa.PLAN_ONLY)
    lines = plan_lines(ctx)
    line = [l for l in lines if l.startswith("compressor node")]
    assert len(line) == 1, lines
    for kernel in ("compressor_level_kernel", "compressor_detector_kernel", "compressor_apply_kernel"):
        assert kernel in line[0]
    assert "2ch, look-ahead 3 quanta, 1 x 1 row(s) of block constants (shared, constant)" in line[0]
    assert not any("dyn_kernel" in l for l in lines)
    assert lines[-1].startswith("alias node 0")  # the destination aliases the compressor's output
    # per-instance values and k-rate automation: [instance][quantum] rows
    ctx, comp = comp_graph(hip, audio, 48000.0, device=waa.PLAN_ONLY)
    comp.threshold.set_value(-30.0, instance=1)
    comp.ratio.set_target_at_time(4.0, 0.01, 0.05)
    line = [l for l in plan_lines(ctx) if l.startswith("compressor node")][0]
    assert "3 x 64 row(s) of block constants (per instance, per quantum)" in line
    # look-ahead by sample rate
    for sr, d in ((8000.0, 1), (44100.0, 3), (96000.0, 5)):
        ctx, _ = comp_graph(hip, white_noise(1, 1, RQ * 16), sr, device=waa.PLAN_ONLY)
        assert any(f"1ch, look-ahead {d} quanta" in l for l in plan_lines(ctx))


def refused(ctx, *words):
    with pytest.raises(waa.WaaError) as e:
        ctx.plan_describe()
    assert e.value.status == 4, (e.value.status, str(e.value))
    for w in words:
        assert w in str(e.value), str(e.value)


def test_out_of_scope_graphs_are_refused_with_the_node_named(hip):
    sr, audio = 48000.0, white_noise(2, 2, RQ * 64)
    # inside a Delay loop
    ctx, comp = comp_graph(hip, audio, sr, device=waa.PLAN_ONLY)
    delay = ctx.create_delay(1.0)
    delay.delay_time.set_value(0.1)
    comp.connect(delay).connect(ctx.create_gain(gain=0.5)).connect(comp)
    refused(ctx, f"DynamicsCompressorNode {comp.id}", "feedback loop")
    # an edge into one of its AudioParams
    ctx, comp = comp_graph(hip, audio, sr, device=waa.PLAN_ONLY)
    lfo = ctx.create_oscillator(frequency=2.0)
    lfo.start()
    lfo.connect(comp.threshold)
    refused(ctx, f"DynamicsCompressorNode {comp.id}", "AudioParam 0")
    # a graph that needs exact per-quantum channel counts: a stereo source that ends mid-render and a mono source that goes on,
    # summed in front of a Biquad (whose input is stereo, then mono)
    ctx = waa.OfflineAudioContext(2, RQ * 64, sr, n_instances=2, binding=hip, device=waa.PLAN_ONLY)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(audio[:, :, :RQ * 20], sr)
    mono = ctx.create_buffer_source()
    mono.set_buffer_batch(audio[:, :1, :], sr)
    flt = ctx.create_biquad_filter()
    comp = ctx.create_dynamics_compressor()
    src.connect(flt)
    mono.connect(flt)
    flt.connect(comp).connect(ctx.destination())
    src.start()
    mono.start()
    refused(ctx, f"DynamicsCompressorNode {comp.id}", "exact per-quantum channel counts")


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_detector_kernel_has_no_spill_and_no_scratch(tmp_path):
    """in the style of tests/test_kernel_resources.py: the detector pays every instruction of its loop per sample, a spilled
    register or a local array in scratch memory there is a slowdown by a multiple"""
    out = str(tmp_path / "waa_compressor.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fgpu-flush-denormals-to-zero",
                           "--cuda-device-only", "-S", os.path.join(ROOT, "web-audio-api-rs_amd", "csrc", "waa_compressor.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    res = {}
    for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.wavefront_size", text, re.S):
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(2)).group(1))  # noqa: E731
        res[m.group(1)] = dict(vgpr=get("vgpr_count"), spill=get("vgpr_spill_count"), sgpr_spill=get("sgpr_spill_count"),
                               scratch=get("private_segment_fixed_size"))
    det = {k: v for k, v in res.items() if "compressor_detector_kernel" in k}
    assert len(det) == 2, sorted(res)  # shared and per-instance block constants
    for name, r in det.items():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
    for name in ("compressor_level_kernel", "compressor_apply_kernel"):
        k = [v for n, v in res.items() if name in n]
        assert len(k) == 1 and k[0]["spill"] == 0 and k[0]["scratch"] == 0, (name, k)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_inner_delay(hip):
    """dynamics_compressor.rs:524-562 through the library, exact zeros included"""
    sr = 44100.0
    ctx = waa.OfflineAudioContext(1, RQ * 8, sr, binding=hip)
    comp = ctx.create_dynamics_compressor()
    comp.connect(ctx.destination())
    buf = ctx.create_buffer(1, RQ * 5, sr)
    buf.data[0, :] = 1.0
    src = ctx.create_buffer_source()
    src.set_buffer(buf)
    src.connect(comp)
    src.start()
    chan = ctx.start_rendering_sync().get_channel_data(0)
    assert np.isfinite(chan).all()
    assert (chan[:384] == 0.0).all() and not np.signbit(chan[:384]).any()
    assert (chan[384:] != 0.0).all()
    x = np.zeros((1, RQ * 8), np.float32)
    x[0, :RQ * 5] = 1.0
    check_batch("inner-delay", chan[None, None], x[None], lambda i: cm.param_rows(8), sr, lambda i: np.array([1] * 5 + [0] * 3, np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("sr", [8000.0, 44100.0, 48000.0, 96000.0])
@pytest.mark.parametrize("n_ch", [1, 2])
@pytest.mark.parametrize("pset", sorted(PARAM_SETS))
def test_parity(hip, pset, n_ch, sr):
    """2 s; one batch per (parameter set, channels, sample rate), its three contexts are the three signals"""
    frames = int(2 * sr) // RQ * RQ
    audio = np.stack([signal(kind, n_ch, frames, sr, 0xC0 + k) for k, kind in enumerate(SIGNALS)])
    ctx, _ = comp_graph(hip, audio, sr, **PARAM_SETS[pset])
    gpu = ctx.start_rendering_sync().data
    rows = cm.param_rows(frames // RQ, **PARAM_SETS[pset])
    check_batch(f"parity {pset} {n_ch}ch {int(sr)} Hz ({', '.join(SIGNALS)})", gpu, audio, lambda i: rows, sr)


@pytest.mark.gpu
@pytest.mark.parametrize("per_instance", [False, True], ids=["shared-params", "per-instance-params"])
def test_256_contexts(hip, per_instance):
    sr, n, frames = 48000.0, 256, RQ * 375  # 1 s
    audio = np.stack([signal(SIGNALS[i % 3], 1, frames, sr, 0x256 + i) for i in range(n)])
    ctx, comp = comp_graph(hip, audio, sr)
    sets = []
    for i in range(n):
        p = dict(cm.DEFAULTS)
        if per_instance:
            p = dict(threshold=-60.0 + 0.2 * i, knee=float(i % 41), ratio=1.0 + (i % 20), attack=0.0005 * (i % 9), release=0.02 + 0.003 * i)
            for name, v in p.items():
                getattr(comp, name).set_value(v, instance=i)
        sets.append(p)
    gpu = ctx.start_rendering_sync().data
    check_batch(f"256 contexts, {'per-instance' if per_instance else 'shared'} params", gpu, audio,
                lambda i: cm.param_rows(frames // RQ, **sets[i]), sr)
    assert len({gpu[i].tobytes() for i in range(n)}) == n  # distinct audio, distinct results


def k_rate_values(orc_lib, name, nq, sr, v0, events):
    """one value per quantum of a k-rate param that starts at v0 and gets `events` [(type, value, time, aux)]: the oracle's
    restatement of AudioParamProcessor (tests/test_automation.py pins it against the reference and the library's twin), index 0
    of every quantum's slice"""
    lo, hi = cm.RANGES[name]
    tl = TL(orc_lib, "orc_", cm.DEFAULTS[name], lo, hi, a_rate=False)
    tl.ok(SET, v0)
    for kind, value, time, aux in events:
        tl.ok(kind, value, time, aux)
    return np.array([tl.compute(q * RQ / sr, count=RQ, dt=1.0 / sr)[0] for q in range(nq)], np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("per_instance", [False, True], ids=["shared", "per-instance"])
def test_k_rate_automation(hip, orc_lib, per_instance):
    """a linear ramp on `threshold` and a set_target_at_time on `ratio`, scheduled for every context alike or per instance; a
    second batch takes the same per-quantum values as explicit k-rate value blocks"""
    sr, n, frames = 48000.0, 4, RQ * 750  # 2 s
    nq = frames // RQ
    audio = np.stack([signal("white", 2, frames, sr, 0xA07 + i) for i in range(n)])
    plans = []
    for i in range(n):
        k = i if per_instance else 0
        plans.append(dict(thr0=-10.0 - 5.0 * k, thr=(LIN, -50.0, 1.5 - 0.25 * k, 0.0), ratio=(TARGET, 2.0 + k, 0.25 + 0.125 * k, 0.3)))
    ctx, comp = comp_graph(hip, audio, sr)
    for i in (range(n) if per_instance else [waa.ALL]):
        p = plans[0 if i == waa.ALL else i]
        comp.threshold.set_value(p["thr0"], instance=i)
        comp.threshold.linear_ramp_to_value_at_time(p["thr"][1], p["thr"][2], instance=i)
        comp.ratio.set_target_at_time(p["ratio"][1], p["ratio"][2], p["ratio"][3], instance=i)
    line = [l for l in plan_lines(ctx) if l.startswith("compressor node")][0]
    assert ("per instance" if per_instance else "shared") in line and "per quantum" in line, line
    gpu = ctx.start_rendering_sync().data
    rows = [cm.param_rows(nq, threshold=k_rate_values(orc_lib, "threshold", nq, sr, p["thr0"], [p["thr"]]),
                          ratio=k_rate_values(orc_lib, "ratio", nq, sr, cm.DEFAULTS["ratio"], [p["ratio"]])) for p in plans]
    assert rows[0][0, 0] != rows[0][-1, 0] and rows[0][0, 2] != rows[0][-1, 2]  # (both really move)
    what = "per instance" if per_instance else "shared"
    check_batch(f"k-rate automation events ({what})", gpu, audio, lambda i: rows[i], sr)
    ctx2, comp2 = comp_graph(hip, audio, sr)
    for i in (range(n) if per_instance else [waa.ALL]):
        r = rows[0 if i == waa.ALL else i]
        comp2.threshold.set_block(0, r[:, 0], instance=i)
        comp2.ratio.set_block(0, r[:, 2], instance=i)
    gpu2 = ctx2.start_rendering_sync().data
    check_batch(f"k-rate value blocks ({what})", gpu2, audio, lambda i: rows[i], sr)
    assert_same_bits(gpu2, gpu, what="the batch with explicit k-rate value blocks")


@pytest.mark.gpu
def test_attack_zero_and_hard_knee(hip):
    """attack = 0 (attack_tau = 0) and knee = 0 (the middle branch unreachable, knee_partial = -inf); ratio = 1 with knee = 0 makes
    knee_partial 0 / 0"""
    sr, frames = 48000.0, RQ * 750
    audio = np.stack([signal(kind, 2, frames, sr, 0x4A + k) for k, kind in enumerate(SIGNALS)])
    sets = [dict(threshold=-30.0, knee=0.0, ratio=8.0, attack=0.0, release=0.1),
            dict(threshold=-30.0, knee=0.0, ratio=1.0, attack=0.0, release=0.1),
            dict(threshold=-20.0, knee=6.0, ratio=20.0, attack=0.0, release=0.0)]
    for k, p in enumerate(sets):
        ctx, _ = comp_graph(hip, audio, sr, **p)
        gpu = ctx.start_rendering_sync().data
        rows = cm.param_rows(frames // RQ, **p)
        check_batch(f"edge values {k}: {p}", gpu, audio, lambda i: rows, sr)


@pytest.mark.gpu
def test_in_a_graph(hip, orc):
    """stereo source (as long as the render: the plan stays static) -> Biquad -> compressor -> Gain -> destination; expected: the
    oracle's render of source -> Biquad fed through model_f32 and scaled"""
    sr, n, frames, gain = 48000.0, 5, RQ * 750, np.float32(0.7)
    audio = np.stack([signal(SIGNALS[i % 3], 2, frames, sr, 0x96A + i) for i in range(n)])

    def build(be, with_comp):
        ctx = waa.OfflineAudioContext(2, frames, sr, n_instances=n, binding=be)
        src = ctx.create_buffer_source()
        src.set_buffer_batch(audio, sr)
        tail = src.connect(ctx.create_biquad_filter(type_="lowpass", frequency=2500.0, q=0.9))
        if with_comp:
            tail = tail.connect(ctx.create_dynamics_compressor()).connect(ctx.create_gain(gain=float(gain)))
        tail.connect(ctx.destination())
        src.start()
        return ctx

    filtered = build(orc, False).start_rendering_sync().data
    ctx = build(hip, True)
    assert not any("dyn_kernel" in l for l in plan_lines(ctx))
    gpu = ctx.start_rendering_sync().data
    rows = cm.param_rows(frames // RQ)
    assert np.isfinite(gpu).all() and np.isfinite(filtered).all()
    worst = None
    for i in range(n):
        want, exact = cm.model_f32(filtered[i], rows, sr) * gain, cm.model_f64(filtered[i], rows, sr) * gain
        assert np.isfinite(want).all() and np.isfinite(exact).all()
        e_ref = rel(want, exact)
        got, bound = rel(gpu[i], want), max(2 * e_ref, 1e-6)
        print(f"in a graph, context {i}: rel = {got:.3e}, E_ref = {e_ref:.3e}, bound = {bound:.3e}")
        if worst is None or got / bound > worst[0] / worst[2]:
            worst = (got, e_ref, bound, i)
    _RATIOS["in a graph: source -> Biquad -> compressor -> Gain"] = dict(rel_gpu_f32=worst[0], e_ref=worst[1], bound=worst[2],
                                                                         ratio_to_e_ref=worst[0] / worst[1], context=worst[3], contexts=n)
    assert worst[0] <= worst[2], worst


@pytest.mark.gpu
@pytest.mark.parametrize("buffer_frames", [RQ * 20, RQ * 20 + 57], ids=["ends-on-a-quantum", "ends-inside-a-quantum"])
def test_mono_source_that_stops_early(hip, buffer_frames):
    """the output is exactly zero from D quanta after the last quantum the source wrote into"""
    sr, n, frames = 48000.0, 3, RQ * 64
    d = cm.delay_quanta(sr)
    audio = np.zeros((n, 1, frames), np.float32)
    audio[:, :, :buffer_frames] = white_noise(n, 1, buffer_frames, seed0=0x57)
    ctx = waa.OfflineAudioContext(1, frames, sr, n_instances=n, binding=hip)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(np.ascontiguousarray(audio[:, :, :buffer_frames]), sr)
    src.connect(ctx.create_dynamics_compressor()).connect(ctx.destination())
    src.start()
    gpu = ctx.start_rendering_sync().data
    last = (buffer_frames - 1) // RQ  # the last quantum the source wrote into
    tail = gpu[:, :, (last + 1 + d) * RQ:]
    assert tail.size > 0 and (tail == 0.0).all() and not np.signbit(tail).any()
    assert (gpu[:, :, :d * RQ] == 0.0).all()
    assert (np.abs(gpu[:, :, d * RQ:(last + d) * RQ]).max(axis=2) > 0.0).all()
    live = np.zeros(frames // RQ, np.uint8)
    live[:last + 1] = 1
    check_batch(f"mono source that stops after {buffer_frames} frames", gpu, audio, lambda i: cm.param_rows(frames // RQ), sr, lambda i: live)


@pytest.mark.gpu
def test_render_contexts_carries_the_node(hip):
    """three single-instance contexts with different thresholds through render_contexts (one merged batch, per-instance params):
    each equals its own render bit for bit"""
    sr, frames = 48000.0, RQ * 200
    thresholds = (-12.0, -35.0, -70.0)

    def build(k):
        ctx = waa.OfflineAudioContext(2, frames, sr, binding=hip)
        src = ctx.create_buffer_source()
        src.set_buffer(waa.AudioBuffer(signal("white", 2, frames, sr, 0x3C + k), sr))
        src.connect(ctx.create_dynamics_compressor(threshold=thresholds[k], ratio=6.0)).connect(ctx.destination())
        src.start()
        return ctx

    ctxs = [build(k) for k in range(3)]
    assert waa.bucket_report(ctxs) == [[0, 1, 2]]
    merged = waa.render_contexts(ctxs)
    for k in range(3):
        own = build(k).start_rendering_sync().data
        assert np.isfinite(own).all()
        assert_same_bits(merged[k].data, own, what=f"context {k} rendered in the merged batch")
    assert_differs(merged[0].data, merged[1].data, what="context 0")


@pytest.mark.gpu
def test_rearm_and_rerender(hip):
    """a re-armed batch with new audio is bit-identical to a fresh batch on that audio (detector state and ring start over);
    two renders of one batch are bit-identical"""
    sr, n, frames = 48000.0, 6, RQ * 300
    a = np.stack([signal("gated", 2, frames, sr, 0xA + i) for i in range(n)])
    bb = np.stack([signal("sweep", 2, frames, sr, 0xB + i) for i in range(n)])
    ctx, _ = comp_graph(hip, a, sr, release=1.0)
    first = ctx.start_rendering_sync().data
    assert np.isfinite(first).all()
    assert_same_bits(render_again(ctx), first, what="the second render of the batch")
    donor, _ = comp_graph(hip, bb, sr, release=1.0)
    assert refill_from(ctx, donor) == 1
    again = render_again(ctx)
    fresh_ctx, _ = comp_graph(hip, bb, sr, release=1.0)
    fresh = fresh_ctx.start_rendering_sync().data
    assert np.isfinite(fresh).all()
    assert_same_bits(again, fresh)
    assert_differs(again, first)
