"""WaveShaperNode with one curve per context of a batch (waa_waveshaper_set_curve_instance, include/waa_hip_device.h), rendered node-major
by one launch of its own (waa_shaper_inst.hip).

CPU part: the refusals of the C ABI and of api.py, the plan lines of plan-only batches, the count replay's per-instance flag, mixed.py's
merge, the registers of the new kernel.

GPU part (-m gpu): two references.  (1) The SHARED path: for every curve k of a per-instance batch a one-context batch renders with curve
k as its shared curve, and instance k is compared as uint32 words — the lookup is the same f32 expression (waa_curve.hpp) on the same
input values, so nothing but equality is right.  (2) The oracle, rendered ONE CONTEXT AT A TIME with that context's curve (its binding
keeps one curve per batch), through the NaN-proof helpers of tests/every_instance.py at the project's bar for this node: 1e-6 RMS per
instance and channel (tests/test_gpu_parity.py).  max |d|: 1e-6 behind a BufferSource (the inputs are the same bits on both sides and the
curves stay within [-1, 1]: an ulp of the output is 6e-8; tests/test_gpu_parity.py holds the shared shaper to the same figure), 5e-6
behind the oscillator (tests/test_oscillator.py's bar for the device's sine against the oracle's, through curves of slope <= 1)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import web_audio_api_rs_amd as waa
from every_instance import _compare_all
from graphs import white_noise

RQ = 128
SR = 48000.0
CAP = 8192          # SHAPER_LDS_CAP (waa_internal.hpp): the longest curve the kernel stages in LDS
SHAPER_TILE = 4096  # frames of a workgroup's time tile
FRAMES = 9001       # lp = 10240: two whole time tiles and half a one; not a multiple of 128
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-audio-api-rs_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
gpu = pytest.mark.gpu
FP = C.POINTER(C.c_float)


def _fp(a):
    return np.ascontiguousarray(a, np.float32).ctypes.data_as(FP)


def tanh_curve(n, drive=2.0):
    """odd n: the centre is exactly 0"""
    return np.tanh(drive * np.linspace(-1.0, 1.0, n)).astype(np.float32)


def lifted_curve(n, lo=0.2, hi=0.9):
    """a curve whose centre is not 0: silence comes out as a signal (waveshaper.rs:498-509)"""
    return np.linspace(lo, hi, n).astype(np.float32)


def centre(c):
    """what the lookup makes of a sample of 0, in its own f32 arithmetic (waa_curve.hpp)"""
    n = c.size
    return c[n // 2] if n % 2 else np.float32(0.5) * c[n // 2 - 1] + np.float32(0.5) * c[n // 2]


# lengths 2, 3, 4, 129, 2048, the cap: odd and even, and (FORM_B) one point above the cap
FORM_A = [tanh_curve(2), tanh_curve(3, 1.0), tanh_curve(4, 3.0), tanh_curve(129, 1.5), tanh_curve(2048, 4.0), tanh_curve(CAP, 2.5)]
FORM_B = FORM_A + [tanh_curve(CAP + 1, 2.5)]


def probe_noise(n_inst, n_ch, frames, seed0):
    """white noise whose first samples are the lookup's edge cases: exactly -1, 0, +1; beyond both clamps; on a knot of the 3-, 129- and
    the (cap + 1)-point curves and one ulp to either side of it"""
    x = white_noise(n_inst, n_ch, frames, seed0=seed0)
    f = np.float32
    knots = [f(-0.375), f(0.5), f(-1.0 + 2.0 * 1000 / CAP)]  # 40 / 64 - 1 and 96 / 64 - 1 of 129 points; 1000 / 4096 - 1 of cap + 1
    probe = [-1.0, 0.0, 1.0, -1.5, 1.5, -100.0, 100.0, -0.0]
    for k in knots:
        probe += [k, np.nextafter(k, f(1.0)), np.nextafter(k, f(-1.0))]
    probe += [np.nextafter(f(1.0), f(0.0)), np.nextafter(f(-1.0), f(0.0)), np.nextafter(f(1.0), f(2.0))]
    x[:, :, :len(probe)] = np.asarray(probe, np.float32)
    x[:, :, SHAPER_TILE - 2:SHAPER_TILE + 2] = np.asarray([1.0, -1.0, 0.0, 1.25], np.float32)  # across a tile boundary
    return x


def build(binding, audio, curves, shared=None, graph="source", channels=2, length=FRAMES, device=-1, start=None, n_inst=None):
    """graph "source": BufferSource -> WaveShaper -> destination; "osc": Oscillator -> Gain -> WaveShaper -> Gain -> destination.
    curves: one per instance, None = that instance has no curve of its own; shared: the ALL curve."""
    n_inst = n_inst or len(curves)
    ctx = waa.OfflineAudioContext(channels, length, SR, n_instances=n_inst, binding=binding, device=device)
    sh = ctx.create_wave_shaper(curve=shared)
    for i, c in enumerate(curves):
        if c is not None:
            sh.set_curve(c, instance=i)
    if graph == "source":
        src = ctx.create_buffer_source()
        src.set_buffer_batch(audio, SR)
        src.connect(sh).connect(ctx.destination())
        src.start() if start is None else src.start_at(start)
    else:
        osc = ctx.create_oscillator(type_="sine", frequency=441.0)
        osc.connect(ctx.create_gain(gain=1.5)).connect(sh).connect(ctx.create_gain(gain=0.5)).connect(ctx.destination())
        osc.start()
    return ctx, sh


def shaper_lines(ctx):
    return [l for l in ctx.plan_describe().splitlines() if l.startswith("shaper node")]


def render(ctx):
    out = ctx.start_rendering_sync().data
    ctx.close()
    return out


def render_per_instance(hip, audio, curves, expect_form="A", **kw):
    ctx, _ = build(hip, audio, curves, **kw)
    lines = shaper_lines(ctx)
    assert len(lines) == 1 and f"form {expect_form}:" in lines[0] and "-> shaper_inst_kernel" in lines[0], ctx.plan_describe()
    return render(ctx)


def effective(curves, shared):
    return [c if c is not None else shared for c in curves]


def shared_each(hip, audio, curves, shared=None, **kw):
    """the SHARED path, one context per curve: instance k of the batch as a one-context batch whose shared curve is curve k"""
    outs = []
    for k, c in enumerate(effective(curves, shared)):
        ctx, _ = build(hip, None if audio is None else audio[k:k + 1], [], shared=c, n_inst=1, **kw)
        assert not shaper_lines(ctx), ctx.plan_describe()
        outs.append(render(ctx)[0])
    return np.stack(outs)


def assert_words(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32
    diff = got.view(np.uint32) != ref.view(np.uint32)
    if diff.any():
        k = tuple(int(v) for v in np.unravel_index(int(np.argmax(diff)), diff.shape))
        raise AssertionError(f"{what}: {int(diff.sum())} of {got.size} words differ from the shared path; the first at (instance, channel, frame) "
                             f"{k}: {got[k]!r} against {ref[k]!r}")


def assert_oracle(orc, got, audio, curves, shared=None, max_abs=1e-6, **kw):
    """the oracle one context at a time, each with its own curve as ITS shared curve; every (instance, channel) row at 1e-6 RMS"""
    eff = effective(curves, shared)

    def one(binding, lo, hi):
        assert hi == lo + 1
        return build(binding, None if audio is None else audio[lo:hi], [], shared=eff[lo], n_inst=1, **kw)

    _compare_all(orc, got, one, 1, max_abs)


# ----------------------------------------------------------------------------------------------------------- CPU: C ABI refusals
def _raw_batch(hip, n_inst, kind=None, frames=RQ * 8, oversample=0):
    """BufferSource -> WaveShaper (or `kind`) -> destination through the C ABI, plan-only"""
    nodes = (waa.api.NodeDesc * 3)()
    nodes[0].kind, nodes[1].kind, nodes[2].kind = waa.api.NODE_DESTINATION, waa.api.NODE_BUFFER_SOURCE, kind or waa.api.NODE_WAVESHAPER
    nodes[2].i[0] = oversample
    edges = (waa.api.EdgeDesc * 2)()
    edges[0].from_, edges[0].to = 1, 2
    edges[1].from_, edges[1].to = 2, 0
    g = waa.api.GraphDesc(3, nodes, 2, edges)
    h = C.c_void_p()
    hip.check(hip.batch_create(C.byref(g), n_inst, 2, frames, SR, waa.PLAN_ONLY, C.byref(h)))
    noise = white_noise(n_inst, 2, frames)
    hip.check(hip.source_set_buffer_batch(h, 1, waa.api._fp(noise), 2, frames, SR))
    return h


def _describe(hip, h):
    need = C.c_size_t()
    st = hip.plan_describe(h, None, 0, C.byref(need))
    if st:
        return st, hip.last_error().decode()
    buf = C.create_string_buffer(need.value + 1)
    hip.check(hip.plan_describe(h, buf, need.value + 1, None))
    return 0, buf.value.decode()


def test_entry_point_is_declared_and_exported(hip):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "waa_hip_device.h")).read(), flags=re.S)
    assert re.search(r"\bwaa_waveshaper_set_curve_instance\s*\(", text)
    assert "waveshaper_set_curve_instance" in waa.api.ABI_DEVICE
    assert hasattr(C.CDLL(waa.LIB_PATH), "waa_waveshaper_set_curve_instance")


def test_abi_refusals(hip):
    c3, c5 = tanh_curve(3), tanh_curve(5)
    h = _raw_batch(hip, 3)
    try:
        f = hip.waveshaper_set_curve_instance
        assert f(h, 2, 3, _fp(c3), 3) == 1 and b"instance 3 out of range" in hip.last_error()       # instance out of range
        assert f(h, 1, 0, _fp(c3), 3) == 1 and b"not of the expected kind" in hip.last_error()      # a source
        assert f(h, 7, 0, _fp(c3), 3) == 1                                                          # no such node
        assert f(h, 2, 1, _fp(c3), 0) == 1 and b"at least one point" in hip.last_error()
        # (a refused call leaves the node as it was: no curve anywhere, an identity)
        st, msg = _describe(hip, h)
        assert st == 0 and "shaper node" not in msg and "WAVESHAPER" not in msg, msg
    finally:
        hip.batch_destroy(h)
    h = _raw_batch(hip, 3)
    try:
        f = hip.waveshaper_set_curve_instance
        hip.check(f(h, 2, 1, _fp(c3), 3))
        assert f(h, 2, 1, _fp(c5), 5) == 3 and hip.last_error() == b"InvalidStateError - cannot assign curve twice"
        # ALL through the per-instance entry point is the shared call, with the shared call's refusal
        hip.check(f(h, 2, waa.api.ALL, _fp(c5), 5))
        assert f(h, 2, waa.api.ALL, _fp(c5), 5) == 3 and hip.last_error() == b"InvalidStateError - cannot assign curve twice"
        assert hip.waveshaper_set_curve(h, 2, _fp(c5), 5) == 3
        hip.check(f(h, 2, 0, _fp(c5), 5))  # (equal to the shared curve: one row of the pool)
        st, msg = _describe(hip, h)
        assert st == 0 and "shaper node 2: 2ch, one curve per instance: 2 distinct curve(s) of 3 .. 5 points, 0 instance(s) without" in msg, msg
        assert f(h, 2, 2, _fp(c3), 3) == 3 and b"frozen" in hip.last_error()                         # after the plan
    finally:
        hip.batch_destroy(h)
    for oversample, name in ((1, "2x"), (2, "4x")):
        h = _raw_batch(hip, 2, oversample=oversample)
        try:
            hip.check(hip.waveshaper_set_curve_instance(h, 2, 0, _fp(c3), 3))
            st, msg = _describe(hip, h)
            assert st == 4 and f"WaveShaperNode 2 with one curve per instance and oversample {name} is out of scope" in msg, msg
        finally:
            hip.batch_destroy(h)


def test_api_refusals(hip, orc):
    noise = white_noise(3, 2, FRAMES)
    ctx, sh = build(hip, noise, [None] * 3, shared=tanh_curve(5), device=waa.PLAN_ONLY)
    assert not sh.per_instance
    with pytest.raises(waa.WaaError, match="cannot assign curve twice") as e:
        sh.set_curve(tanh_curve(3))
    assert e.value.status == 3
    for i in (3, -2):
        with pytest.raises(waa.WaaError, match="out of range") as e:
            sh.set_curve(tanh_curve(3), instance=i)
        assert e.value.status == 1
    with pytest.raises(waa.WaaError) as e:
        sh.set_curve_batch([tanh_curve(3)] * 2)  # (two curves for three contexts)
    assert e.value.status == 1
    with pytest.raises(waa.WaaError, match="at least one point") as e:
        sh.set_curve([], instance=1)
    assert e.value.status == 1 and not sh.per_instance
    sh.set_curve(tanh_curve(7), instance=1)
    assert sh.per_instance
    with pytest.raises(waa.WaaError, match="cannot assign curve twice") as e:
        sh.set_curve(tanh_curve(9), instance=1)
    assert e.value.status == 3
    assert "2 distinct curve(s) of 5 .. 7 points" in shaper_lines(ctx)[0]
    with pytest.raises(waa.WaaError, match="frozen") as e:  # after the plan
        sh.set_curve(tanh_curve(3), instance=2)
    assert e.value.status == 3
    ctx.close()
    # set_curve_batch: lengths differ, nothing is padded
    ctx, sh = build(hip, noise, [], n_inst=3, device=waa.PLAN_ONLY)
    sh.set_curve_batch([tanh_curve(3), tanh_curve(2048), tanh_curve(4)])
    assert "3 distinct curve(s) of 3 .. 2048 points" in shaper_lines(ctx)[0]
    ctx.close()
    # the oracle keeps one curve per batch: refused, never rendered with one instance's curve
    ctx, _ = build(orc, noise, [tanh_curve(3), tanh_curve(5), tanh_curve(7)])
    with pytest.raises(waa.WaaError) as e:
        ctx.start_rendering_sync()
    assert e.value.status == 4 and "one curve per batch" in str(e.value)
    # oversampled, through api.py
    ctx = waa.OfflineAudioContext(2, FRAMES, SR, n_instances=2, binding=hip, device=waa.PLAN_ONLY)
    sh = ctx.create_wave_shaper(oversample="4x")
    sh.set_curve(tanh_curve(5), instance=1)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(noise[:2], SR)
    src.connect(sh).connect(ctx.destination())
    src.start()
    with pytest.raises(waa.WaaError, match="WaveShaperNode 1 with one curve per instance and oversample 4x is out of scope") as e:
        ctx.plan_describe()
    assert e.value.status == 4
    ctx.close()


def test_refused_inside_a_feedback_loop_and_in_a_dynamic_count_plan(hip):
    curves = [tanh_curve(5), tanh_curve(7)]
    for delay in (0.003, 0.1):  # the quantum-serial loop kernel, and a block-scheduled loop
        ctx = waa.OfflineAudioContext(2, FRAMES, SR, n_instances=2, binding=hip, device=waa.PLAN_ONLY)
        src = ctx.create_buffer_source()
        src.set_buffer_batch(white_noise(2, 2, FRAMES), SR)
        d = ctx.create_delay(0.2, delay_time=delay)
        sh = ctx.create_wave_shaper()
        sh.set_curve_batch(curves)
        fb = ctx.create_gain(gain=0.5)
        src.connect(d)
        d.connect(sh).connect(fb).connect(d)
        sh.connect(ctx.destination())
        src.start()
        with pytest.raises(waa.WaaError, match=f"WaveShaperNode {sh.id} with one curve per instance inside a feedback loop is out of scope") as e:
            ctx.plan_describe()
        assert e.value.status == 4
        ctx.close()
    # a mono and a late stereo source into one Biquad: the count of its input changes mid-render -> exact per-quantum counts
    ctx = waa.OfflineAudioContext(2, RQ * 40, SR, n_instances=2, binding=hip, device=waa.PLAN_ONLY)
    mono, stereo = ctx.create_buffer_source(), ctx.create_buffer_source()
    mono.set_buffer_batch(white_noise(2, 1, RQ * 40), SR)
    stereo.set_buffer_batch(white_noise(2, 2, RQ * 10), SR)
    flt = ctx.create_biquad_filter(type_="lowpass", frequency=900.0)
    sh = ctx.create_wave_shaper()
    sh.set_curve_batch(curves)
    mono.connect(flt)
    stereo.connect(flt)
    flt.connect(sh).connect(ctx.destination())
    mono.start()
    stereo.start_at(RQ * 9.5 / SR)
    with pytest.raises(waa.WaaError, match=f"WaveShaperNode {sh.id} with one curve per instance in a graph that needs exact per-quantum channel counts") as e:
        ctx.plan_describe()
    assert e.value.status == 4
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- CPU: plan lines
def _strip(text):
    return [re.sub(r" \| timing:.*", "", l) for l in text.splitlines()]


def test_shared_curves_plan_as_before(hip):
    """a batch whose shapers all have shared curves: the plan of the fused chain, as on the parent commit, line for line"""
    noise = white_noise(3, 2, FRAMES)
    ctx, _ = build(hip, noise, [], shared=tanh_curve(2048), n_inst=3, device=waa.PLAN_ONLY)
    assert _strip(ctx.plan_describe()) == [
        "batch: 3 instance(s) x 9001 frames (71 quanta, 5 tiles of 2048) @ 48000 Hz, 2 output channel(s)",
        "source node 2 schedule 0: quanta fast=71 fast_loop=0 slow=0 silent=0 fast_tiles=4/5",
        "source node 2 schedule 0: tiles [0, 4) are one linear run from buffer frame 0",
        "source node 2: 1 distinct schedule(s) for 3 instance(s)",
        "chain parallel C=2 in=[source:2ch]->2ch ops=[WAVESHAPER] out=2ch"]
    shared_plan = _strip(ctx.plan_describe())
    ctx.close()
    # the same curve handed to every instance as its own: the source's lines stand, the chain ends in front of the node
    ctx, _ = build(hip, noise, [tanh_curve(2048)] * 3, device=waa.PLAN_ONLY)
    per = _strip(ctx.plan_describe())
    ctx.close()
    assert per[:4] == shared_plan[:4] and per[4] == "chain parallel C=2 in=[source:2ch]->2ch ops=[] out=2ch" and "1 distinct curve(s)" in per[5], per
    ctx, _ = build(hip, None, [], shared=tanh_curve(2048), n_inst=3, graph="osc", device=waa.PLAN_ONLY)
    assert _strip(ctx.plan_describe())[1:] == [
        "oscillator node 2: sine (time-parallel, closed-form phase) frequency=const detune=const",
        "chain parallel C=2 in=[signal:1ch]->1ch ops=[GAIN,WAVESHAPER,GAIN,MIX(1->2)] out=2ch"]
    ctx.close()


def test_plan_line_counts_distinct_curves_and_names_the_form(hip):
    noise = white_noise(9, 2, FRAMES)
    curves = FORM_A + [None, FORM_A[1].copy(), FORM_A[4].copy()]  # instance 6 without a curve, 7 and 8 repeat 1 and 4
    ctx, _ = build(hip, noise, curves, device=waa.PLAN_ONLY)
    assert shaper_lines(ctx) == [f"shaper node 1: 2ch, one curve per instance: 6 distinct curve(s) of 2 .. {CAP} points, 1 instance(s) without a curve "
                                 f"pass through; form A: every instance's curve staged in LDS (cap {CAP} points) -> shaper_inst_kernel"]
    ctx.close()
    ctx, _ = build(hip, noise[:7], FORM_B, device=waa.PLAN_ONLY)  # one point above the cap: the whole node reads global memory
    assert shaper_lines(ctx) == [f"shaper node 1: 2ch, one curve per instance: 7 distinct curve(s) of 2 .. {CAP + 1} points, 0 instance(s) without a curve "
                                 f"pass through; form B: curves read from global memory (cap {CAP} points) -> shaper_inst_kernel"]
    ctx.close()
    # an instance without a curve of its own uses the shared one: three rows, one of them the shared curve's
    ctx, _ = build(hip, noise[:4], [tanh_curve(5), None, tanh_curve(9), None], shared=tanh_curve(7), device=waa.PLAN_ONLY)
    assert "3 distinct curve(s) of 5 .. 9 points, 0 instance(s) without" in shaper_lines(ctx)[0]
    ctx.close()


def test_not_folded_into_the_oscillator_and_not_taken_by_the_resample_kernel(hip):
    curves = [tanh_curve(129), tanh_curve(2048)]
    ctx, _ = build(hip, None, curves, graph="osc", device=waa.PLAN_ONLY)
    plan = _strip(ctx.plan_describe())
    ctx.close()
    # the Gain in front may ride in the oscillator's kernel; the shaper and what follows it may not
    assert plan[1:] == ["oscillator node 2: sine (time-parallel, closed-form phase) frequency=const detune=const",
                        "oscillator node 2 renders 1 gain(s) of node 3's chain itself",
                        "shaper node 1: 1ch, one curve per instance: 2 distinct curve(s) of 129 .. 2048 points, 0 instance(s) without a curve pass "
                        f"through; form A: every instance's curve staged in LDS (cap {CAP} points) -> shaper_inst_kernel",
                        "chain parallel C=2 in=[signal:1ch]->1ch ops=[GAIN,MIX(1->2)] out=2ch"], plan

    def resampled(per_instance):
        ctx = waa.OfflineAudioContext(2, FRAMES, SR, n_instances=2, binding=hip, device=waa.PLAN_ONLY)
        src = ctx.create_buffer_source()
        src.set_buffer_batch(white_noise(2, 2, FRAMES), 44100.0)  # a rate-changing source
        sh = ctx.create_wave_shaper(curve=None if per_instance else curves[0])
        if per_instance:
            sh.set_curve_batch(curves)
        src.connect(sh).connect(ctx.destination())
        src.start()
        text = ctx.plan_describe()
        ctx.close()
        return text

    shared, per = resampled(False), resampled(True)
    assert "ops=[WAVESHAPER]" in shared and "shaper node" not in shared, shared
    assert "ops=[] out=2ch" in per and "ops=[WAVESHAPER]" not in per and "-> shaper_inst_kernel" in per, per


def test_the_centre_of_the_instances_own_curve_enters_the_count_replay(hip):
    """source (stereo, ends inside the render) -> shaper -> Biquad -> destination.  A curve whose centre is not 0 turns the silence
    behind the source into an active MONO signal (waveshaper.rs:498-509), which the stereo Biquad behind it must see as a change of
    its input's channel count.  Only instance 1 has such a curve: its flag has to reach the replay (read from ITS curve) and the
    signature (else instance 1 is taken for a copy of instance 0 and never simulated).  The plan reports what the replay found: with
    centres of 0 everywhere it stands; with instance 1's lifted curve the replay finds the change and asks for the dynamic-count plan, which
    does not render this node: status 4, naming the node."""
    def plan(curves):
        ctx = waa.OfflineAudioContext(2, RQ * 40, SR, n_instances=2, binding=hip, device=waa.PLAN_ONLY)
        src = ctx.create_buffer_source()
        src.set_buffer_batch(white_noise(2, 2, RQ * 10), SR)
        sh = ctx.create_wave_shaper()
        sh.set_curve_batch(curves)
        flt = ctx.create_biquad_filter(type_="lowpass", frequency=900.0)
        src.connect(sh).connect(flt).connect(ctx.destination())
        src.start()
        assert sh.id == 2
        try:
            return 0, ctx.plan_describe()
        except waa.WaaError as e:
            return e.status, str(e)
        finally:
            ctx.close()

    st, text = plan([tanh_curve(129), tanh_curve(129, 3.0)])
    assert st == 0 and "shaper node 2" in text and "channel count changes" not in text, text
    st, text = plan([tanh_curve(129), lifted_curve(129)])
    # (the dynamic-count plan the finding asks for does not render this node: the refusal is the report)
    assert st == 4 and "WaveShaperNode 2 with one curve per instance in a graph that needs exact per-quantum channel counts" in text, text
    st, text = plan([lifted_curve(129), tanh_curve(129)])
    assert st == 4, text
    # 9.9e-10 is "zero" to the reference, 1.1e-9 is not: the threshold of waveshaper.rs:501
    st, text = plan([tanh_curve(129), np.asarray([-1.0, 9.9e-10, 1.0], np.float32)])
    assert st == 0, text
    st, text = plan([tanh_curve(129), np.asarray([-1.0, 1.1e-9, 1.0], np.float32)])
    assert st == 4, text


# ------------------------------------------------------------------------------------------------------------------ CPU: mixed.py
def _single(binding, curve, seed, device=waa.PLAN_ONLY, oversample="none", frames=FRAMES):
    c = waa.OfflineAudioContext(2, frames, SR, binding=binding, device=device)
    s = c.create_buffer_source()
    s.set_buffer(waa.AudioBuffer(probe_noise(1, 2, frames, seed)[0], SR))
    s.connect(c.create_wave_shaper(curve=curve, oversample=oversample)).connect(c.destination())
    s.start()
    return c


MIXED_CURVES = [tanh_curve(129), tanh_curve(2048, 3.0), tanh_curve(129), lifted_curve(4), tanh_curve(3)]  # five contexts, four curves


def test_mixed_contexts_that_differ_in_curves_share_a_batch(hip, orc):
    from web_audio_api_rs_amd import mixed
    ctxs = [_single(hip, c, seed=i) for i, c in enumerate(MIXED_CURVES)]
    assert mixed.bucket_report(ctxs) == [[0, 1, 2, 3, 4]]
    batch = mixed._merge(ctxs)
    sh = [n for n in batch._nodes if isinstance(n, waa.api.WaveShaperNode)][0]
    assert batch.n_instances == 5 and sh.per_instance
    for i, c in enumerate(MIXED_CURVES):
        assert np.array_equal(sh._inst_curves[i], c)
    assert "4 distinct curve(s) of 3 .. 2048 points" in shaper_lines(batch)[0]
    batch.close()
    # equal curves: one batch whose node stays shared, planned as ever
    ctxs = [_single(hip, MIXED_CURVES[0], seed=i) for i in range(3)]
    assert mixed.bucket_report(ctxs) == [[0, 1, 2]]
    batch = mixed._merge(ctxs)
    sh = [n for n in batch._nodes if isinstance(n, waa.api.WaveShaperNode)][0]
    assert not sh.per_instance and not shaper_lines(batch) and "ops=[WAVESHAPER]" in batch.plan_describe()
    batch.close()
    # a context without a curve is another shape; other bindings and oversampled shapers keep the digests in the key
    assert mixed.bucket_report([_single(hip, MIXED_CURVES[0], 0), _single(hip, None, 1)]) == [[0], [1]]
    assert mixed.bucket_report([_single(orc, c, seed=i, device=-1) for i, c in enumerate(MIXED_CURVES)]) == [[0, 2], [1], [3], [4]]
    assert mixed.bucket_report([_single(hip, c, seed=i, oversample="2x") for i, c in enumerate(MIXED_CURVES)]) == [[0, 2], [1], [3], [4]]
    assert mixed.bucket_report([_single(hip, MIXED_CURVES[0], 0), _single(hip, MIXED_CURVES[1], 1, oversample="4x")]) == [[0], [1]]
    # a single context that already holds an instance-0 curve is keyed and merged by the curve it renders with
    own = _single(hip, None, 1)
    own._nodes[-1].set_curve(MIXED_CURVES[3], instance=0)
    ctxs = [_single(hip, MIXED_CURVES[0], 0), own]
    assert mixed.bucket_report(ctxs) == [[0, 1]]
    batch = mixed._merge(ctxs)
    sh = [n for n in batch._nodes if isinstance(n, waa.api.WaveShaperNode)][0]
    assert np.array_equal(sh._inst_curves[0], MIXED_CURVES[0]) and np.array_equal(sh._inst_curves[1], MIXED_CURVES[3])
    batch.close()


# -------------------------------------------------------------------------------------------------------------- CPU: registers
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_kernel_registers_and_no_scratch(tmp_path):
    """waa_shaper_inst.hip compiled to ISA with the library's flags, read like tests/test_convolver_per_instance.py reads it: both forms
    spill nothing and use no scratch memory; at most 64 vector registers, so that registers never limit the eight wavefronts per SIMD
    a streaming kernel wants; no static LDS (the curve's is dynamic, sized to the node's longest curve)"""
    out = str(tmp_path / "waa_shaper_inst.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fgpu-flush-denormals-to-zero",
                           "--cuda-device-only", "-S", os.path.join(CSRC, "waa_shaper_inst.hip"), "-o", out], stderr=subprocess.DEVNULL)
    res = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)(.*?)\.wavefront_size", open(out).read(), re.S):  # (one kernel's metadata, keys in order)
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(2)).group(1))  # noqa: E731
        res[re.search(r"\.name:\s+(\S+)", m.group(2)).group(1)] = {
            "vgpr": get("vgpr_count"), "spill": get("vgpr_spill_count"), "sgpr_spill": get("sgpr_spill_count"),
            "scratch": get("private_segment_fixed_size"), "lds": int(m.group(1))}
    forms = {k: v for k, v in res.items() if "shaper_inst_kernel" in k}
    assert sorted(forms) == ["_ZN3waa18shaper_inst_kernelILb0EEEvNS_14ShaperInstDescE", "_ZN3waa18shaper_inst_kernelILb1EEEvNS_14ShaperInstDescE"], res
    for name, r in forms.items():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0 and r["vgpr"] <= 64, (name, r)


# ------------------------------------------------------------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("graph", ["source", "osc"])
@pytest.mark.parametrize("form", ["A", "B"])
def test_bit_equal_to_the_shared_path_and_close_to_the_oracle(hip, orc, graph, form):
    """every curve length (2, 3, 4, 129, 2048, the cap; form B: and cap + 1), one instance without a curve, two with equal curves; the
    source's samples include -1, 0, +1, both clamps, knots and their neighbours"""
    curves = (FORM_A if form == "A" else FORM_B) + [None, tanh_curve(129, 1.5)]
    if graph == "osc":  # (slopes <= 1: the oscillator's own distance from the oracle's sine is not amplified)
        curves = [None if c is None else tanh_curve(c.size, 1.0) for c in curves]
    audio = probe_noise(len(curves), 2, FRAMES, seed0=11) if graph == "source" else None
    if audio is not None:
        audio[-1] = audio[3]  # (the two instances with equal curves: equal audio, equal output)
    got = render_per_instance(hip, audio, curves, expect_form=form, graph=graph)
    ref = shared_each(hip, audio, curves, graph=graph)
    assert_words(got, ref, f"{graph}, form {form}")
    if graph == "source":  # the instance without a curve: its input (as words it is the shared path's copy, above, which makes the probe's -0 a +0)
        k = [i for i, c in enumerate(curves) if c is None][0]
        assert np.array_equal(got[k], audio[k])
    assert np.array_equal(got[3], got[-1]) and np.abs(got[3] - got[0]).max() > 1e-3
    assert_oracle(orc, got, audio, curves, graph=graph, max_abs=1e-6 if graph == "source" else 5e-6)


@gpu
@pytest.mark.parametrize("n_inst,channels", [(3, 1), (3, 6), (67, 2), (67, 8)])
def test_instances_and_channels(hip, orc, n_inst, channels):
    """3 and 67 instances, 1 / 2 / 6 / 8 channels (every channel with the instance's one staged curve); the shared curve under two
    instances without one of their own"""
    lengths = [2, 3, 4, 129, 2048, 33, 1000]
    curves = [tanh_curve(lengths[i % 7], 1.0 + 0.05 * i) for i in range(n_inst)]
    curves[1] = None
    shared = lifted_curve(65, -0.7, 0.9)
    frames = 5003
    audio = probe_noise(n_inst, channels, frames, seed0=100 + channels)
    kw = dict(channels=channels, length=frames)
    got = render_per_instance(hip, audio, curves, shared=shared, **kw)
    ref = shared_each(hip, audio, curves, shared=shared, **kw)
    assert_words(got, ref, f"{n_inst} instances, {channels} channel(s)")
    assert_oracle(orc, got, audio, curves, shared=shared, **kw)


@gpu
def test_a_source_read_in_place_that_ends_inside_the_render(hip, orc):
    """the buffer (10 quanta) is shorter than the render and rendered unchanged: the kernel reads it in place, frames past its end are
    silence (in_valid) — which a lifted curve turns into its centre value"""
    curves = [tanh_curve(129), lifted_curve(4), lifted_curve(129), None]
    audio = white_noise(4, 2, RQ * 10, seed0=21)
    kw = dict(length=5003)
    ctx, _ = build(hip, audio, curves, **kw)
    plan = ctx.plan_describe()
    assert "source node 2 renders its AudioBuffer unchanged: node 1 reads it in place (1280 frames per channel)" in plan and shaper_lines(ctx), plan
    got = render(ctx)
    assert np.all(got[1][:, RQ * 10:] == centre(curves[1])) and np.all(got[2][:, RQ * 10:] == centre(curves[2]))
    assert np.all(got[0][:, RQ * 10:] == 0.0) and np.all(got[3][:, RQ * 10:] == 0.0) and np.array_equal(got[3][:, :RQ * 10], audio[3])
    assert_words(got, shared_each(hip, audio, curves, **kw), "source read in place")
    assert_oracle(orc, got, audio, curves, **kw)


@gpu
def test_a_source_that_starts_late_in_front_of_a_lifted_curve(hip, orc):
    curves = [lifted_curve(129), lifted_curve(4, -0.3, 0.9), tanh_curve(129)]
    audio = probe_noise(3, 2, 5003, seed0=22)
    kw = dict(start=RQ * 9.5 / SR)
    got = render_per_instance(hip, audio, curves, **kw)
    assert np.all(got[0][:, :RQ * 9] == centre(curves[0])) and np.all(got[1][:, :RQ * 9] == centre(curves[1])) and np.all(got[2][:, :RQ * 9] == 0.0)
    assert_words(got, shared_each(hip, audio, curves, **kw), "late source")
    assert_oracle(orc, got, audio, curves, **kw)


def _composed(binding, audio, curves_a, curves_b, ir, which, shared=False):
    """which = "biquad-conv": source -> Biquad -> shaper A -> Convolver -> destination
               "two":         source -> shaper A -> shaper B -> destination
               "fan-out":     source -> shaper A -> {Gain 0.5, Biquad} -> destination
               "with-shared": source -> shaper (shared curve curves_b[0]) -> Gain -> shaper A -> destination
    shared: every instance renders with curves_a[0] / curves_b[0] as the nodes' SHARED curves (the fused path)"""
    ctx = waa.OfflineAudioContext(2, audio.shape[2], SR, n_instances=audio.shape[0], binding=binding)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(audio, SR)

    def shaper(curves):
        sh = ctx.create_wave_shaper(curve=curves[0] if shared else None)
        if not shared:
            sh.set_curve_batch(curves)
        return sh

    a = shaper(curves_a)
    dest = ctx.destination()
    if which == "biquad-conv":
        cv = ctx.create_convolver(buffer=waa.AudioBuffer(ir, SR))
        src.connect(ctx.create_biquad_filter(type_="lowpass", frequency=2500.0)).connect(a).connect(cv).connect(dest)
    elif which == "two":
        src.connect(a).connect(shaper(curves_b)).connect(dest)
    elif which == "fan-out":
        src.connect(a)
        a.connect(ctx.create_gain(gain=0.5)).connect(dest)
        a.connect(ctx.create_biquad_filter(type_="highpass", frequency=700.0)).connect(dest)
    else:
        src.connect(ctx.create_wave_shaper(curve=curves_b[0])).connect(ctx.create_gain(gain=0.8)).connect(a).connect(dest)
    src.start()
    return ctx, a


@gpu
@pytest.mark.parametrize("which", ["biquad-conv", "two", "fan-out", "with-shared"])
def test_composition(hip, orc, which):
    """instance k against the SAME batch rendered with instance k's curves as the nodes' shared curves (every other kernel of the plan
    is then chosen for the same batch: bit for bit), and every instance against the oracle, one context at a time.  Behind the Convolver
    the words are not compared: its FFT kernels transform the instances of a batch in PAIRS, one complex transform per two instances
    (waa_plan_conv.cpp: n_pairs), so the roundoff of instance k (1e-8 here) depends on what its neighbour holds — which is another
    signal when the neighbour renders with curve k than when it renders with its own; the unpaired last instance is equal.  max |d|: 2e-6 (sums of
    two terms below 2: an ulp is 2.4e-7), behind the 300-tap Convolver 1e-5 (300 f32 products accumulated: sqrt(300) ulps of its peak)"""
    n = 3
    audio = white_noise(n, 2, 5003, seed0=31) * np.float32(0.9)
    curves_a = [tanh_curve(129), tanh_curve(4, 1.0), tanh_curve(2048, 3.0)]
    curves_b = [tanh_curve(33, 1.0)] * n if which == "with-shared" else [tanh_curve(5), tanh_curve(2048, 1.5), tanh_curve(2)]
    rng = np.random.default_rng(5)
    ir = (rng.standard_normal((2, 300)) * np.exp(-np.arange(300) / 60.0)).astype(np.float32)
    ctx, _ = _composed(hip, audio, curves_a, curves_b, ir, which)
    assert len(shaper_lines(ctx)) == (2 if which == "two" else 1), ctx.plan_describe()
    got = render(ctx)
    ref = None if which == "biquad-conv" else np.stack([render(_composed(hip, audio, curves_a[k:k + 1], curves_b[k:k + 1], ir, which, shared=True)[0])[k]
                                                        for k in range(n)])
    if which != "biquad-conv":
        assert_words(got, ref, which)
    _compare_all(orc, got, lambda be, lo, hi: _composed(be, audio[lo:hi], curves_a[lo:hi], curves_b[lo:hi], ir, which, shared=True), 1,
                 1e-5 if which == "biquad-conv" else 2e-6)


@gpu
def test_rearm_keeps_the_curves(hip):
    from rearm import assert_differs, assert_same_bits, dense, other_dense, refill_from, render_again
    curves = FORM_A[:5] + [None]
    a, b2 = dense(6, 2, 5003), other_dense(6, 2, 5003)
    kw = dict(length=5003)
    ctx, _ = build(hip, a, curves, **kw)
    assert shaper_lines(ctx)
    first = ctx.start_rendering_sync().data
    donor, _ = build(hip, b2, curves, **kw)  # (never applied: only its audio is taken)
    assert refill_from(ctx, donor) == 1
    again = render_again(ctx)
    ctx.close()
    assert_differs(again, first)
    assert_same_bits(again, render_per_instance(hip, b2, curves, **kw))


@gpu
def test_render_sharded_installs_each_sub_batch_its_slice(hip):
    """two sub-batches whose setup installs the curves [first, first + count): equal to the one-batch render"""
    curves = [tanh_curve(n, 1.0 + 0.3 * i) for i, n in enumerate((2, 129, 2048, 3, 4, 1000))]
    audio = white_noise(6, 2, 5003, seed0=41)
    want = render_per_instance(hip, audio, curves, length=5003)

    def build_sub(n_instances, device, first=0):
        ctx = waa.OfflineAudioContext(2, 5003, SR, n_instances=n_instances, binding=hip, device=device)
        src = ctx.create_buffer_source()
        sh = ctx.create_wave_shaper()
        sh.set_curve_batch(curves[first:first + n_instances])
        src.connect(sh).connect(ctx.destination())
        src.start()
        return ctx, src

    out = np.zeros_like(want)
    from web_audio_api_rs_amd.sharding import render_sharded
    info = render_sharded(build_sub, audio, out, devices=[0], sub_batches=2, sample_rate=SR, pass_first=True)
    assert len(info["shards"]) == 2, info
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


@gpu
def test_mixed_render_contexts_equals_five_separate_renders(hip):
    from web_audio_api_rs_amd import mixed
    alone = [render(_single(hip, c, seed=i, device=-1, frames=5003)) for i, c in enumerate(MIXED_CURVES)]
    ctxs = [_single(hip, c, seed=i, device=-1, frames=5003) for i, c in enumerate(MIXED_CURVES)]
    assert mixed.bucket_report(ctxs) == [[0, 1, 2, 3, 4]]
    together = mixed.render_contexts(ctxs)
    for i in range(5):
        assert_words(together[i].data, alone[i], f"context {i}")
