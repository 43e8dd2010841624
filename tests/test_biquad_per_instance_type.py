"""BiquadFilterNode with one filter TYPE per context of a batch (waa_biquad_set_type_instance, include/waa_hip_device.h).

CPU part: the refusals of the C ABI and of api.py, the rule that keeps existing plans (every instance given the same type plans word
for word as the shared option), the plan lines of batches whose types differ, mixed.py's buckets, get_frequency_response per instance,
the code object of the new kernel.

GPU part (-m gpu): (1) the SAME BITS as a single-type batch: for every type T of a mixed batch the same batch is rendered with the
shared type T, and every context of type T is compared as uint32 words — the constant and k-rate rows come from one host function, the
per-frame rows from one device function (biquad_coef_element, waa_biquad_coef.hpp), read by the same consumer kernel, so nothing but
equality is right.  (2) The one form (1) cannot hold that way, a SHARED a-rate automation under differing types (a single-type batch
takes the shared-table kernels), against tests/biquad_model.py and the oracle with the inputs and bounds of
tests/test_biquad_a_rate_types.py.  (3) Every renderer that reads the coefficient rows, each a small graph against the oracle rendered
ONE CONTEXT AT A TIME with that context's type (its binding keeps one type per batch), at the bound of the existing test of that
renderer.  (4) re-arm, (5) mixed.render_contexts, (6) render_sharded.

Contexts: 11 with type i % 8 (all eight types, three repeats, neighbours always differ) and 67 (more than a wavefront of contexts),
each with its own frequency, Q and gain, so that no two contexts share a coefficient row."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import biquad_model as bm
import web_audio_api_rs_amd as waa
from graphs import assert_all_finite, assert_le, rms_err, white_noise
from test_biquad_a_rate_types import MAX_TOL, TOL, case_params, noise

RQ = 128
SR = 48000.0
FRAMES = 2 * 2048 + 3 * RQ + 9  # two full tiles, the table's padded tail, a last partial quantum (tests/test_biquad_a_rate_types.py)
NQ = (FRAMES + RQ - 1) // RQ
TYPES = tuple(waa.BIQUAD_TYPE)  # in the order of their numbers
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-audio-api-rs_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
gpu = pytest.mark.gpu
NOTE = "one type per instance:"
assert TYPES == bm.TYPES and [waa.BIQUAD_TYPE[t] for t in TYPES] == list(range(8))


def types_of(n, reverse=False):
    return [TYPES[7 - i % 8 if reverse else i % 8] for i in range(n)]


def counts(types):
    return " ".join(f"{t} x{types.count(t)}" for t in TYPES if t in types)


def freq_of(i):
    return float(np.float32(300.0 * 1.06 ** i))  # 300 Hz .. 14 kHz over 67 contexts


def q_of(i):
    return float(np.float32(0.7 + 0.05 * i))


def gain_of(i):
    return float(np.float32(-6.0 + 0.25 * i))


def set_params(bq, idx, form):
    """context idx[k] -> instance k: its own frequency, Q and gain; form "k-rate": one frequency per quantum and instance, "a-rate":
    one per frame and instance (a sweep of its own), "const": constants only"""
    for k, i in enumerate(idx):
        bq.frequency.set_value(freq_of(i), instance=k)
        bq.q.set_value(q_of(i), instance=k)
        bq.gain.set_value(gain_of(i), instance=k)
        if form == "k-rate":
            bq.frequency.set_block(0, np.geomspace(freq_of(i), 3.0 * freq_of(i) / (1 + i % 3), NQ).astype(np.float32), instance=k)
        elif form == "a-rate":
            bq.frequency.set_block(0, np.geomspace(freq_of(i), 20000.0, NQ * RQ).astype(np.float32).reshape(NQ, RQ), instance=k)


def give_types(binding, bq, types, idx):
    """the device batch: every instance its own type; another binding renders one context (or one type) at a time"""
    mine = [types[i] for i in idx]
    if binding.prefix == "waa_" and len(set(mine)) > 1:
        bq.set_type_batch(mine)
    else:
        assert len(set(mine)) == 1, mine
        bq.set_type(mine[0])


def chain(binding, audio, types, idx=None, form="const", device=-1, length=None):
    """BufferSource -> Biquad -> Gain(0.5) -> destination; idx: the contexts this batch holds (default all of `audio`)"""
    idx = list(range(audio.shape[0])) if idx is None else list(idx)
    ctx = waa.OfflineAudioContext(2, length or audio.shape[2], SR, n_instances=len(idx), binding=binding, device=device)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(np.ascontiguousarray(audio[idx]), SR)
    bq = ctx.create_biquad_filter()
    give_types(binding, bq, types, idx)
    set_params(bq, idx, form)
    src.connect(bq).connect(ctx.create_gain(gain=0.5)).connect(ctx.destination())
    src.start()
    return ctx, bq


def render(ctx):
    out = ctx.start_rendering_sync().data
    ctx.close()
    return out


def plan_lines(ctx):
    """the plan's text without the timing figures of its first line"""
    lines = ctx.plan_describe().splitlines()
    return [lines[0].split(" | timing:")[0]] + lines[1:]


def oracle_each(orc, build, n):
    """the oracle, one context at a time, each with its own type as ITS shared type"""
    outs = []
    for i in range(n):
        outs.append(render(build(orc, [i]))[0])
    return np.stack(outs)


def assert_words(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32
    diff = got.view(np.uint32) != ref.view(np.uint32)
    if diff.any():
        k = tuple(int(v) for v in np.unravel_index(int(np.argmax(diff)), diff.shape))
        raise AssertionError(f"{what}: {int(diff.sum())} of {got.size} words differ from the single-type batch; the first at (context, channel, "
                             f"frame) {k}: {got[k]!r} against {ref[k]!r}")


def assert_oracle(got, ref, what, rms_tol, max_tol, scaled=False):
    """per (context, channel) RMS and max |d| against the oracle; scaled: both bounds times max(1, peak(oracle))"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert_all_finite(got, what + ": device")
    assert_all_finite(ref, what + ": oracle")
    scale = max(1.0, float(np.abs(ref).max())) if scaled else 1.0
    r, m = float(rms_err(got, ref).max()), float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{what}: worst RMS {r:.3e} (bar {rms_tol * scale:.1e}), max |d| {m:.3e} (bar {max_tol * scale:.1e}), peak {np.abs(ref).max():.3f}")
    assert float(np.abs(ref).max()) > 1e-3
    assert_le(r, rms_tol * scale, what + ": RMS per context and channel")
    assert_le(m, max_tol * scale, what + ": max |d|")


# ----------------------------------------------------------------------------------------------------------- CPU: the C ABI
def _raw_batch(hip, n_inst, kind=None, frames=RQ * 8, type_=0):
    """BufferSource -> Biquad (or `kind`) -> destination through the C ABI, plan-only (tests/test_waveshaper_per_instance.py)"""
    nodes = (waa.api.NodeDesc * 3)()
    nodes[0].kind, nodes[1].kind, nodes[2].kind = waa.api.NODE_DESTINATION, waa.api.NODE_BUFFER_SOURCE, kind or waa.api.NODE_BIQUAD
    nodes[2].i[0] = type_
    edges = (waa.api.EdgeDesc * 2)()
    edges[0].from_, edges[0].to = 1, 2
    edges[1].from_, edges[1].to = 2, 0
    g = waa.api.GraphDesc(3, nodes, 2, edges)
    h = C.c_void_p()
    hip.check(hip.batch_create(C.byref(g), n_inst, 2, frames, SR, waa.PLAN_ONLY, C.byref(h)))
    hip.check(hip.source_set_buffer_batch(h, 1, waa.api._fp(white_noise(n_inst, 2, frames)), 2, frames, SR))
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
    assert re.search(r"\bwaa_biquad_set_type_instance\s*\(", text)
    assert "biquad_set_type_instance" in waa.api.ABI_DEVICE
    assert hasattr(C.CDLL(waa.LIB_PATH), "waa_biquad_set_type_instance")


def test_abi_refusals(hip):
    ALL = waa.api.ALL
    h = _raw_batch(hip, 3)
    try:
        f = hip.biquad_set_type_instance
        assert f(h, 2, 3, 1) == 1 and b"instance 3 out of range (BiquadFilterNode 2, 3 instances)" in hip.last_error()
        assert f(h, 1, 0, 1) == 1 and b"not of the expected kind" in hip.last_error()  # a source
        assert f(h, 7, 0, 1) == 1                                                      # no such node
        for bad in (-1, 8, 100):
            assert f(h, 2, 1, bad) == 1 and hip.last_error() == b"bad biquad type", bad
            assert f(h, 2, ALL, bad) == 1 and hip.last_error() == b"bad biquad type", bad
        # (a refused call leaves the node as it was: one type everywhere, no note)
        st, msg = _describe(hip, h)
        assert st == 0 and NOTE not in msg, msg
        assert f(h, 2, 1, 3) == 3 and b"frozen" in hip.last_error()  # InvalidStateError once the batch is planned
    finally:
        hip.batch_destroy(h)
    h = _raw_batch(hip, 2, kind=waa.api.NODE_GAIN)
    try:
        assert hip.biquad_set_type_instance(h, 2, 0, 1) == 1 and b"not of the expected kind" in hip.last_error()
    finally:
        hip.batch_destroy(h)


def _raw_note(hip, calls, n_inst=4, type_=0):
    h = _raw_batch(hip, n_inst, type_=type_)
    try:
        for inst, t in calls:
            hip.check(hip.biquad_set_type_instance(h, 2, inst, t))
        st, msg = _describe(hip, h)
        assert st == 0, msg
        notes = [l for l in msg.splitlines() if NOTE in l]
        assert len(notes) <= 1, msg
        return notes[0] if notes else None
    finally:
        hip.batch_destroy(h)


def test_all_and_single_instances_in_either_order(hip):
    ALL = waa.api.ALL
    # ALL, then single instances: the singles keep theirs, the others follow ALL
    assert _raw_note(hip, [(ALL, 5), (1, 2), (3, 7)]) == "biquad node 2: one type per instance: bandpass x1 peaking x2 highshelf x1"
    # single instances, then ALL: ALL leaves the types given to single instances alone
    assert _raw_note(hip, [(1, 2), (3, 7), (ALL, 5)]) == "biquad node 2: one type per instance: bandpass x1 peaking x2 highshelf x1"
    # an instance without a type of its own uses the shared one of waa_batch_create
    assert _raw_note(hip, [(0, 6)], type_=1) == "biquad node 2: one type per instance: highpass x3 lowshelf x1"
    # a second call for one instance wins
    assert _raw_note(hip, [(0, 6), (0, 4), (2, 3), (2, 4)], type_=1) == "biquad node 2: one type per instance: highpass x2 allpass x2"
    # ... also back to the shared type: no instance differs, no note
    assert _raw_note(hip, [(0, 6), (0, 1)], type_=1) is None
    assert _raw_note(hip, [(ALL, 3), (ALL, 4)]) is None


# ------------------------------------------------------------------------------------------------------------- CPU: api.py
def test_api_calls_and_refusals(hip, orc):
    audio = white_noise(3, 2, FRAMES)
    ctx, bq = chain(hip, audio, ["lowpass"] * 3, device=waa.PLAN_ONLY)
    assert not bq.per_instance and bq.type_of(2) == "lowpass"
    for i in (3, -2):
        with pytest.raises(waa.WaaError, match="out of range") as e:
            bq.set_type("notch", instance=i)
        assert e.value.status == 1
        with pytest.raises(waa.WaaError, match="out of range"):
            bq.type_of(i)
    with pytest.raises(waa.WaaError, match="bad biquad type") as e:
        bq.set_type("brickwall", instance=1)
    assert e.value.status == 1 and not bq.per_instance
    with pytest.raises(waa.WaaError) as e:
        bq.set_type_batch(["notch"] * 2)  # (two types for three contexts)
    assert e.value.status == 1 and not bq.per_instance
    bq.set_type("notch", instance=1).set_type("peaking", instance=1)  # (the last call wins)
    bq.set_type("allpass")
    assert bq.per_instance and [bq.type_of(i) for i in range(3)] == ["allpass", "peaking", "allpass"]
    assert [l for l in plan_lines(ctx) if NOTE in l] == ["biquad node 2: one type per instance: allpass x2 peaking x1"]
    with pytest.raises(waa.WaaError, match="frozen") as e:  # after the plan
        bq.set_type("notch", instance=2)
    assert e.value.status == 3
    ctx.close()
    # the oracle keeps one type per batch: differing types are refused, never rendered with one instance's type
    ctx, bq = chain(orc, audio, ["lowpass"] * 3)
    bq.set_type_batch(["lowpass", "highpass", "lowpass"])
    with pytest.raises(waa.WaaError) as e:
        ctx.start_rendering_sync()
    assert e.value.status == 4 and "one type per batch" in str(e.value)
    # ... and equal ones collapse to the shared option and render
    ctx, bq = chain(orc, audio, ["lowpass"] * 3)
    bq.set_type_batch(["highshelf"] * 3)
    got = render(ctx)
    ref = render(chain(orc, audio, ["highshelf"] * 3)[0])
    assert np.array_equal(got, ref) and float(np.abs(ref).max()) > 1e-3
    assert not np.array_equal(ref, render(chain(orc, audio, ["lowpass"] * 3)[0]))


def test_frequency_response_per_instance(hip):
    hz = np.geomspace(10.0, 30000.0, 97).astype(np.float32)  # (past Nyquist too: NaN there)
    ctx, bq = chain(hip, white_noise(11, 2, RQ), types_of(11), device=waa.PLAN_ONLY)
    for i, t in enumerate(types_of(11)):
        one = waa.OfflineAudioContext(2, RQ, SR, binding=hip, device=waa.PLAN_ONLY)
        ref = one.create_biquad_filter(type_=t, frequency=freq_of(i), q=q_of(i), gain=gain_of(i)).get_frequency_response(hz)
        got = bq.get_frequency_response(hz, instance=i)
        for g, r in zip(got, ref):
            assert np.array_equal(g, r, equal_nan=True), (i, t)
        one.close()
    # ALL: the shared type and the shared constants, as before
    one = waa.OfflineAudioContext(2, RQ, SR, binding=hip, device=waa.PLAN_ONLY)
    ref = one.create_biquad_filter().get_frequency_response(hz)
    for g, r in zip(bq.get_frequency_response(hz), ref):
        assert np.array_equal(g, r, equal_nan=True)
    ctx.close()


# --------------------------------------------------------------------------------------------- CPU: the rule that keeps existing plans
def a_rate_shared(binding, audio, types, idx=None, device=-1, case="sweep"):
    """BufferSource -> Biquad -> destination with ONE a-rate automation for the whole batch: the blocks of a case of
    tests/test_biquad_a_rate_types.py.  Its gain constant is 6 dB for the three types that read it and 0 for the others, which do
    not: 6 dB for every context is the same filters, and keeps the four params independent of the instance."""
    idx = list(range(audio.shape[0])) if idx is None else list(idx)
    params = dict(case_params(case, "peaking")[0])
    ctx = waa.OfflineAudioContext(2, FRAMES, SR, n_instances=len(idx), binding=binding, device=device)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(np.ascontiguousarray(audio[idx]), SR)
    bq = ctx.create_biquad_filter(**{k: (v if np.isscalar(v) else v[0]) for k, v in params.items()})
    for name, v in params.items():
        if not np.isscalar(v):
            getattr(bq, name).set_block(v[1], v[2])
    give_types(binding, bq, types, idx)
    src.connect(bq).connect(ctx.destination())
    src.start()
    return ctx, bq


def folded(binding, audio, types, idx=None, device=-1, taps=60000):
    """BufferSource -> Biquad (the same constants on every context) -> ConvolverNode with a long response: the shape whose Biquad
    the planner folds into the impulse response"""
    idx = list(range(audio.shape[0])) if idx is None else list(idx)
    ctx = waa.OfflineAudioContext(2, audio.shape[2], SR, n_instances=len(idx), binding=binding, device=device)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(np.ascontiguousarray(audio[idx]), SR)
    bq = ctx.create_biquad_filter(frequency=900.0, q=1.3, gain=3.0)
    give_types(binding, bq, types, idx)
    src.connect(bq).connect(ctx.create_convolver(buffer=waa.AudioBuffer(decaying_ir(2, taps), SR))).connect(ctx.destination())
    src.start()
    return ctx, bq


def decaying_ir(n_ch, taps, seed=3, tau=0.3):
    rng = np.random.default_rng(seed)
    t = np.arange(taps) / max(taps, 1)
    return (rng.uniform(-1, 1, (n_ch, taps)) * np.exp(-t / tau)).astype(np.float32)


@pytest.mark.parametrize("graph,marker", [("const", "biquad_stream in=source:2ch"), ("k-rate", "biquad_stream(k-rate)"),
                                          ("a-rate-shared", "biquad_lanes(a-rate, shared table"),
                                          ("folded", "folded into the impulse response")])
def test_equal_types_plan_as_the_shared_option(hip, graph, marker):
    """every instance set one by one to the same type (not the type the batch was created with): the plan's text is the shared
    option's, line for line"""
    n = 5
    audio = white_noise(n, 2, RQ * 64 if graph == "folded" else FRAMES)

    def build(types, one_by_one):
        if graph == "a-rate-shared":
            ctx, bq = a_rate_shared(hip, audio, types, device=waa.PLAN_ONLY)
        elif graph == "folded":
            ctx, bq = folded(hip, audio, types, device=waa.PLAN_ONLY)
        else:
            ctx, bq = chain(hip, audio, types, form=graph, device=waa.PLAN_ONLY)
        if one_by_one:
            bq.set_type("lowpass")
            for i in range(n):
                bq.set_type("peaking", instance=i)
            assert bq.per_instance
        lines = plan_lines(ctx)
        ctx.close()
        return lines

    shared = build(["peaking"] * n, False)
    assert any(marker in l for l in shared), shared
    assert build(["peaking"] * n, True) == shared
    assert not any(NOTE in l for l in shared)


def test_differing_types_plan_lines(hip):
    types = types_of(11)
    audio = white_noise(11, 2, FRAMES)
    for form in ("const", "k-rate"):
        ctx, _ = chain(hip, audio, types, form=form, device=waa.PLAN_ONLY)
        lines = plan_lines(ctx)
        ctx.close()
        assert [l for l in lines if NOTE in l] == [f"biquad node 2: one type per instance: {counts(types)}"], lines
        assert any(l.startswith("biquad_stream(k-rate)" if form == "k-rate" else "biquad_stream in=") for l in lines), lines
    # per-instance a-rate blocks: the table was per instance already
    ctx, _ = chain(hip, audio, types, form="a-rate", device=waa.PLAN_ONLY)
    lines = plan_lines(ctx)
    ctx.close()
    assert [l for l in lines if NOTE in l] == [f"biquad node 2: one type per instance: {counts(types)}; a-rate"], lines
    assert any("biquad_stream(a-rate, per-instance table)" in l for l in lines), lines
    # one shared a-rate automation: the single-type batch shares one table, the mixed one cannot
    ctx, _ = a_rate_shared(hip, audio, types, device=waa.PLAN_ONLY)
    lines = plan_lines(ctx)
    ctx.close()
    assert [l for l in lines if NOTE in l] == [
        f"biquad node 2: one type per instance: {counts(types)}; a-rate: the coefficient table is per instance because of the types"], lines
    assert any("biquad_stream(a-rate, per-instance table)" in l for l in lines) and not any("shared table" in l for l in lines), lines


def test_differing_types_refuse_the_response_fold(hip):
    audio = white_noise(3, 2, RQ * 64)
    ctx, _ = folded(hip, audio, ["peaking", "notch", "peaking"], device=waa.PLAN_ONLY)
    plan = ctx.plan_describe()
    ctx.close()
    assert "folded into the impulse response" not in plan and "in the impulse response)" not in plan, plan
    assert "biquad node 2 has constant coefficients and only feeds convolver node 3: filtered by the forward transform's input stage" in plan, plan
    assert "biquad node 2: one type per instance: notch x1 peaking x2" in plan, plan


# --------------------------------------------------------------------------------------------------------------- CPU: mixed.py
def _single(binding, type_, i, device=-1, extra_gain=False, frames=FRAMES):
    """one context of the reference: BufferSource -> Biquad -> Gain -> destination"""
    ctx = waa.OfflineAudioContext(2, frames, SR, binding=binding, device=device)
    src = ctx.create_buffer_source()
    src.set_buffer(waa.AudioBuffer(white_noise(1, 2, frames, first=i)[0], SR))
    bq = ctx.create_biquad_filter(type_=type_, frequency=freq_of(i), q=q_of(i), gain=gain_of(i))
    node = src.connect(bq).connect(ctx.create_gain(gain=0.5))
    if extra_gain:
        node = node.connect(ctx.create_gain(gain=0.9))
    node.connect(ctx.destination())
    src.start()
    return ctx


def test_mixed_buckets(hip, orc):
    from web_audio_api_rs_amd.mixed import bucket_report

    def requests(binding):
        ctxs = [_single(binding, t, i, device=waa.PLAN_ONLY if binding is hip else -1) for i, t in enumerate(TYPES)]
        ctxs.append(_single(binding, "lowpass", 8, device=waa.PLAN_ONLY if binding is hip else -1, extra_gain=True))  # another graph
        return ctxs

    ctxs = requests(hip)
    assert bucket_report(ctxs) == [list(range(8)), [8]]
    for c in ctxs:
        c.close()
    ctxs = requests(orc)  # one type per batch: every type its own bucket
    assert bucket_report(ctxs) == [[i] for i in range(9)]
    for c in ctxs:
        c.close()


def test_mixed_merge_carries_the_types(hip):
    from web_audio_api_rs_amd.mixed import _merge
    ctxs = [_single(hip, t, i, device=waa.PLAN_ONLY) for i, t in enumerate(["notch", "peaking", "notch"])]
    car = _merge(ctxs)
    bq = car._nodes[2]
    assert car.n_instances == 3 and bq.per_instance and [bq.type_of(i) for i in range(3)] == ["notch", "peaking", "notch"]
    assert "biquad node 2: one type per instance: notch x2 peaking x1" in car.plan_describe()
    car.close()
    # equal types everywhere: the node stays shared
    car = _merge([_single(hip, "allpass", i, device=waa.PLAN_ONLY) for i in range(3)])
    assert not car._nodes[2].per_instance and car._nodes[2].type_ == "allpass" and NOTE not in car.plan_describe()
    car.close()


# ------------------------------------------------------------------------------------------------ CPU: the new kernel's code object
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_kernel_has_no_scratch_and_no_spills(tmp_path):
    """waa_biquad_coef_inst.hip compiled to ISA with the library's flags, read like tests/test_waveshaper_per_instance.py reads its
    kernel: nothing spilled, no scratch memory, no LDS"""
    out = str(tmp_path / "waa_biquad_coef_inst.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fgpu-flush-denormals-to-zero",
                           "--cuda-device-only", "-S", os.path.join(CSRC, "waa_biquad_coef_inst.hip"), "-o", out], stderr=subprocess.DEVNULL)
    res = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)(.*?)\.wavefront_size", open(out).read(), re.S):  # (one kernel's metadata, keys in order)
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(2)).group(1))  # noqa: E731
        res[re.search(r"\.name:\s+(\S+)", m.group(2)).group(1)] = {
            "spill": get("vgpr_spill_count"), "sgpr_spill": get("sgpr_spill_count"), "scratch": get("private_segment_fixed_size"),
            "lds": int(m.group(1))}
    assert len(res) == 1 and "biquad_coef_inst_kernel" in next(iter(res)), res
    assert next(iter(res.values())) == {"spill": 0, "sgpr_spill": 0, "scratch": 0, "lds": 0}, res


# ---------------------------------------------------------- the references of GPU test 2 (helpers: its oracle-against-model leg holds them)
A_RATE_CASES = ("sweep", "detune_a_rate")
N_SHARED = 11
_REF = {}


def shared_audio():
    """11 contexts on the three noise rows of tests/test_biquad_a_rate_types.py (the inputs its input cap was checked with)"""
    x = noise()
    return np.ascontiguousarray(x[[i % x.shape[0] for i in range(N_SHARED)]])


def shared_model(case):
    if ("model", case) not in _REF:
        x, params = shared_audio(), dict(case_params(case, "peaking")[0])  # (gain 6 dB for all: see a_rate_shared)
        out = np.stack([bm.render(t, SR, x[i], **params) for i, t in enumerate(types_of(N_SHARED))])
        assert_all_finite(out, f"model {case}")
        for i, t in enumerate(types_of(N_SHARED)):  # ... and it IS that file's model for every type
            if i < 8:
                assert np.array_equal(out[i], bm.render(t, SR, x[i], **case_params(case, t)[0])), (case, t)
        _REF["model", case] = out
    return _REF["model", case]


def shared_oracle(orc, case):
    if ("oracle", case) not in _REF:
        x, types = shared_audio(), types_of(N_SHARED)
        _REF["oracle", case] = oracle_each(orc, lambda be, idx: a_rate_shared(be, x, types, idx, case=case)[0], N_SHARED)
    return _REF["oracle", case]


def check_a_rate(name, got, want, peak_of):
    """the bounds of tests/test_biquad_a_rate_types.py: per (context, channel) RMS <= 1e-6 and max |diff| <= 2e-6 * max(1, peak(model))"""
    assert got.shape == want.shape == (N_SHARED, 2, FRAMES)
    assert_all_finite(got, name)
    bound = MAX_TOL * max(1.0, float(np.abs(peak_of).max()))
    r, m = float(rms_err(got, want).max()), float(np.abs(got.astype(np.float64) - want).max())
    print(f"{name}: RMS {r:.3e} (bound {TOL:.0e}), max |diff| {m:.3e} (bound {bound:.2e})")
    return r, m, bound


# ======================================================================================================================== GPU
# ---------------------------------------------------------------------------------------- 1. the same bits as a single-type batch
FORM_LINE = {"const": "biquad_stream in=source:2ch", "k-rate": "biquad_stream(k-rate)", "a-rate": "biquad_stream(a-rate, per-instance table)"}


@gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("form", ["const", "k-rate", "a-rate"])
@pytest.mark.parametrize("n", [11, 67])
def test_same_bits_as_a_single_type_batch(hip, n, form, reverse):
    types = types_of(n, reverse)
    audio = white_noise(n, 2, FRAMES)
    ctx, _ = chain(hip, audio, types, form=form)
    plan = ctx.plan_describe()
    assert f"one type per instance: {counts(types)}" in plan and FORM_LINE[form] in plan, plan
    got = render(ctx)
    assert_all_finite(got, "mixed types")
    for t in TYPES:
        ctx, _ = chain(hip, audio, [t] * n, form=form)
        plan = ctx.plan_describe()
        assert NOTE not in plan and FORM_LINE[form] in plan, plan
        ref = render(ctx)
        mine = [i for i in range(n) if types[i] == t]
        assert mine
        assert_words(got[mine], ref[mine], f"{form}, {n} contexts, type {t}")
        others = [i for i in range(n) if types[i] != t]
        assert (got[others].view(np.uint32) != ref[others].view(np.uint32)).any()  # (the types really differ)


# --------------------------------------------------------------------- 2. a shared a-rate automation against the model and the oracle
@gpu
@pytest.mark.parametrize("case", A_RATE_CASES)
def test_shared_a_rate_against_model_and_oracle(hip, orc, case):
    ctx, _ = a_rate_shared(hip, shared_audio(), types_of(N_SHARED), case=case)
    plan = ctx.plan_describe()
    assert "the coefficient table is per instance because of the types" in plan and "biquad_stream(a-rate, per-instance table)" in plan, plan
    got = render(ctx)
    want, ref = shared_model(case), shared_oracle(orc, case)
    assert float(np.abs(want).max()) > 1e-3
    results = [check_a_rate(f"{case}: device vs model", got, want, want), check_a_rate(f"{case}: device vs oracle", got, ref, want),
               check_a_rate(f"{case}: oracle vs model", ref, want, want)]
    for r, m, bound in results:  # (after every leg's figures have been printed)
        assert_le(r, TOL, "RMS")
        assert_le(m, bound, "max |diff|")


# ------------------------------------------------------------------------------------------- 3. every renderer that reads the rows
@gpu
@pytest.mark.parametrize("n_ch", [4, 6])
def test_wide_signals(hip, orc, n_ch):
    # bound: tests/test_gpu_parity.py::test_filters_on_wide_signals (RMS 1e-6, max |d| 2e-6)
    n, frames = 11, RQ * 50 + 9
    audio, types = white_noise(n, n_ch, frames), types_of(n)
    build = lambda be, idx=None: chain(be, audio, types, idx)[0]  # noqa: E731
    ctx = build(hip)
    plan = ctx.plan_describe()
    assert NOTE in plan and f"biquad_stream in=source:{n_ch}ch" in plan, plan
    assert_oracle(render(ctx), oracle_each(orc, build, n), f"{n_ch} channels", 1e-6, 2e-6)


@gpu
def test_exact_counts_through_the_dynamic_kernel(hip, orc):
    # bound: tests/test_dynamic_counts.py::_render (RMS 1e-6, max |d| 2e-5, both times max(1, peak))
    n, frames = 11, RQ * 40 + 50
    mono, stereo, types = white_noise(n, 1, frames, seed0=11) * 0.5, white_noise(n, 2, RQ * 20, seed0=12) * 0.5, types_of(n)

    def build(be, idx=None):
        """mono from t = 0; a stereo source joins late, per context at a sub-quantum time of its own, and ends early"""
        idx = list(range(n)) if idx is None else idx
        ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=len(idx), binding=be)
        a, b = ctx.create_buffer_source(), ctx.create_buffer_source()
        a.set_buffer_batch(np.ascontiguousarray(mono[idx]), SR)
        b.set_buffer_batch(np.ascontiguousarray(stereo[idx]), SR)
        bq = ctx.create_biquad_filter()
        give_types(be, bq, types, idx)
        set_params(bq, idx, "const")
        a.connect(bq)
        b.connect(bq)
        bq.connect(ctx.destination())
        a.start()
        for k, i in enumerate(idx):
            b.start_at(RQ * 9.5 / SR + i * 300.0 / SR, instance=k)
        return ctx

    ctx = build(hip)
    plan = ctx.plan_describe()
    assert NOTE in plan and "dynamic-count group" in plan, plan
    assert_oracle(render(ctx), oracle_each(orc, build, n), "late stereo source", 1e-6, 2e-5, scaled=True)


def echo(be, audio, types, delays, idx=None):
    """source -> Delay -> Biquad -> Gain -> back into the Delay; the filter's output and the source reach the destination"""
    idx = list(range(audio.shape[0])) if idx is None else idx
    ctx = waa.OfflineAudioContext(2, audio.shape[2], SR, n_instances=len(idx), binding=be)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(np.ascontiguousarray(audio[idx]), SR)
    delay, bq, fb = ctx.create_delay(0.4), ctx.create_biquad_filter(), ctx.create_gain()
    give_types(be, bq, types, idx)
    for k, i in enumerate(idx):
        delay.delay_time.set_value(float(delays[i]), instance=k)
        fb.gain.set_value(float((0.5, -0.7, 0.6, 0.3)[i % 4]), instance=k)
        bq.frequency.set_value(700.0 + 400.0 * i, instance=k)
        bq.q.set_value(0.7 + 0.1 * i, instance=k)
        bq.gain.set_value(3.0 - 0.5 * i, instance=k)
    src.connect(delay)
    delay.connect(bq).connect(fb).connect(delay)
    bq.connect(ctx.destination())
    src.connect(ctx.destination())
    src.start()
    return ctx


@gpu
@pytest.mark.parametrize("loop", ["echo", "comb"])
def test_filtered_feedback_loops(hip, orc, loop):
    # bound: tests/test_cycles.py::test_parity_filtered_echo_loop_from_the_lds_ring and
    # ::test_parity_short_filtered_echo_loop_from_the_lds_ring (RMS 1e-6, max |d| 4e-6, both times max(1, peak))
    n, frames = 11, RQ * 40
    audio, types = white_noise(n, 2, frames, seed0=38), types_of(n)
    if loop == "echo":  # longer than a tile: the one-launch filtered echo
        delays = (np.float64([2064 + 37.25 * i for i in range(n)]) / SR).astype(np.float32)
    else:               # shorter than a tile: a comb / plucked string
        delays = (np.float64([266 + 71.5 * i for i in range(n)]) / SR).astype(np.float32)
    build = lambda be, idx=None: echo(be, audio, types, delays, idx)  # noqa: E731
    ctx = build(hip)
    plan = ctx.plan_describe()
    assert NOTE in plan and "with the Biquad between the delayed read and the sum" in plan, plan
    assert ("shorter than a tile" in plan) == (loop == "comb"), plan
    assert_oracle(render(ctx), oracle_each(orc, build, n), loop, 1e-6, 4e-6, scaled=True)


def into_convolver(be, audio, types, irs, idx=None, length=None):
    """source -> Biquad -> ConvolverNode; irs [n_ch, taps]: one response for the batch, [n, n_ch, taps]: one per context"""
    idx = list(range(audio.shape[0])) if idx is None else idx
    ctx = waa.OfflineAudioContext(2, length or audio.shape[2], SR, n_instances=len(idx), binding=be)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(np.ascontiguousarray(audio[idx]), SR)
    bq = ctx.create_biquad_filter()
    give_types(be, bq, types, idx)
    set_params(bq, idx, "const")
    conv = ctx.create_convolver()
    if irs.ndim == 2:
        conv.set_buffer(waa.AudioBuffer(irs, SR))
    elif len(idx) == 1:
        conv.set_buffer(waa.AudioBuffer(irs[idx[0]], SR))
    else:
        conv.set_buffer_batch(np.ascontiguousarray(irs[idx]), SR)
    src.connect(bq).connect(conv).connect(ctx.destination())
    src.start()
    return ctx


@gpu
@pytest.mark.parametrize("taps", [300, 5000, 49153])
def test_in_front_of_a_convolver(hip, orc, taps):
    # bound: tests/test_gpu_parity.py::test_t1_small_multi_partition (RMS 1e-6, max |d| 2e-6) for the two sizes whose Biquad is a
    # biquad_stream launch; at 49153 taps, the size at which a Biquad with the same constants everywhere is folded into the response
    # (refused here), the forward transform's filter stage: ::test_biquad_folded_into_the_forward_transform bounds the RMS (1e-6) and
    # tests/test_convolver_per_instance.py::test_biquad_in_front_at_the_three_pass_size the max |d| of that stage (2e-6)
    n, length = 5, RQ * 96 + 11
    audio, types, ir = white_noise(n, 2, RQ * 97), types_of(n), decaying_ir(2, taps)
    build = lambda be, idx=None: into_convolver(be, audio, types, ir, idx, length)  # noqa: E731
    ctx = build(hip)
    plan = ctx.plan_describe()
    assert NOTE in plan and "in the impulse response" not in plan, plan
    assert ("filtered by the forward transform's input stage" if taps > 40000 else "biquad_stream in=source:2ch") in plan, plan
    got, ref = render(ctx), oracle_each(orc, build, n)
    assert_oracle(got, ref, f"{taps} taps", 1e-6, 2e-6)


@gpu
def test_in_front_of_per_context_responses(hip, orc):
    # bound: tests/test_convolver_per_instance.py::test_biquad_in_front_at_the_three_pass_size (RMS 1e-6, max |d| 2e-6)
    n, length = 3, RQ * 96 + 11
    audio, types = white_noise(n, 2, RQ * 97), ["highpass", "peaking", "lowshelf"]
    irs = np.stack([decaying_ir(2, 49153, seed=100 + 7 * i) for i in range(n)])
    build = lambda be, idx=None: into_convolver(be, audio, types, irs, idx, length)  # noqa: E731
    ctx = build(hip)
    plan = ctx.plan_describe()
    conv = [l for l in plan.splitlines() if l.startswith("convolver")]
    assert NOTE in plan and len(conv) == 1 and "the Biquad in front, in the forward transform" in conv[0] and "per-instance" in conv[0], plan
    assert_oracle(render(ctx), oracle_each(orc, build, n), "per-context responses", 1e-6, 2e-6)


# ------------------------------------------------------------------------------------------------------------------ 4. re-arm
@gpu
@pytest.mark.parametrize("form", ["const", "a-rate"])
def test_rearm_keeps_the_types(hip, form):
    from rearm import assert_differs, assert_same_bits, dense, other_dense, refill_from, render_again
    types = types_of(11)
    a, b2 = dense(11, 2, FRAMES), other_dense(11, 2, FRAMES)
    ctx, _ = chain(hip, a, types, form=form)
    assert NOTE in ctx.plan_describe()
    first = ctx.start_rendering_sync().data
    donor, _ = chain(hip, b2, types, form=form)  # (never applied: only its audio is taken)
    assert refill_from(ctx, donor) == 1
    again = render_again(ctx)
    ctx.close()
    donor.close()
    fresh = render(chain(hip, b2, types, form=form)[0])
    assert_all_finite(again, "re-armed render")
    assert_differs(again, first)
    assert_same_bits(again, fresh)


# ------------------------------------------------------------------------------------------------------ 5. mixed.render_contexts
@gpu
def test_render_contexts_merges_the_types(hip):
    from web_audio_api_rs_amd.mixed import bucket_report, render_contexts
    alone = [render(_single(hip, t, i)) for i, t in enumerate(TYPES)]
    ctxs = [_single(hip, t, i) for i, t in enumerate(TYPES)]
    assert bucket_report(ctxs) == [list(range(8))]
    merged = render_contexts(ctxs)
    for i, t in enumerate(TYPES):
        assert merged[i].data.shape == alone[i].shape == (1, 2, FRAMES)
        assert np.array_equal(merged[i].data, alone[i]), t
    assert not np.array_equal(alone[0], alone[1])


# ------------------------------------------------------------------------------------------------------------------ 6. sharded
@gpu
def test_render_sharded_slices_the_types_by_first(hip):
    from web_audio_api_rs_amd.sharding import render_sharded
    n, types = 11, types_of(11)
    audio = white_noise(n, 2, FRAMES, seed0=41)
    want = render(chain(hip, audio, types)[0])

    def build(n_instances, device, first=0):
        idx = list(range(first, first + n_instances))
        ctx = waa.OfflineAudioContext(2, FRAMES, SR, n_instances=n_instances, binding=hip, device=device)
        src = ctx.create_buffer_source()
        bq = ctx.create_biquad_filter()
        bq.set_type_batch([types[i] for i in idx])
        set_params(bq, idx, "const")
        src.connect(bq).connect(ctx.create_gain(gain=0.5)).connect(ctx.destination())
        src.start()
        return ctx, src

    out = np.zeros_like(want)
    info = render_sharded(build, audio, out, devices=[0], sub_batches=2, sample_rate=SR, pass_first=True)
    assert len(info["shards"]) == 2, info
    assert np.array_equal(out, want)
