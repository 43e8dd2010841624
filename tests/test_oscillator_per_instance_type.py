"""OscillatorNode with one waveform TYPE per context of a batch (waa_oscillator_set_type_instance, include/waa_hip_device.h).

The criterion of the GPU tests is bit equality with single-type batches: phase construction, replay tables and the store do not
depend on the type, and the waveform function of waa_osc_types.hip is the one of waa_osc.hip (csrc/waa_osc_wave.hpp) on the same
inputs — there is no tolerance to choose.  Against tests/oscillator_model.py and the oracle the bound is the one
tests/test_oscillator_kernels.py computes for (case, type): context i of the mixed batch is context i % n_ctx of the case with
type i % 4, and is held against that context's row of expected(case, type) / oracle(case, type)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import web_audio_api_rs_amd as waa
from graphs import assert_le
from test_oscillator_kernels import PLAN_LINE, RQ, SR, case_spec, compare, custom_table, expected, oracle

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-audio-api-rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BUILT_IN = ("sine", "square", "sawtooth", "triangle")
ALL5 = BUILT_IN + ("custom",)
NOTE = "one type per instance:"


def types_of(n, k=4):
    return [ALL5[i % k] for i in range(n)]


def wave_of(i):
    """the PeriodicWave of custom context i: two distinct coefficient sets and one finished table, by i % 3"""
    if i % 3 == 2:
        return waa.PeriodicWave.from_wavetable(custom_table())
    real = np.zeros(6, np.float32)
    imag = np.asarray([0.0, 1.0, 0.5, 0.0, 0.25, 0.1] if i % 3 else [0.0, 0.3, 0.0, 1.0, 0.0, 0.2], np.float32)
    real[3] = 0.4 if i % 3 else 0.0
    return waa.PeriodicWave(real=real, imag=imag)


def a_rate_block(length, i):
    n = (length + RQ - 1) // RQ * RQ
    return (300.0 + 40.0 * i + 900.0 * np.sin(np.arange(n) * (0.002 + 0.0001 * i))).astype(np.float32).reshape(-1, RQ)


def batch(hip, types, length=640, form="par", graph="plain", plan_only=False, shared_type=None, per_instance=True):
    """n contexts with distinct frequency / detune / start / stop; types[i] 'custom' = wave_of(i).  per_instance=False: the shared
    option (all types equal).  graph: plain | post (two Gains + up-mix) | lfo (tremolo) | fm_mod (typed modulator) | fm_car"""
    n = len(types)
    kw = dict(device=waa.PLAN_ONLY) if plan_only else {}
    ctx = waa.OfflineAudioContext(2 if graph == "post" else 1, length, SR, n_instances=n, binding=hip, **kw)

    def settings(osc, base, a_rate):
        for i in range(n):
            if a_rate:
                osc.frequency.set_block(0, a_rate_block(length, i), instance=i)
            else:
                osc.frequency.set_value(base * (1.0 + 0.173 * i) * (-1.0 if i % 5 == 3 else 1.0), instance=i)
            osc.detune.set_value(7.0 * i - 30.0, instance=i)
            osc.start_at((3.37 * i + 0.25) / SR, instance=i)
            if i % 3 == 1:
                osc.stop_at((length - (17.5 * i) % (length / 2) - 3.0) / SR, instance=i)

    def typed(osc):
        if not per_instance:
            if types[0] == "custom":
                osc.set_periodic_wave(wave_of(0))
            else:
                osc.set_type(types[0])
            return osc
        if shared_type is not None:
            osc.set_type(shared_type)
        for i, t in enumerate(types):
            if t == "custom":
                osc.set_periodic_wave(wave_of(i), instance=i)
            else:
                osc.set_type(t, instance=i)
        return osc

    if graph in ("plain", "post"):
        osc = typed(ctx.create_oscillator())
        settings(osc, 220.0, form == "scan")
        head = osc
        if graph == "post":
            g1, g2 = ctx.create_gain(gain=0.5), ctx.create_gain(gain=1.0)
            for i in range(n):
                g2.gain.set_value([0.25, 1.0 + 5e-7, 5e-7][i % 3], instance=i)
            head = osc.connect(g1).connect(g2)
        head.connect(ctx.destination())
    elif graph == "lfo":  # tremolo: a typed LFO on a Gain's AudioParam, a constant source through the Gain
        lfo = typed(ctx.create_oscillator())
        settings(lfo, 5.0, False)
        depth, amp, src = ctx.create_gain(gain=0.4), ctx.create_gain(gain=0.5), ctx.create_constant_source(offset=1.0)
        lfo.connect(depth).connect(amp.gain)
        src.connect(amp).connect(ctx.destination())
        src.start()
    else:  # two-operator FM: modulator -> Gain -> carrier.frequency
        mod, car = ctx.create_oscillator(), ctx.create_oscillator(frequency=440.0)
        typed(mod if graph == "fm_mod" else car)
        (car if graph == "fm_mod" else mod).set_type("triangle" if graph == "fm_mod" else "sine")
        settings(mod, 110.0, False)
        mod.connect(ctx.create_gain(gain=150.0)).connect(car.frequency)
        car.connect(ctx.destination())
        car.start()
    return ctx


def render(ctx):
    out = ctx.start_rendering_sync().data
    ctx.close()
    return out


def osc_node(ctx):
    return next(nd for nd in ctx._nodes if isinstance(nd, waa.api.OscillatorNode))


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_entry_point_is_declared_and_exported(hip):
    text = open(os.path.join(ROOT, "include", "waa_hip_device.h")).read()
    assert re.search(r"\bwaa_oscillator_set_type_instance\s*\(", text)
    assert "waa_oscillator_set_type_instance" in open(os.path.join(ROOT, "include", "waa_hip.h")).read()
    assert "oscillator_set_type_instance" in waa.api.ABI_DEVICE
    assert hasattr(C.CDLL(waa.LIB_PATH), "waa_oscillator_set_type_instance")


def test_abi_refusals(hip):
    ctx = batch(hip, ["sine"] * 3, per_instance=False, plan_only=True)
    gain = ctx.create_gain()
    ctx.prepare()
    h, f = ctx._handle, hip.oscillator_set_type_instance
    osc_id = osc_node(ctx).id
    assert f(h, osc_id, 0, 4) == 3 and b"InvalidStateError: Custom type cannot be set manually" in hip.last_error()
    assert f(h, osc_id, 0, 5) == 1 and b"bad oscillator type" in hip.last_error()
    assert f(h, osc_id, 0, -1) == 1 and b"bad oscillator type" in hip.last_error()
    assert f(h, osc_id, 3, 1) == 1 and b"out of range" in hip.last_error()
    assert f(h, gain.id, 0, 1) == 1 and b"not of the expected kind" in hip.last_error()
    assert f(h, osc_id, 1, 2) == 0
    # instance = WAA_ALL_INSTANCES sets the shared type, as the Biquad's call does: instances with a type of their own keep it
    assert f(h, osc_id, 0xFFFFFFFF, 4) == 3 and f(h, osc_id, 0xFFFFFFFF, 7) == 1
    assert f(h, osc_id, 0xFFFFFFFF, 3) == 0
    plan = ctx.plan_describe()
    assert f"oscillator node {osc_id}: {NOTE} sawtooth x1 triangle x2 (" in plan, plan
    assert f(h, osc_id, 1, 1) == 3 and b"InvalidStateError" in hip.last_error()  # the batch is frozen
    out = np.empty(8192, np.float32)
    assert hip.oscillator_get_wavetable(h, osc_id, 1, out.ctypes.data_as(C.POINTER(C.c_float)), 8192) == 3
    assert b"has no PeriodicWave" in hip.last_error()
    ctx.close()


def test_api_refusals_and_type_of(hip, orc):
    ctx = waa.OfflineAudioContext(1, 256, SR, n_instances=4, binding=hip, device=waa.PLAN_ONLY)
    osc = ctx.create_oscillator(type_="triangle")
    for bad, status, msg in (("custom", 3, "Custom type cannot be set manually"), ("noise", 1, "bad oscillator type")):
        with pytest.raises(waa.WaaError) as e:
            osc.set_type(bad, instance=0)
        assert e.value.status == status and msg in str(e.value)
    with pytest.raises(waa.WaaError) as e:
        osc.set_type("sine", instance=4)
    assert e.value.status == 1 and "out of range" in str(e.value)
    with pytest.raises(waa.WaaError):
        osc.set_type_batch(["sine"] * 3)
    # the resolution order: 5 (shared type), 2 (own type), then with a shared wave 3 and 2, with an own wave 1
    assert [osc.type_of(i) for i in range(4)] == ["triangle"] * 4
    osc.set_type("square", instance=1)
    assert [osc.type_of(i) for i in range(4)] == ["triangle", "square", "triangle", "triangle"]
    osc.set_periodic_wave(wave_of(0))
    assert [osc.type_of(i) for i in range(4)] == ["custom", "square", "custom", "custom"]
    osc.set_periodic_wave(wave_of(1), instance=1)
    assert osc.type_of(1) == "custom"  # its own wave: the type given to it is ignored
    assert osc.set_type("sine") is osc  # the ALL form is ignored once the node is custom, as before
    assert osc.type_ == "custom"
    osc.connect(ctx.destination())
    osc.start()
    plan = ctx.plan_describe()
    assert "custom (time-parallel" in plan and NOTE not in plan  # all four resolve to custom: today's per-instance-wave plan
    with pytest.raises(waa.WaaError) as e:
        osc.set_type("sine", instance=0)
    assert e.value.status == 3
    ctx.close()
    # 4: per-instance waves, no shared one, an instance with neither a wave nor a type — today's refusal, same words
    ctx = waa.OfflineAudioContext(1, 256, SR, n_instances=3, binding=hip, device=waa.PLAN_ONLY)
    osc = ctx.create_oscillator()
    osc.set_periodic_wave(wave_of(0), instance=0)
    osc.set_type("sawtooth", instance=2)
    assert osc.type_of(0) == "custom" and osc.type_of(2) == "sawtooth"
    with pytest.raises(waa.WaaError) as e:
        osc.type_of(1)
    assert e.value.status == 3
    osc.connect(ctx.destination())
    osc.start()
    with pytest.raises(waa.WaaError) as e:
        ctx.plan_describe()
    assert e.value.status == 3 and f"OscillatorNode {osc.id} has no PeriodicWave for instance 1" in str(e.value)
    ctx.close()


def test_other_bindings_keep_one_type_per_batch(orc):
    def two(types):
        ctx = waa.OfflineAudioContext(1, 256, SR, n_instances=2, binding=orc)
        osc = ctx.create_oscillator()
        osc.set_type_batch(types)
        osc.connect(ctx.destination())
        osc.start()
        return ctx
    shared = waa.OfflineAudioContext(1, 256, SR, n_instances=2, binding=orc)
    o = shared.create_oscillator(type_="square")
    o.connect(shared.destination())
    o.start()
    assert np.array_equal(render(two(["square", "square"])), render(shared))
    ctx = two(["square", "sine"])
    with pytest.raises(waa.WaaError) as e:
        ctx.start_rendering_sync()
    assert e.value.status == 4 and "one oscillator type per instance is a feature of the device library" in str(e.value)
    assert ctx._handle is None


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("form", ["par", "k", "scan"])
@pytest.mark.parametrize("type_", ALL5)
def test_equal_types_plan_as_the_shared_option(hip, monkeypatch, type_, form, exact):
    if exact:
        monkeypatch.setenv("WAA_OSC_EXACT", "1")
    def plan(per_instance):
        types = [type_] * 3
        ctx = waa.OfflineAudioContext(1, 640, SR, n_instances=3, binding=hip, device=waa.PLAN_ONLY)
        osc = ctx.create_oscillator()
        if type_ == "custom":  # a wave per instance, and a type per instance that the waves outrank: today's all-custom plan
            for i in range(3):
                if per_instance:
                    osc.set_type("square", instance=i)
                osc.set_periodic_wave(wave_of(i), instance=i)
        else:
            if per_instance:
                osc.set_periodic_wave(wave_of(0))  # a shared wave that every instance's own type outranks
                osc.set_type_batch(types)
            else:
                osc.set_type(type_)
        if form == "scan":
            for i in range(3):
                osc.frequency.set_block(0, a_rate_block(640, i), instance=i)
        elif form == "k":
            osc.frequency.set_block(0, np.linspace(200.0, 900.0, 5).astype(np.float32))
        osc.connect(ctx.destination())
        osc.start()
        text = re.sub(r" \| timing:[^\n]*", "", ctx.plan_describe())  # (the one part of the text that is measured, not planned)
        ctx.close()
        return text

    a, b = plan(True), plan(False)
    assert a == b, (a, b)
    if type_ == "custom":
        assert NOTE not in a and "custom (" in a and "one PeriodicWave per instance" in a
    else:
        assert f"{type_} ({PLAN_LINE['exact' if exact else 'scan' if form == 'scan' else 'par']})" in a


@pytest.mark.parametrize("form,kernel", [("par", "par"), ("scan", "scan"), ("par", "exact")])
def test_mixed_plan_line(hip, monkeypatch, form, kernel):
    if kernel == "exact":
        monkeypatch.setenv("WAA_OSC_EXACT", "1")
    ctx = batch(hip, types_of(11, 5), form=form, plan_only=True)
    plan = ctx.plan_describe()
    ctx.close()
    line = f"oscillator node 1: {NOTE} sine x3 square x2 sawtooth x2 triangle x2 custom x2 ({PLAN_LINE[kernel]})"
    assert line in plan, plan
    assert "2 table row(s) for 2 instance(s)" in plan, plan
    ctx = batch(hip, types_of(11, 4), form=form, plan_only=True)
    plan = ctx.plan_describe()
    ctx.close()
    assert f"{NOTE} sine x3 square x3 sawtooth x3 triangle x2 ({PLAN_LINE[kernel]})" in plan and "table row(s)" not in plan, plan


def test_folds_are_planned_on_a_mixed_node(hip):
    for graph, marker in (("post", "renders 2 gain(s) and the up-mix 1 -> 2"), ("lfo", "LFO: launch"), ("fm_mod", "FM: launches"),
                          ("fm_car", "FM: launches")):
        ctx = batch(hip, types_of(11, 5), graph=graph, plan_only=True)
        plan = ctx.plan_describe()
        ctx.close()
        assert NOTE in plan and marker in plan, (graph, plan)


def _single(binding, type_, i, device):
    ctx = waa.OfflineAudioContext(1, 640, SR, binding=binding, device=device)
    osc = ctx.create_oscillator(frequency=200.0 + 31.0 * i) if type_ != "custom" else ctx.create_oscillator(periodic_wave=wave_of(i))
    if type_ != "custom":
        osc.set_type(type_)
    osc.connect(ctx.destination())
    osc.start_at((i + 0.5) / SR)
    return ctx


def test_mixed_buckets(hip, orc):
    from web_audio_api_rs_amd.mixed import _merge, bucket_report
    ctxs = [_single(hip, t, i, waa.PLAN_ONLY) for i, t in enumerate(ALL5)]
    assert bucket_report(ctxs) == [[0, 1, 2, 3], [4]]  # a context with a wave stays apart from the built-in ones
    car = _merge(ctxs[:4])
    assert [osc_node(car).type_of(i) for i in range(4)] == list(BUILT_IN)
    assert f"{NOTE} sine x1 square x1 sawtooth x1 triangle x1" in car.plan_describe()
    for c in (car, ctxs[4]):
        c.close()
    ctxs = [_single(orc, t, i, -1) for i, t in enumerate(BUILT_IN)]
    assert bucket_report(ctxs) == [[0], [1], [2], [3]]
    for c in ctxs:
        c.close()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    """waa_osc_types.hip compiled to ISA with the library's flags; resource counts only.  VGPR budgets: the time-parallel kernel
    (256 lanes) 64 — eight wavefronts per SIMD: the bound with its 8 KB of LDS for a node without a custom instance, more than its
    32 KB allow with one (five workgroups per CU);
    the prefix-sum passes and the serial kernel (one wavefront per workgroup) 168 — three wavefronts per SIMD, the occupancy
    DESIGN.md 3.1e states for them"""
    out = str(tmp_path / "waa_osc_types.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fgpu-flush-denormals-to-zero",
                           "--cuda-device-only", "-S", os.path.join(CSRC, "waa_osc_types.hip"), "-o", out], stderr=subprocess.DEVNULL)
    res = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)(.*?)\.wavefront_size", open(out).read(), re.S):
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(2)).group(1))  # noqa: E731
        res[re.search(r"\.name:\s+(\S+)", m.group(2)).group(1)] = dict(
            vgpr=get("vgpr_count"), spill=get("vgpr_spill_count"), sgpr_spill=get("sgpr_spill_count"),
            scratch=get("private_segment_fixed_size"), lds=int(m.group(1)))
    assert len(res) == 4, res
    for name, r in res.items():
        assert (r["spill"], r["sgpr_spill"], r["scratch"], r["lds"]) == (0, 0, 0, 0), (name, r)  # (the LDS is dynamic)
        assert r["vgpr"] <= (64 if "par_kernel" in name else 168), (name, r)


# ------------------------------------------------------------------------------------------------------------------------ GPU
def assert_same_bits_per_type(hip, types, **kw):
    """every context of the mixed batch against the same context in a batch where all contexts have its type"""
    mixed = render(batch(hip, types, **kw))
    assert np.isfinite(mixed).all()
    for t in sorted(set(types)):
        if t == "custom":  # all-custom per-instance-wave batch: the custom contexts keep their waves
            ctx = batch(hip, ["custom"] * len(types), **kw)
        else:
            ctx = batch(hip, [t] * len(types), per_instance=False, **kw)
        assert NOTE not in ctx.plan_describe()
        single = render(ctx)
        for i, ti in enumerate(types):
            if ti == t:
                assert np.array_equal(mixed[i], single[i]), (t, i, kw)
        assert np.abs(single).max() > 0.1
    return mixed


FORMS = [("par", "par", 640), ("scan", "scan", 2441), ("par", "exact", 640), ("scan", "scan", 4225), ("par", "par", 70 * RQ)]


@gpu
@pytest.mark.parametrize("n", [11, 67])
@pytest.mark.parametrize("k", [4, 5])
@pytest.mark.parametrize("form,kernel,length", FORMS)
def test_same_bits_as_single_type_batches(hip, monkeypatch, form, kernel, length, k, n):
    if kernel == "exact":
        monkeypatch.setenv("WAA_OSC_EXACT", "1")
    ctx = batch(hip, types_of(n, k), length=length, form=form, plan_only=True)
    assert f"{NOTE} sine" in ctx.plan_describe() and PLAN_LINE[kernel] in ctx.plan_describe()
    ctx.close()
    mixed = assert_same_bits_per_type(hip, types_of(n, k), length=length, form=form)
    assert not np.array_equal(mixed[0], mixed[1])


@gpu
@pytest.mark.parametrize("graph", ["post", "lfo", "fm_mod", "fm_car"])
def test_folds_same_bits(hip, graph):
    assert_same_bits_per_type(hip, types_of(11, 5), graph=graph)


MODEL_CASES = [("par", "const_sub_sample"), ("scan", "freq_a_rate"), ("exact", "const_sub_sample")]


@gpu
@pytest.mark.parametrize("kernel,case", MODEL_CASES)
def test_mixed_batch_against_model_and_oracle(hip, orc, monkeypatch, kernel, case):
    if kernel == "exact":
        monkeypatch.setenv("WAA_OSC_EXACT", "1")
    types = types_of(11)
    specs = {t: case_spec(case, t) for t in BUILT_IN}
    s0 = specs["sine"]
    ctx = waa.OfflineAudioContext(1, s0.length, SR, n_instances=11, binding=hip)
    osc = ctx.create_oscillator()
    osc.set_type_batch(types)
    for i, t in enumerate(types):
        s, c = specs[t], i % s0.n_ctx
        for name in ("frequency", "detune"):
            kind, vals = getattr(s, name)
            param = getattr(osc, name)
            if kind == "const":
                param.set_value(vals[c], instance=i)
            else:
                param.set_block(0, vals[c] if kind == "k" else vals[c].reshape(-1, RQ), instance=i)
        osc.start_at(s.start[c], instance=i)
        if s.stop[c] is not None:
            osc.stop_at(s.stop[c], instance=i)
    osc.connect(ctx.destination())
    plan = ctx.plan_describe()
    assert f"{NOTE} sine x3 square x3 sawtooth x3 triangle x2 ({PLAN_LINE[kernel]})" in plan, plan
    got = render(ctx)
    for i, t in enumerate(types):
        c = i % s0.n_ctx
        want, bound = expected(case, t)
        ref = oracle(orc, case, t)
        name = f"{case}/{kernel}: context {i} ({t}, case context {c})"
        vs_model, loud = compare(name + " vs model", got[i:i + 1], want[c:c + 1], bound[c:c + 1])
        vs_oracle, _ = compare(name + " vs oracle", got[i:i + 1], ref[c:c + 1], bound[c:c + 1], factor=2.0)
        assert loud == 0
        assert_le(vs_model, 1.0, "device vs model, |diff| / (U + L_f * dphi)")
        assert_le(vs_oracle, 1.0, "device vs oracle, |diff| / (2 * (U + L_f * dphi))")


@gpu
def test_render_contexts_merges_the_types(hip):
    from web_audio_api_rs_amd.mixed import bucket_report, render_contexts
    alone = [render(_single(hip, t, i, 0)) for i, t in enumerate(BUILT_IN)]
    ctxs = [_single(hip, t, i, 0) for i, t in enumerate(BUILT_IN)]
    assert bucket_report(ctxs) == [[0, 1, 2, 3]]
    merged = render_contexts(ctxs)
    for i, t in enumerate(BUILT_IN):
        assert np.array_equal(merged[i].data, alone[i]), t
    assert not np.array_equal(alone[0], alone[1])


@gpu
def test_wavetable_of_a_mixed_node(hip):
    ctx = batch(hip, types_of(11, 5))
    osc = osc_node(ctx)
    assert np.array_equal(osc.wavetable(4), wave_table_reference(hip, 4))
    with pytest.raises(waa.WaaError) as e:
        osc.wavetable(1)
    assert e.value.status == 3 and "has no PeriodicWave" in str(e.value)
    ctx.close()


def wave_table_reference(hip, i):
    """the table instance i of an all-custom per-instance-wave node renders with"""
    ctx = batch(hip, ["custom"] * 11)
    t = osc_node(ctx).wavetable(i)
    ctx.close()
    return t


def voice(hip, audio, types, idx=None, form="par", device=-1, fill=True):
    """BufferSource -> Gain <- (gain) Gain(0.4) <- Oscillator, -> destination: a tremolo whose LFO has types[i] in context i, so the
    output depends on the context's audio AND on its type.  idx: the contexts of `audio` / `types` this batch holds (default all).
    form par: constant LFO frequencies (time-parallel kernel, folded into the param); scan: a-rate frequencies (prefix-sum kernel)"""
    idx = list(range(audio.shape[0])) if idx is None else list(idx)
    ctx = waa.OfflineAudioContext(2, audio.shape[2], SR, n_instances=len(idx), binding=hip, device=device)
    src = ctx.create_buffer_source()
    if fill:  # (render_sharded uploads the audio itself)
        src.set_buffer_batch(np.ascontiguousarray(audio[idx]), SR)
    lfo = ctx.create_oscillator()
    mine = [types[i] for i in idx]
    if len(set(mine)) == 1 and mine[0] != "custom":
        lfo.set_type(mine[0])
    else:
        for k, i in enumerate(idx):
            if types[i] == "custom":
                lfo.set_periodic_wave(wave_of(i), instance=k)
            else:
                lfo.set_type(types[i], instance=k)
    for k, i in enumerate(idx):
        if form == "scan":
            lfo.frequency.set_block(0, a_rate_block(audio.shape[2], i), instance=k)
        else:
            lfo.frequency.set_value(150.0 + 31.0 * i, instance=k)
        lfo.detune.set_value(7.0 * i - 30.0, instance=k)
        lfo.start_at((3.37 * i + 0.25) / SR, instance=k)
    amp = ctx.create_gain(gain=0.5)
    lfo.connect(ctx.create_gain(gain=0.4)).connect(amp.gain)
    src.connect(amp).connect(ctx.destination())
    src.start()
    return ctx, src


def assert_voice_rows_equal_single_type_batches(hip, got, audio, types, form):
    for t in sorted(set(types)):
        single = render(voice(hip, audio, [t] * len(types), form=form)[0])
        for i, ti in enumerate(types):
            if ti == t:
                assert np.array_equal(got[i], single[i]), (t, i)


@gpu
@pytest.mark.parametrize("form", ["par", "scan"])
def test_rearm_keeps_the_types(hip, form):
    """A re-armed batch is frozen but for its audio (waa_hip.h: start / stop times cannot be set again), so what is new in the
    second render is the audio: it must equal a fresh mixed batch on that audio, and through it the single-type batches"""
    from rearm import assert_differs, assert_same_bits, dense, other_dense, refill_from, render_again
    types = types_of(11, 5)
    a, b2 = dense(11, 2, 640), other_dense(11, 2, 640)
    ctx, _ = voice(hip, a, types, form=form)
    assert NOTE in ctx.plan_describe()
    first = ctx.start_rendering_sync().data
    donor, _ = voice(hip, b2, types, form=form)  # (never applied: only its audio is taken)
    assert refill_from(ctx, donor) == 1
    assert NOTE in ctx.plan_describe()
    again = render_again(ctx)
    ctx.close()
    donor.close()
    fresh = render(voice(hip, b2, types, form=form)[0])
    assert np.isfinite(again).all()
    assert_differs(again, first)
    assert_same_bits(again, fresh)
    assert_voice_rows_equal_single_type_batches(hip, again, b2, types, form)
    assert not np.array_equal(render(voice(hip, b2, ["sine"] * 11, form=form)[0])[1], again[1])  # (the type is audible in the output)


@gpu
def test_render_sharded_slices_the_types_by_first(hip):
    from graphs import white_noise
    from web_audio_api_rs_amd.sharding import render_sharded
    n, types = 11, types_of(11, 5)
    audio = white_noise(n, 2, 640, seed0=43)
    want = render(voice(hip, audio, types)[0])
    assert_voice_rows_equal_single_type_batches(hip, want, audio, types, "par")

    def build(n_instances, device, first=0):
        return voice(hip, audio, types, idx=range(first, first + n_instances), device=device, fill=False)

    out = np.zeros_like(want)
    info = render_sharded(build, audio, out, devices=[0], sub_batches=2, sample_rate=SR, pass_first=True)
    assert len(info["shards"]) == 2, info
    assert np.array_equal(out, want)


@gpu
@pytest.mark.measure
@pytest.mark.parametrize("k", [4, 5])
def test_sine_table_through_the_caches_gives_the_same_bits(hip, monkeypatch, k):
    """WAA_OSC_TYPES_SINE_CACHED (measurement build; the A/B of tools/osc_types_probe.py), with and without the 32 KB of a custom row"""
    want = render(batch(hip, types_of(11, k), length=70 * RQ))
    monkeypatch.setenv("WAA_OSC_TYPES_SINE_CACHED", "1")
    assert np.array_equal(render(batch(hip, types_of(11, k), length=70 * RQ)), want)
