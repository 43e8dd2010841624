"""OscillatorNode with one PeriodicWave per context of a batch (waa_oscillator_set_periodic_wave_instance, _set_wavetable_instance,
waa_oscillator_get_wavetable: include/waa_hip_device.h), the tables of coefficient sets generated on the device
(waa_periodic_wave.hip).

CPU part: the refusals of the C ABI and of api.py, the plan note of plan-only batches (rows, instances deduplicated to rows),
mixed.py's merge, the numpy model's f32 table against its f64 table under B(1) (tests/periodic_wave_model.py, where the bound is
derived), the generator kernel's registers.

GPU part (-m gpu).  The reference is the oracle rendered ONE CONTEXT PER INSTANCE with that instance's wave (the oracle's binding
keeps one wave per batch).  Every render first reads the oscillator's kernel from plan_describe().
 * tables: wavetable(i) against table_f64 under the c = 4 bound with the node's padded n.
 * renders with finished tables per instance: per sample |device - oracle| <= U + L dphi, the bar tests/test_oscillator_kernels.py
   computes for a table waveform (U = 3 * 2^-24 * peak(table), L = 8192 * max |table[i + 1] - table[i]|, dphi = 8 * frames *
   2^-53), and exactly 0 outside an instance's start / stop times.  Both sides read the same table, so nothing is added.
 * renders with coefficient sets per instance: the same plus the instance's table bounds, c = 4 for the device's table and c = 1
   for the oracle's host-built one: linear interpolation is a convex combination of two entries, so a table error reaches the
   output at most one to one.  U and L are taken from the model's f32 table.
 * compositions: the bars of the corresponding tests of tests/test_oscillator.py plus the table bound carried through the
   composition (each test says how)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import periodic_wave_model as pm
import test_oscillator_kernels as tok
import web_audio_api_rs_amd as waa
from graphs import rms_err

RQ = 128
SR = 48000.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-audio-api-rs_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
gpu = pytest.mark.gpu
LEN = pm.LEN
PLAN_LINE = tok.PLAN_LINE


# ------------------------------------------------------------------------------------------------------------ coefficient sets
def _sets():
    rng = np.random.default_rng(0x9E71)
    j64, j257, j2048 = (np.arange(n, dtype=np.float64) for n in (64, 257, 2048))
    with np.errstate(divide="ignore"):
        saw = np.where(j64 > 0, 1.0 / j64, 0.0)
        decay257 = np.where(j257 > 0, 1.0 / j257, 0.0)
        decay2048 = np.where(j2048 > 0, 1.0 / j2048, 0.0)
    out = {
        "sine": (np.array([0.0, 0.0]), np.array([0.0, 1.0])),
        "saw64": (np.zeros(64), saw),
        "rand33": (rng.uniform(-1.0, 1.0, 33), rng.uniform(-1.0, 1.0, 33)),
        "rand257": (rng.uniform(-1.0, 1.0, 257) * decay257, rng.uniform(-1.0, 1.0, 257) * decay257),
        "decay2048": (rng.uniform(-1.0, 1.0, 2048) * decay2048, rng.uniform(-1.0, 1.0, 2048) * decay2048),
    }
    return {k: (r.astype(np.float32), i.astype(np.float32)) for k, (r, i) in out.items()}


SETS = _sets()
_F64 = {}


def f64_table(name, normalize=True):
    key = (name, normalize)
    if key not in _F64:
        t = pm.table_f64(*SETS[name], normalize=normalize)
        t.setflags(write=False)
        _F64[key] = t
    return _F64[key]


def wave(name, normalize=True):
    return waa.PeriodicWave(real=SETS[name][0], imag=SETS[name][1], disable_normalization=not normalize)


def finished_tables(k):
    """k distinct finished 8192-point tables: tok.custom_table() and variants of it (other harmonics, other noise), peak 1"""
    out = [tok.custom_table()]
    i = np.arange(LEN, dtype=np.float64) / LEN
    for m in range(1, k):
        t = np.sin(2 * np.pi * i + 0.3 * m) + 0.5 / m * np.cos(2 * np.pi * (m + 1) * i) + 0.2 * np.sin(2 * np.pi * (2 * m + 3) * i)
        t += 0.03 * np.random.default_rng(100 + m).uniform(-1.0, 1.0, LEN)
        out.append((t / np.abs(t).max()).astype(np.float32))
    return out


def osc_lines(plan):
    return [l for l in plan.splitlines() if l.startswith("oscillator node")]


def wave_note(plan, node=None):
    notes = [l for l in plan.splitlines() if "one PeriodicWave per instance" in l and (node is None or f"oscillator node {node}:" in l)]
    assert len(notes) == 1, plan
    m = re.search(r"(\d+) table row\(s\) for (\d+) instance\(s\), (\d+) generated on the device \(coefficient sets padded to (\d+)\), (\d+) uploaded", notes[0])
    assert m, notes[0]
    return tuple(int(x) for x in m.groups())  # rows, instances, generated, padded n, uploaded


# ----------------------------------------------------------------------------------------------------------- CPU: C ABI, api.py
def _fp(a):
    return np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))


def _plan_only(hip, n_inst, shared=None, frames=RQ * 8):
    ctx = waa.OfflineAudioContext(1, frames, SR, n_instances=n_inst, binding=hip, device=waa.PLAN_ONLY)
    osc = ctx.create_oscillator(**({"periodic_wave": shared} if shared is not None else {}))
    osc.connect(ctx.destination())
    osc.start()
    return ctx, osc


def test_entry_points_are_declared_and_exported(hip):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "waa_hip_device.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(waa_[a-z_0-9]+)\s*\(", text))
    lib = C.CDLL(waa.LIB_PATH)
    for s in ("waa_oscillator_set_periodic_wave_instance", "waa_oscillator_set_wavetable_instance", "waa_oscillator_get_wavetable"):
        assert s in declared and s[4:] in waa.api.ABI_DEVICE and hasattr(lib, s), s


def test_abi_refusals(hip):
    re2, im2 = [0.0, 0.5], [0.0, 1.0]
    table = tok.custom_table()
    ctx, osc = _plan_only(hip, 3)
    ctx.prepare()  # (the batch exists, nothing is planned)
    h, node = ctx._handle, osc.id
    fw, ft, get = hip.oscillator_set_periodic_wave_instance, hip.oscillator_set_wavetable_instance, hip.oscillator_get_wavetable
    out = np.empty(LEN, np.float32)
    try:
        # the shared calls' validation, per instance, in their words
        assert fw(h, node, 1, None, None, 2, 0) == 1 and b"length should at least 2" in hip.last_error()
        assert fw(h, node, 1, _fp(re2), _fp(im2), 1, 0) == 1 and b"length should at least 2" in hip.last_error()
        assert ft(h, node, 1, _fp(table), LEN - 1) == 1 and b"has 8192 points (got 8191)" in hip.last_error()
        assert ft(h, node, 1, None, LEN) == 1
        # an instance out of range, a node of another kind, no such node
        assert fw(h, node, 3, _fp(re2), _fp(im2), 2, 0) == 1 and b"instance 3 out of range" in hip.last_error()
        assert ft(h, node, 3, _fp(table), LEN) == 1 and b"instance 3 out of range" in hip.last_error()
        assert get(h, node, 3, _fp(out), LEN) == 1 and b"instance 3 out of range" in hip.last_error()
        assert get(h, node, 0, _fp(out), LEN - 1) == 1
        for f, args in ((fw, (_fp(re2), _fp(im2), 2, 0)), (ft, (_fp(table), LEN))):
            assert f(h, 0, 0, *args) == 1 and b"not of the expected kind" in hip.last_error()  # node 0 is the destination
            assert f(h, 7, 0, *args) == 1
        # (a refused call leaves the node as it was: a sine oscillator, no wave anywhere)
        assert get(h, node, 0, _fp(out), LEN) == 3 and b"has no PeriodicWave" in hip.last_error()
        # instances 0 and 2 only, no shared wave: the plan names the node and the instance
        hip.check(fw(h, node, 0, _fp(re2), None, 2, 0))
        hip.check(ft(h, node, 2, _fp(table), LEN))
        with pytest.raises(waa.WaaError, match=f"OscillatorNode {node} has no PeriodicWave for instance 1") as e:
            ctx.plan_describe()
        assert e.value.status == 3 and "InvalidStateError" in str(e.value)
        # instance = ALL is the shared call; with it the plan stands ... and the batch is frozen
        hip.check(fw(h, node, waa.api.ALL, _fp(re2), _fp(im2), 2, 0))
        assert wave_note(ctx.plan_describe()) == (3, 3, 1, 2, 2)
        for f, args in ((fw, (_fp(re2), _fp(im2), 2, 0)), (ft, (_fp(table), LEN))):
            assert f(h, node, 1, *args) == 3 and b"frozen" in hip.last_error()
            assert f(h, node, waa.api.ALL, *args) == 3 and b"frozen" in hip.last_error()
        # the tables of a plan-only batch are the host's: the finished table as it is, the shared wave's for instance 1
        hip.check(get(h, node, 2, _fp(out), LEN))
        assert np.array_equal(out, table)
    finally:
        ctx.close()


def test_api_refusals(hip, orc):
    ctx, osc = _plan_only(hip, 3)
    assert not osc.per_instance
    for i in (3, -2):
        with pytest.raises(waa.WaaError, match="out of range") as e:
            osc.set_periodic_wave(wave("sine"), instance=i)
        assert e.value.status == 1
        with pytest.raises(waa.WaaError, match="out of range") as e:
            osc.wavetable(i)
        assert e.value.status == 1
    for bad in ((np.zeros((2, 4)), None), (None, None), (np.zeros(4), None), (np.zeros((3, 4)), np.zeros((2, 4)))):
        with pytest.raises(waa.WaaError) as e:
            osc.set_periodic_wave_batch(*bad)
        assert e.value.status == 1
    with pytest.raises(waa.WaaError, match="at least 2") as e:
        osc.set_periodic_wave_batch(np.zeros((3, 1)))
    assert e.value.status == 1
    with pytest.raises(waa.WaaError, match="8192 points") as e:
        osc.set_periodic_wave(waa.PeriodicWave.from_wavetable(np.zeros(100)), instance=0)
    assert not osc.per_instance and osc.type_ == "sine"
    osc.set_periodic_wave_batch(np.zeros((3, 4)), np.tile([0.0, 1.0, 0.5, 0.25], (3, 1)))
    assert osc.per_instance and osc.type_ == "custom"
    assert wave_note(ctx.plan_describe()) == (1, 3, 1, 4, 0)
    with pytest.raises(waa.WaaError) as e:  # after the plan
        osc.set_periodic_wave(wave("sine"), instance=1)
    assert e.value.status == 3
    ctx.close()
    # the oracle keeps one wave per batch: refused, never rendered with one instance's wave
    ctx = waa.OfflineAudioContext(1, RQ * 4, SR, n_instances=2, binding=orc)
    osc = ctx.create_oscillator()
    osc.set_periodic_wave(wave("saw64"), instance=1)
    osc.connect(ctx.destination())
    osc.start()
    with pytest.raises(waa.WaaError) as e:
        ctx.start_rendering_sync()
    assert e.value.status == 4 and "one wave per batch" in str(e.value)
    with pytest.raises(waa.WaaError) as e:
        osc.wavetable(0)
    assert e.value.status == 4


def test_host_table_of_an_instance_is_the_shared_calls_table(hip):
    """before the plan, and on a plan-only batch, wavetable(i) is the host generator's table of instance i's coefficients: the
    same bits the same coefficients give as the shared wave"""
    ctx, osc = _plan_only(hip, 2, shared=wave("saw64"))
    osc.set_periodic_wave(wave("rand33", normalize=False), instance=1)
    own, shared = osc.wavetable(1), osc.wavetable(0)
    ctx.close()
    ctx, osc = _plan_only(hip, 1, shared=wave("rand33", normalize=False))
    assert np.array_equal(osc.wavetable(0), own) and not np.array_equal(own, shared)
    ctx.close()
    ctx, osc = _plan_only(hip, 1, shared=wave("saw64"))
    assert np.array_equal(osc.wavetable(0), shared)
    ctx.close()
    for name, t in (("rand33", own), ("saw64", shared)):  # ... and the host's table keeps the model's B(1) bound
        norm = name == "saw64"
        assert np.abs(t - f64_table(name, norm)).max() <= pm.bound(*SETS[name], normalize=norm, c=1)


# ------------------------------------------------------------------------------------------------------------- CPU: plan note
def test_plan_note_counts_rows_and_instances(hip):
    tables = finished_tables(2)
    ctx, osc = _plan_only(hip, 8, shared=waa.PeriodicWave.from_wavetable(tables[0]))
    osc.set_periodic_wave(wave("saw64"), instance=1)
    osc.set_periodic_wave(wave("saw64"), instance=2)                                   # bitwise equal to instance 1's: one row
    padded = np.concatenate([SETS["saw64"][1], np.zeros(10, np.float32)])
    osc.set_periodic_wave(waa.PeriodicWave(imag=padded), instance=3)                   # equal once padded: the same row
    osc.set_periodic_wave(wave("saw64", normalize=False), instance=4)                  # another flag: another row
    osc.set_periodic_wave(waa.PeriodicWave.from_wavetable(tables[1]), instance=5)
    osc.set_periodic_wave(waa.PeriodicWave.from_wavetable(tables[0].copy()), instance=6)  # the shared wave's table again: its row
    plan = ctx.plan_describe()                                                         # (instances 0 and 7: the shared wave)
    assert wave_note(plan, osc.id) == (4, 8, 2, 74, 2), plan
    assert len(osc_lines(plan)) == 2 and "custom (time-parallel, closed-form phase)" in plan
    ctx.close()
    # a node in shared mode has no such note, and its plan line is today's
    ctx, osc = _plan_only(hip, 8, shared=wave("saw64"))
    plan = ctx.plan_describe()
    assert "one PeriodicWave per instance" not in plan and len(osc_lines(plan)) == 1
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- CPU: mixed.py
def _single(binding, w, freq, device=waa.PLAN_ONLY):
    c = waa.OfflineAudioContext(1, RQ * 16, SR, binding=binding, device=device)
    o = c.create_oscillator(periodic_wave=w, frequency=freq)
    o.connect(c.destination())
    o.start()
    return c


def test_mixed_contexts_that_differ_in_their_waves_share_a_batch(hip, orc):
    from web_audio_api_rs_amd import mixed
    table = waa.PeriodicWave.from_wavetable(tok.custom_table())
    waves = [wave("saw64"), wave("rand33"), table, wave("saw64")]
    ctxs = [_single(hip, w, 100.0 * (i + 1)) for i, w in enumerate(waves)]
    assert mixed.bucket_report(ctxs) == [[0, 1, 2, 3]]
    batch = mixed._merge(ctxs)
    osc = [n for n in batch._nodes if isinstance(n, waa.api.OscillatorNode)][0]
    assert batch.n_instances == 4 and osc.per_instance and osc.periodic_wave is None
    assert wave_note(batch.plan_describe()) == (3, 4, 2, 64, 1)
    for i, w in enumerate(waves):  # each context's wave became its instance's
        alone = _single(hip, w, 100.0)
        assert np.array_equal(osc.wavetable(i), alone._nodes[-1].wavetable(0)), i
        alone.close()
    batch.close()
    # equal waves everywhere: one batch whose node stays shared
    ctxs = [_single(hip, wave("saw64"), 100.0 * (i + 1)) for i in range(3)]
    assert mixed.bucket_report(ctxs) == [[0, 1, 2]]
    batch = mixed._merge(ctxs)
    osc = [n for n in batch._nodes if isinstance(n, waa.api.OscillatorNode)][0]
    assert not osc.per_instance and "one PeriodicWave per instance" not in batch.plan_describe()
    batch.close()
    # a built-in waveform and a custom one are different shapes; other bindings keep the waves in the key
    sine = waa.OfflineAudioContext(1, RQ * 16, SR, binding=hip, device=waa.PLAN_ONLY)
    o = sine.create_oscillator(frequency=100.0)
    o.connect(sine.destination())
    o.start()
    assert mixed.bucket_report([_single(hip, wave("saw64"), 100.0), sine]) == [[0], [1]]
    assert mixed.bucket_report([_single(orc, w, 100.0, device=-1) for w in waves]) == [[0, 3], [1], [2]]


# ------------------------------------------------------------------------------------------------------------------ CPU: model
@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("normalize", [True, False])
def test_model_f32_table_is_within_b1_of_its_f64_table(name, normalize):
    eps = pm.epsilon(*SETS[name], c=4, n=2048)
    assert eps <= 1e-3, eps  # (the linearisation behind the normalised bound, with the widest c and n the tests use)
    err = float(np.abs(pm.table_f32(*SETS[name], normalize=normalize) - f64_table(name, normalize)).max())
    b = pm.bound(*SETS[name], normalize=normalize, c=1)
    print(f"{name} normalize={normalize}: err {err:.3e}, bound {b:.3e}, err / bound {err / b:.3f}, eps(c=4, n=2048) {eps:.2e}")
    assert err <= b


def test_model_all_zero_set_and_padding():
    z = np.zeros(5, np.float32)
    assert np.array_equal(pm.table_f32(z, z), np.zeros(LEN, np.float32)) and pm.bound(z, z, True, 4) == 0.0
    re_, im_ = SETS["rand33"]
    pad = np.zeros(31, np.float32)
    assert np.array_equal(pm.table_f32(re_, im_), pm.table_f32(np.concatenate([re_, pad]), np.concatenate([im_, pad])))


# -------------------------------------------------------------------------------------------------------------- CPU: registers
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_generator_kernel_uses_no_scratch_and_spills_nothing(tmp_path):
    """waa_periodic_wave.hip and waa_osc.hip compiled to ISA, read like tests/test_iir_per_instance.py reads its kernels: resource
    counts only.  The generator, and the time-parallel kernel's form with the instance's table in LDS (32 KB: five workgroups per CU)"""
    res = {}
    for src in ("waa_periodic_wave.hip", "waa_osc.hip"):
        out = str(tmp_path / (src + ".s"))
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fgpu-flush-denormals-to-zero",
                               "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out], stderr=subprocess.DEVNULL)
        for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.wavefront_size", open(out).read(), re.S):
            get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(2)).group(1))  # noqa: E731
            res[m.group(1)] = {"vgpr": get("vgpr_count"), "spill": get("vgpr_spill_count"), "sgpr_spill": get("sgpr_spill_count"),
                               "scratch": get("private_segment_fixed_size")}
    for name in ("periodic_wave_kernel", "osc_par_lds_kernel"):
        k = [v for n, v in res.items() if name in n]
        assert len(k) == 1 and k[0]["spill"] == 0 and k[0]["sgpr_spill"] == 0 and k[0]["scratch"] == 0 and k[0]["vgpr"] <= 128, (name, res)


# ------------------------------------------------------------------------------------------------------------------------ GPU
def _kernel_of(plan, node):
    line = [l for l in osc_lines(plan) if f"oscillator node {node}: custom (" in l]
    assert len(line) == 1, plan
    return line[0]


@gpu
def test_tables_generated_on_the_device(hip):
    """five coefficient sets of lengths 2, 33, 64, 257 and 2048 (the large-argument path of the range reduction; zero padding to
    2048), one un-normalised, an all-zero set, a repeated set, a finished table and an instance on the shared wave"""
    names = ["sine", "rand33", "saw64", "rand257", "decay2048"]
    norm = [True, False, True, True, True]
    finished = finished_tables(2)[1]
    n_inst = 9
    ctx = waa.OfflineAudioContext(1, RQ * 4, SR, n_instances=n_inst, binding=hip)
    osc = ctx.create_oscillator(periodic_wave=wave("saw64"))   # the shared wave: instance 8's, built on the host
    for i, (name, nm) in enumerate(zip(names, norm)):
        osc.set_periodic_wave(wave(name, nm), instance=i)
    osc.set_periodic_wave(waa.PeriodicWave(real=np.zeros(7), imag=np.zeros(7)), instance=5)
    osc.set_periodic_wave(wave("rand257"), instance=6)         # bitwise equal to instance 3's
    osc.set_periodic_wave(waa.PeriodicWave.from_wavetable(finished), instance=7)
    osc.connect(ctx.destination())
    osc.start()
    plan = ctx.plan_describe()
    assert "custom (time-parallel, closed-form phase)" in _kernel_of(plan, osc.id)
    # 6 distinct sets generated (the repeat shares its row), 2 uploaded (the finished table, the shared wave's host table)
    assert wave_note(plan, osc.id) == (8, 9, 6, 2048, 2), plan
    got = [osc.wavetable(i) for i in range(n_inst)]
    ctx.close()
    for i, (name, nm) in enumerate(zip(names, norm)):
        eps = pm.epsilon(*SETS[name], c=4, n=2048)
        b = pm.bound(*SETS[name], normalize=nm, c=4, n=2048)
        err = float(np.abs(got[i] - f64_table(name, nm)).max())
        print(f"{name} normalize={nm}: device table err {err:.3e}, bound(c=4, n=2048) {b:.3e}, err / bound {err / b:.3f}, eps {eps:.2e}")
        assert eps <= 1e-3
        assert np.isfinite(got[i]).all() and err <= b, (name, err, b)
        if nm:
            assert abs(float(np.abs(got[i]).max()) - 1.0) <= 2.0 ** -23
    assert float(np.abs(got[1]).max()) > 1.5                                   # (the un-normalised one really is)
    assert np.array_equal(got[5], np.zeros(LEN, np.float32))                   # max = 0: no scaling, a table of zeros
    assert np.array_equal(got[6].view(np.uint32), got[3].view(np.uint32))      # one row for equal sets
    assert np.array_equal(got[7].view(np.uint32), finished.view(np.uint32))    # a finished table as it is
    alone = waa.OfflineAudioContext(1, RQ * 4, SR, binding=hip)                 # the shared wave: the host table, bit for bit
    o = alone.create_oscillator(periodic_wave=wave("saw64"))
    o.connect(alone.destination())
    host = o.wavetable(0)
    alone.close()
    assert np.array_equal(got[8].view(np.uint32), host.view(np.uint32))
    assert np.abs(host - f64_table("saw64")).max() <= pm.bound(*SETS["saw64"], normalize=True, c=1)


# ---- renders: the inputs of tests/test_oscillator_kernels.py's cases, one wave per instance ---------------------------------
FORMS = {"par": ("const", "par"), "scan": ("a", "scan"), "exact_const": ("const", "exact"), "exact_a_rate": ("a", "exact")}
RENDER_CASES = [(form, n, frames) for form in FORMS for n in (3, 67) for frames in (1024, 4096 + 37)]


def render_spec(kind, n_inst, frames):
    """frequency / detune per instance from test_oscillator_kernels' case helpers, start / stop times per instance"""
    many = tok.case_spec("many_contexts", "sine")  # 67 contexts: distinct constants, both signs, sub-sample starts
    nq = (frames + RQ - 1) // RQ
    detune = ("const", many.detune[1][:n_inst])
    if kind == "const":
        freq = ("const", many.frequency[1][:n_inst])
    else:
        block = tok._freq_block(nq * RQ, 8.0)  # both signs, the changes between two frames, 8 Hz .. 4 kHz
        freq = ("a", [(block * np.float32(0.55 + 0.02 * (i % 23))).astype(np.float32) for i in range(n_inst)])
    start = [256.0 / SR] + list(many.start[1:n_inst])           # instance 0 starts on a frame, the others between two
    stop = [None if i % 3 == 0 else (0.8 * frames + 0.5 + i) / SR for i in range(n_inst)]
    return dict(n=n_inst, frames=frames, frequency=freq, detune=detune, start=start, stop=stop)


def build(binding, spec, idx, waves, shared=None, tail=None, channels=1):
    """the oscillator of contexts `idx` of a spec as one batch on `binding`; waves[i] = instance i's PeriodicWave or None (it
    uses `shared`); tail(ctx, osc): the graph behind it (default: the destination)"""
    ctx = waa.OfflineAudioContext(channels, spec["frames"], SR, n_instances=len(idx), binding=binding)
    if len(idx) == 1 and binding.prefix != "waa_":  # the oracle, one context: its wave is the context's only wave
        osc = ctx.create_oscillator(periodic_wave=waves[idx[0]] if waves[idx[0]] is not None else shared)
    else:
        osc = ctx.create_oscillator(**({"periodic_wave": shared} if shared is not None else {}))
        for k, i in enumerate(idx):
            if waves[i] is not None:
                osc.set_periodic_wave(waves[i], instance=k)
    for name in ("frequency", "detune"):
        kind, vals = spec[name]
        for k, i in enumerate(idx):
            if kind == "const":
                getattr(osc, name).set_value(vals[i], instance=k)
            else:
                getattr(osc, name).set_block(0, vals[i].reshape(-1, RQ), instance=k)
    for k, i in enumerate(idx):
        osc.start_at(spec["start"][i], instance=k)
        if spec["stop"][i] is not None:
            osc.stop_at(spec["stop"][i], instance=k)
    (tail or (lambda c, o: o.connect(c.destination())))(ctx, osc)
    return ctx, osc


def render_device(hip, spec, waves, kernel, **kw):
    ctx, osc = build(hip, spec, list(range(spec["n"])), waves, **kw)
    plan = ctx.plan_describe()
    assert f"custom ({PLAN_LINE[kernel]})" in _kernel_of(plan, osc.id), plan
    out = ctx.start_rendering_sync().data
    ctx.close()
    return out, plan


_ORACLE = {}


def oracle_each(orc, key, spec, waves, **kw):
    """the oracle, one context per instance, each with its own wave; rendered once per key"""
    if key not in _ORACLE:
        outs = []
        for i in range(spec["n"]):
            ctx, _ = build(orc, spec, [i], waves, **kw)
            outs.append(ctx.start_rendering_sync().data[0])
            ctx.close()
        out = np.stack(outs)
        out.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def table_bar(table, frames):
    """U + L dphi of tests/test_oscillator_kernels.py for a table waveform"""
    t = np.asarray(table, np.float64)
    lipschitz = LEN * float(np.abs(np.roll(t, -1) - t).max())
    return 3.0 * 2.0 ** -24 * float(np.abs(t).max()) + lipschitz * 8.0 * frames * 2.0 ** -53


def silent_mask(spec, i):
    """frames certainly outside [start, stop) of instance i (a one-frame margin around both)"""
    t = np.arange(spec["frames"]) / SR
    stop = spec["stop"][i]
    return (t < spec["start"][i] - 1.0 / SR) | ((t > stop + 1.0 / SR) if stop is not None else False)


def assert_render(what, got, ref, spec, bars):
    assert got.shape == ref.shape == (spec["n"], 1, spec["frames"]) and np.isfinite(got).all()
    worst = 0.0
    for i in range(spec["n"]):
        d = float(np.abs(got[i].astype(np.float64) - ref[i]).max())
        worst = max(worst, d / bars[i])
        assert d <= bars[i], (what, i, d, bars[i])
        quiet = silent_mask(spec, i)
        assert not got[i, 0, quiet].any() and not ref[i, 0, quiet].any(), (what, i)
        assert np.abs(ref[i, 0, ~quiet]).max() > 0.1, (what, i)  # (every instance sounds)
    print(f"{what}: worst |device - oracle| / bar = {worst:.3f}")


def _set_form(monkeypatch, form):
    kind, kernel = FORMS[form]
    if kernel == "exact":
        monkeypatch.setenv("WAA_OSC_EXACT", "1")
    return kind, kernel


@gpu
@pytest.mark.parametrize("form,n_inst,frames", RENDER_CASES)
def test_render_with_finished_tables_per_instance(hip, orc, monkeypatch, form, n_inst, frames):
    """five tables over the instances (instances that share a table differ in frequency: no crosstalk between rows), every third
    instance on the shared wave"""
    kind, kernel = _set_form(monkeypatch, form)
    spec = render_spec(kind, n_inst, frames)
    tables = finished_tables(5)
    own = [waa.PeriodicWave.from_wavetable(tables[(2 * i) % 5]) for i in range(n_inst)]
    shared = waa.PeriodicWave.from_wavetable(tables[1])
    waves = [None if i % 3 == 1 else own[i] for i in range(n_inst)]
    got, plan = render_device(hip, spec, waves, kernel, shared=shared)
    assert wave_note(plan)[:3] == (min(5, len({1 if w is None else (2 * i) % 5 for i, w in enumerate(waves)})), n_inst, 0), plan
    ref = oracle_each(orc, ("tables", kind, n_inst, frames), spec, waves, shared=shared)
    used = [tables[1] if w is None else tables[(2 * i) % 5] for i, w in enumerate(waves)]
    assert_render(f"finished tables, {form}, {n_inst} x {frames}", got, ref, spec, [table_bar(t, frames) for t in used])


COEF_NAMES = ["saw64", "rand33", "sine", "rand257"]


@gpu
@pytest.mark.parametrize("form,n_inst,frames", RENDER_CASES)
def test_render_with_coefficient_sets_per_instance(hip, orc, monkeypatch, form, n_inst, frames):
    """four coefficient sets of lengths 64, 33, 2 and 257 over the instances (padded to the longest), instance 1 un-normalised; the oracle
    builds each context's table on the host from the same coefficients"""
    kind, kernel = _set_form(monkeypatch, form)
    spec = render_spec(kind, n_inst, frames)
    names = [COEF_NAMES[i % 4] for i in range(n_inst)]
    norm = [i != 1 for i in range(n_inst)]
    waves = [wave(nm, nz) for nm, nz in zip(names, norm)]
    got, plan = render_device(hip, spec, waves, kernel)
    rows = len(set(zip(names, norm)))
    padded = max(SETS[nm][0].size for nm in names)  # (three instances: 64; 67: 257)
    assert wave_note(plan) == (rows, n_inst, rows, padded, 0), plan
    ref = oracle_each(orc, ("coefs", kind, n_inst, frames), spec, waves)
    bars = []
    for nm, nz in zip(names, norm):
        assert pm.epsilon(*SETS[nm], c=4, n=padded) <= 1e-3
        t = pm.table_f32(*SETS[nm], normalize=nz)
        bars.append(table_bar(t, frames) + pm.bound(*SETS[nm], normalize=nz, c=4, n=padded) + pm.bound(*SETS[nm], normalize=nz, c=1))
    assert_render(f"coefficient sets, {form}, {n_inst} x {frames}", got, ref, spec, bars)


# ---- compositions ------------------------------------------------------------------------------------------------------------
def _table_delta(name, normalize, n):
    """what the device's and the oracle's tables of one set may differ by, entry by entry"""
    return pm.bound(*SETS[name], normalize=normalize, c=4, n=n) + pm.bound(*SETS[name], normalize=normalize, c=1)


def _composition(binding, idx, names, frames, kind):
    """contexts `idx` of a 3-context composition whose custom oscillator has one coefficient set per context"""
    ctx = waa.OfflineAudioContext(2 if kind == "post" else 1, frames, SR, n_instances=len(idx), binding=binding)
    freq = 110.0 if kind == "fm" else 6.0 if kind == "lfo" else 220.0
    if len(idx) == 1 and binding.prefix != "waa_":
        osc = ctx.create_oscillator(frequency=freq, periodic_wave=wave(names[idx[0]]))
    else:
        osc = ctx.create_oscillator(frequency=freq)
        for k, i in enumerate(idx):
            osc.set_periodic_wave(wave(names[i]), instance=k)
    for k, i in enumerate(idx):
        osc.frequency.set_value(freq * (1.0 + 0.13 * i) * (-1.0 if kind == "fm" and i == 1 else 1.0), instance=k)
    if kind == "fm":    # custom modulator -> index -> carrier.frequency (tests/test_oscillator.py::_two_operator, custom-mod)
        car = ctx.create_oscillator(type_="sine", frequency=440.0)
        for k, i in enumerate(idx):
            car.detune.set_value(30.0 * i, instance=k)
        osc.connect(ctx.create_gain(gain=300.0)).connect(car.frequency)
        car.connect(ctx.destination())
        car.start_at(0.0005)
        osc.start()
    elif kind == "lfo":  # custom LFO -> depth -> GainNode.gain, a constant 1 through the gain: the output IS the param's value
        src = ctx.create_constant_source(offset=1.0)
        g = ctx.create_gain(gain=0.5)
        osc.connect(ctx.create_gain(gain=0.4)).connect(g.gain)
        src.connect(g).connect(ctx.destination())
        src.start()
        osc.start_at(0.0013)
    else:                # two constant gains and the up-mix 1 -> 2 (test_folded_post_ops_are_bit_identical's graph)
        g1 = ctx.create_gain(gain=0.5)
        for k, i in enumerate(idx):
            g1.gain.set_value(0.25 * (i + 1), instance=k)
        osc.connect(g1).connect(ctx.create_gain(gain=0.8)).connect(ctx.destination())
        osc.start_at(0.0013)
        osc.stop_at(0.09)
    return ctx, osc


@gpu
@pytest.mark.parametrize("kind", ["fm", "lfo", "post"])
def test_compositions(hip, orc, kind):
    names = ["saw64", "rand33", "sine"]
    frames = RQ * 60 + 37 if kind == "fm" else RQ * 37 + 11
    ctx, osc = _composition(hip, [0, 1, 2], names, frames, kind)
    plan = ctx.plan_describe()
    assert "custom (time-parallel, closed-form phase)" in _kernel_of(plan, osc.id), plan
    assert wave_note(plan, osc.id) == (3, 3, 3, 64, 0)
    fold = {"fm": "folded into the carrier's prefix-sum kernel", "lfo": "is folded into the store of the oscillator that drives it",
            "post": "renders 2 gain(s) and the up-mix 1 -> 2"}[kind]
    assert fold in plan, plan
    got = ctx.start_rendering_sync().data
    ctx.close()
    outs = []
    for i in range(3):
        c, _ = _composition(orc, [i], names, frames, kind)
        outs.append(c.start_rendering_sync().data[0])
        c.close()
    ref = np.stack(outs)
    assert np.abs(ref).max() > 0.3
    for i in range(3):
        delta = _table_delta(names[i], True, 64)
        d = float(np.abs(got[i].astype(np.float64) - ref[i]).max())
        r = float(rms_err(got[i:i + 1], ref[i:i + 1]).max())
        if kind == "fm":
            # test_parity_fm_fold's bars (2e-4 max, 2e-5 RMS).  A table error of delta is a frequency error of 300 delta Hz at most,
            # on every frame: a phase error of the carrier of at most frames * 300 delta / SR cycles, times the sine's slope 2 pi
            extra = 2.0 * np.pi * frames * 300.0 * delta / SR
            bar_max, bar_rms = 2e-4 + extra, 2e-5 + extra
        elif kind == "lfo":
            # the output is the clamped sum 0.5 + 0.4 lfo: test_folded_post_ops' RMS bar, a table oscillator's U + L dphi through the
            # depth gain for the maximum, and 0.4 delta
            extra = 0.4 * delta
            bar_rms = 1e-6 + extra
            bar_max = 0.4 * table_bar(pm.table_f32(*SETS[names[i]]), frames) + 2.0 ** -23 + extra
        else:
            # test_folded_post_ops_are_bit_identical's RMS bar; the gains' product times (U + L dphi + delta), one rounding each
            g = 0.25 * (i + 1) * 0.8
            extra = g * delta
            bar_rms = 1e-6 + extra
            bar_max = g * table_bar(pm.table_f32(*SETS[names[i]]), frames) + 2.0 ** -23 + extra
        print(f"{kind} context {i}: max |d| {d:.3e} (bar {bar_max:.3e}), RMS {r:.3e} (bar {bar_rms:.3e})")
        assert d <= bar_max and r <= bar_rms, (kind, i, d, bar_max, r, bar_rms)
    if kind == "post":
        assert np.array_equal(got[:, 0], got[:, 1])


# ---- re-arm, a second render, a shared node beside a per-instance one ---------------------------------------------------------
@gpu
def test_rearm_and_second_render_reproduce_the_first(hip):
    spec = render_spec("const", 5, 2048 + 37)
    waves = [wave(COEF_NAMES[i % 4]) for i in range(5)]
    ctx, osc = build(hip, spec, list(range(5)), waves)
    plan = ctx.plan_describe()
    assert "custom (time-parallel, closed-form phase)" in _kernel_of(plan, osc.id)
    tables = [osc.wavetable(i) for i in range(5)]

    def download():
        out = np.empty((5, 1, spec["frames"]), np.float32)
        hip.check(hip.download_all(ctx._handle, waa.api._fp(out)))
        return out

    hip.check(hip.render(ctx._handle))
    first = download()
    hip.check(hip.render(ctx._handle))            # a second render of the same batch
    second = download()
    hip.check(hip.batch_rearm(ctx._handle))
    assert ctx.plan_describe() == plan            # the plan stands: nothing is generated again
    hip.check(hip.render(ctx._handle))
    third = download()
    assert np.abs(first).max() > 0.1
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32)) and np.array_equal(first.view(np.uint32), third.view(np.uint32))
    for i in range(5):
        assert np.array_equal(osc.wavetable(i).view(np.uint32), tables[i].view(np.uint32))
    ctx.close()


@gpu
def test_shared_node_beside_a_per_instance_node_renders_what_it_renders_alone(hip):
    frames = 2048 + 37

    def graph(with_other):
        ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=3, binding=hip)
        keep = ctx.create_oscillator(frequency=330.0, periodic_wave=wave("rand33"))   # shared mode
        for i in range(3):
            keep.frequency.set_value(330.0 + 71.0 * i, instance=i)
        merger = ctx.create_channel_merger(number_of_inputs=2)
        keep.connect(merger, 0, 0)
        keep.start_at(0.0011)
        other = None
        if with_other:
            other = ctx.create_oscillator(frequency=500.0)
            for i in range(3):
                other.set_periodic_wave(wave(COEF_NAMES[i]), instance=i)
            other.connect(merger, 0, 1)
            other.start()
        merger.connect(ctx.destination())
        plan = ctx.plan_describe()
        assert "custom (time-parallel, closed-form phase)" in _kernel_of(plan, keep.id)
        assert ("one PeriodicWave per instance" in plan) == with_other
        if with_other:
            assert wave_note(plan, other.id) == (3, 3, 3, 64, 0)
        out = ctx.start_rendering_sync().data
        ctx.close()
        return out

    both, alone = graph(True), graph(False)
    assert np.abs(alone[:, 0]).max() > 0.1 and not alone[:, 1].any() and np.abs(both[:, 1]).max() > 0.1
    assert np.array_equal(both[:, 0].view(np.uint32), alone[:, 0].view(np.uint32))


@pytest.mark.measure
@gpu
@pytest.mark.parametrize("frames", [1024, 8192 * 2 + 4096 + 37])
def test_table_in_lds_and_table_in_global_memory_are_the_same_bits(hip, monkeypatch, frames):
    """the time-parallel kernel of a per-instance node stages the instance's table in LDS (osc_par_lds_kernel, 8192 frames per
    workgroup: the longer render has two full workgroups and a partial one per instance); WAA_OSC_NO_LDS_TABLE=1 reads the row from
    global memory instead (osc_par_kernel).  The arithmetic is the same"""
    spec = render_spec("const", 5, frames)
    waves = [wave(COEF_NAMES[i % 4]) for i in range(5)]
    lds, _ = render_device(hip, spec, waves, "par")
    monkeypatch.setenv("WAA_OSC_NO_LDS_TABLE", "1")
    glob, _ = render_device(hip, spec, waves, "par")
    assert np.abs(lds).max() > 0.1 and np.array_equal(lds.view(np.uint32), glob.view(np.uint32))
