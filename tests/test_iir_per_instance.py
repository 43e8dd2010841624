"""IIRFilterNode with one coefficient set per context of a batch (waa_iir_set_coefficients_instance, include/waa_hip_device.h).

CPU part: the refusals of the C ABI and of api.py, the plan lines of plan-only batches, mixed.py's merge, the registers of the
per-instance kernel forms.

GPU part (-m gpu): the reference is the oracle rendered ONE CONTEXT PER INSTANCE with that instance's coefficients (the oracle's
binding keeps one set per batch).  Bars are those of tests/test_iir.py, the arithmetic being the same: the scan kernel RMS <= 1e-6
and max |d| <= 1e-6, each times max(1, |oracle| max); the exact kernels bit for bit.  Every test first reads from plan_describe()
which kernel it is on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import signal

import web_audio_api_rs_amd as waa
from graphs import rms_err, white_noise

RQ = 128
SR = 48000.0
TILE = 2048
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-audio-api-rs_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
gpu = pytest.mark.gpu
DP = C.POINTER(C.c_double)


def _dp(a):
    return np.ascontiguousarray(a, np.float64).ctypes.data_as(DP)


def butter_sets(orders, wns):
    return [signal.butter(o, w) for o, w in zip(orders, wns)]


SCAN_SETS = butter_sets([1, 2, 4, 5, 6], [0.15, 0.3, 0.45, 0.6, 0.25])   # orders and cut-offs of GPU test 1


def graph(binding, noise, sets, shared=None, length=None, channels=2, head="source", device=-1, n_inst=None):
    """src -> [Gain] -> IIR -> destination; sets: {instance: (ff, fb)} or a list (one per instance); shared: the ALL set (default: the
    constructor takes sets[0], which every instance then overrides).  head: "source" = the source is the filter's plain input,
    "gain" = a signal (the Gain's output) is."""
    n_inst = n_inst or noise.shape[0]
    ctx = waa.OfflineAudioContext(channels, length or noise.shape[2], SR, n_instances=n_inst, binding=binding, device=device)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(noise, SR)
    if isinstance(sets, (list, tuple)):
        sets = dict(enumerate(sets))
    first = shared if shared is not None else next(iter(sets.values()))
    iir = ctx.create_iir_filter(*first)
    for i, (ff, fb) in sets.items():
        iir.set_coefficients(ff, fb, instance=i)
    node = src.connect(ctx.create_gain(gain=0.7)) if head == "gain" else src
    node.connect(iir).connect(ctx.destination())
    src.start()
    return ctx, iir


def iir_lines(ctx):
    return [l for l in ctx.plan_describe().splitlines() if l.startswith("iir_")]


def render_device(hip, noise, sets, expect, **kw):
    """render on the device after checking from the plan which kernel the node is on (`expect`: the start of its plan line)"""
    ctx, _ = graph(hip, noise, sets, **kw)
    lines = iir_lines(ctx)
    assert len(lines) == 1 and lines[0].startswith(expect) and "coef=per-instance(" in lines[0], ctx.plan_describe()
    out = ctx.start_rendering_sync().data
    ctx.close()
    return out


def oracle_each(orc, noise, per_inst_sets, **kw):
    """the oracle, one context per instance, each constructed with its own coefficients"""
    outs = []
    kw.pop("shared", None)
    for i, (ff, fb) in enumerate(per_inst_sets):
        ctx = waa.OfflineAudioContext(kw.get("channels", 2), kw.get("length") or noise.shape[2], SR, n_instances=1, binding=orc)
        src = ctx.create_buffer_source()
        src.set_buffer_batch(noise[i:i + 1], SR)
        iir = ctx.create_iir_filter(ff, fb)
        node = src.connect(ctx.create_gain(gain=0.7)) if kw.get("head") == "gain" else src
        node.connect(iir).connect(ctx.destination())
        src.start()
        outs.append(ctx.start_rendering_sync().data[0])
        ctx.close()
    return np.stack(outs)


def assert_scan_parity(got, ref, what):
    assert got.shape == ref.shape and np.isfinite(ref).all()
    scale = max(1.0, float(np.abs(ref).max()))
    r, m = rms_err(got, ref).max(), np.abs(got.astype(np.float64) - ref).max()
    print(f"{what}: worst RMS {r:.3e}, max |d| {m:.3e} (bars 1e-6 x {scale:.3g})")
    assert r <= 1e-6 * scale, (what, r)
    assert m <= 1e-6 * scale, (what, m)


def assert_bits(got, ref, what):
    assert got.shape == ref.shape
    bad = np.flatnonzero((got != ref).reshape(got.shape[0], -1).any(axis=1))
    assert np.array_equal(got, ref), f"{what}: instances {bad.tolist()} differ from the oracle"


# ----------------------------------------------------------------------------------------------------------- CPU: C ABI refusals
def _raw_batch(hip, n_inst, kind=None, frames=RQ * 8):
    """BufferSource -> IIRFilter (or `kind`) -> destination through the C ABI, plan-only"""
    nodes = (waa.api.NodeDesc * 3)()
    nodes[0].kind, nodes[1].kind, nodes[2].kind = waa.api.NODE_DESTINATION, waa.api.NODE_BUFFER_SOURCE, kind or waa.api.NODE_IIR_FILTER
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
    declared = sorted(set(re.findall(r"\b(waa_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted("waa_" + k for k in waa.api.ABI_DEVICE)
    lib = C.CDLL(waa.LIB_PATH)
    for s in declared:
        assert hasattr(lib, s), s


def test_abi_refusals(hip):
    one, two = [1.0], [1.0, -0.5]
    h = _raw_batch(hip, 3)
    try:
        f = hip.iir_set_coefficients_instance
        assert f(h, 2, 3, _dp(two), 2, _dp(two), 2) == 1 and b"instance 3 out of range" in hip.last_error()   # instance out of range
        assert f(h, 1, 0, _dp(two), 2, _dp(two), 2) == 1 and b"not of the expected kind" in hip.last_error()  # a source
        assert f(h, 7, 0, _dp(two), 2, _dp(two), 2) == 1
        # each validation error, per instance: the texts of waa_iir_set_coefficients
        assert f(h, 2, 1, _dp([1.0] * 21), 21, _dp(one), 1) == 2 and b"feedforward coefficients should have length" in hip.last_error()
        assert f(h, 2, 1, _dp(one), 0, _dp(one), 1) == 2
        assert f(h, 2, 1, _dp([0.0, 0.0]), 2, _dp(one), 1) == 3 and b"cannot be all zeros" in hip.last_error()
        assert f(h, 2, 1, _dp(one), 1, _dp([1.0] * 21), 21) == 2 and b"feedback coefficients should have length" in hip.last_error()
        assert f(h, 2, 1, _dp(one), 1, _dp([0.0, 1.0]), 2) == 3 and b"feedback first coefficient cannot be zero" in hip.last_error()
        # (a refused call leaves the node as it was: still without any set)
        st, msg = _describe(hip, h)
        assert st == 3 and "IIRFilterNode 2 has no coefficients" in msg and "instance" not in msg, msg
        # instances 0 and 2 only, no ALL set: planning names the node and the instance
        hip.check(f(h, 2, 0, _dp(two), 2, _dp(two), 2))
        hip.check(f(h, 2, 2, _dp(two), 2, _dp(one), 1))
        st, msg = _describe(hip, h)
        assert st == 3 and "InvalidStateError" in msg and "IIRFilterNode 2" in msg and "instance 1" in msg, msg
        # with an ALL set the plan stands ... and the batch is frozen
        hip.check(hip.iir_set_coefficients(h, 2, _dp(one), 1, _dp(one), 1))
        st, msg = _describe(hip, h)
        assert st == 0 and "coef=per-instance(3)" in msg, msg
        assert f(h, 2, 1, _dp(two), 2, _dp(two), 2) == 3 and b"frozen" in hip.last_error()
    finally:
        hip.batch_destroy(h)


def test_api_refusals_and_frequency_response(hip, orc):
    noise = white_noise(3, 2, RQ * 8)
    ctx, iir = graph(hip, noise, {}, shared=([1.0, 0.5], [1.0, -0.5]), device=waa.PLAN_ONLY)
    assert not iir.per_instance
    for bad, status, text in ((([1.0] * 21, [1.0]), 2, "feedforward coefficients should have length"),
                              (([0.0] * 3, [1.0]), 3, "cannot be all zeros"),
                              (([1.0], [1.0] * 21), 2, "feedback coefficients should have length"),
                              (([1.0], [0.0, 1.0]), 3, "first coefficient cannot be zero")):
        with pytest.raises(waa.WaaError, match=text) as e:
            iir.set_coefficients(*bad, instance=1)
        assert e.value.status == status
    for i in (3, -2):
        with pytest.raises(waa.WaaError, match="out of range") as e:
            iir.set_coefficients([1.0], [1.0], instance=i)
        assert e.value.status == 1
    with pytest.raises(waa.WaaError) as e:
        iir.set_coefficients_batch(np.ones((2, 2)), np.ones((2, 2)))  # (two sets for three contexts)
    assert e.value.status == 1
    assert not iir.per_instance
    b1, a1 = signal.butter(3, 0.2)
    iir.set_coefficients(b1, a1, instance=1)
    assert iir.per_instance
    hz = [100.0, 1000.0, 5000.0]
    own = waa.OfflineAudioContext(1, RQ, SR, binding=hip, device=waa.PLAN_ONLY).create_iir_filter(b1, a1).get_frequency_response(hz)
    assert np.array_equal(iir.get_frequency_response(hz, instance=1)[0], own[0])
    assert np.array_equal(iir.get_frequency_response(hz, instance=1)[1], own[1])
    assert np.array_equal(iir.get_frequency_response(hz, instance=0)[0], iir.get_frequency_response(hz)[0])
    assert not np.array_equal(iir.get_frequency_response(hz)[0], own[0])
    assert "coef=per-instance(2)" in iir_lines(ctx)[0]
    with pytest.raises(waa.WaaError) as e:  # after the plan
        iir.set_coefficients(b1, a1, instance=2)
    assert e.value.status == 3
    ctx.close()
    # the oracle keeps one set per batch: refused, never rendered with one instance's set
    ctx, iir = graph(orc, noise, [signal.butter(2, 0.2 + 0.1 * i) for i in range(3)])
    with pytest.raises(waa.WaaError) as e:
        ctx.start_rendering_sync()
    assert e.value.status == 4 and "one set per batch" in str(e.value)


# ------------------------------------------------------------------------------------------------------------- CPU: plan lines
def test_plan_lines(hip):
    noise = white_noise(6, 2, RQ * 64)
    strip = lambda text: [re.sub(r" \| timing:.*", "", l) for l in text.splitlines()]  # noqa: E731
    sets = butter_sets([2, 4, 4, 3, 2, 4], [0.2, 0.3, 0.4, 0.5, 0.2, 0.3])  # instances 4 and 5 repeat 0 and 1
    ctx, _ = graph(hip, noise, sets, device=waa.PLAN_ONLY)
    per = strip(ctx.plan_describe())
    ctx.close()
    line = [l for l in per if l.startswith("iir_")]
    assert line == ["iir_stream states=4 in=source:2ch out=final coef=per-instance(4)"], per
    # the same graph with one shared set (of the node's state count): today's line, and nothing else differs
    ctx, _ = graph(hip, noise, {}, shared=sets[1], device=waa.PLAN_ONLY)
    shared = strip(ctx.plan_describe())
    ctx.close()
    assert [l for l in shared if l.startswith("iir_")] == ["iir_stream states=4 in=source:2ch out=final"], shared
    assert [l for l in shared if not l.startswith("iir_")] == [l for l in per if not l.startswith("iir_")]
    # ALL plus overrides that repeat the ALL set: one distinct set
    ctx, _ = graph(hip, noise, {1: sets[1], 3: sets[1]}, shared=sets[1], device=waa.PLAN_ONLY)
    assert "coef=per-instance(1)" in iir_lines(ctx)[0]
    ctx.close()
    # one ill-conditioned instance among well-conditioned ones: the whole node is exact
    sets = [signal.butter(3, 0.3), signal.butter(11, 0.1), signal.butter(2, 0.4), signal.butter(3, 0.3)]
    ctx, _ = graph(hip, noise[:4], sets, device=waa.PLAN_ONLY)
    line = iir_lines(ctx)
    ctx.close()
    assert len(line) == 1 and line[0].startswith("iir_exact(row) states=11 in=signal") and line[0].endswith("coef=per-instance(3)"), line
    # ... and on its own each well-conditioned one is a scan-kernel filter
    ctx, _ = graph(hip, noise[:4], [sets[0], sets[2], sets[2], sets[3]], device=waa.PLAN_ONLY)
    assert iir_lines(ctx)[0].startswith("iir_stream states=3")
    ctx.close()


def test_plan_of_the_dynamic_and_loop_paths_accepts_per_instance_nodes(hip):
    """the quantum-by-quantum kernel reads the item's instance's block (DK_IIR): a per-instance node there is planned, not refused"""
    ctx = _dynamic_counts_graph(hip, _order3_sets(3), device=waa.PLAN_ONLY)
    _fill_dynamic(ctx, 0, 3)
    assert "dynamic-count group" in ctx.plan_describe()
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ CPU: mixed.py
def _single(binding, ff, fb, seed, device=waa.PLAN_ONLY):
    c = waa.OfflineAudioContext(2, RQ * 16, SR, binding=binding, device=device)
    s = c.create_buffer_source()
    s.set_buffer(waa.AudioBuffer(white_noise(1, 2, RQ * 16, seed0=seed)[0], SR))
    s.connect(c.create_iir_filter(ff, fb)).connect(c.destination())
    s.start()
    return c


def test_mixed_contexts_that_differ_in_coefficients_share_a_batch(hip, orc):
    from web_audio_api_rs_amd import mixed
    sets = [signal.butter(3, w) for w in (0.2, 0.3, 0.4)]
    ctxs = [_single(hip, *sets[i], seed=i) for i in range(3)]
    assert mixed.bucket_report(ctxs) == [[0, 1, 2]]
    batch = mixed._merge(ctxs)
    iir = [n for n in batch._nodes if isinstance(n, waa.api.IIRFilterNode)][0]
    assert batch.n_instances == 3 and iir.per_instance
    for i in range(3):
        assert np.array_equal(iir.get_frequency_response([1000.0], instance=i)[0],
                              _single(hip, *sets[i], seed=0)._nodes[-1].get_frequency_response([1000.0])[0])
    assert "coef=per-instance(3)" in iir_lines(batch)[0]
    batch.close()
    # equal coefficients: one batch whose node stays shared
    ctxs = [_single(hip, *sets[0], seed=i) for i in range(3)]
    assert mixed.bucket_report(ctxs) == [[0, 1, 2]]
    batch = mixed._merge(ctxs)
    iir = [n for n in batch._nodes if isinstance(n, waa.api.IIRFilterNode)][0]
    assert not iir.per_instance and iir_lines(batch) == [l for l in iir_lines(batch) if "per-instance" not in l]
    batch.close()
    # another padded length is another shape; other bindings keep the digests in the key
    assert mixed.bucket_report([_single(hip, *sets[0], seed=0), _single(hip, *signal.butter(4, 0.2), seed=1)]) == [[0], [1]]
    assert mixed.bucket_report([_single(orc, *sets[i], seed=i, device=-1) for i in range(3)]) == [[0], [1], [2]]
    assert mixed.bucket_report([_single(orc, *sets[0], seed=i, device=-1) for i in range(3)]) == [[0, 1, 2]]


def test_mixed_merges_on_the_set_each_context_renders_with(hip):
    """a single context may already hold an instance-0 set (set_coefficients(..., instance=0)): key and merge go by that set, never
    by the constructor's alone — equal constructor sets with different overrides, and unequal constructor sets with overrides"""
    from web_audio_api_rs_amd import mixed
    base, other = signal.butter(3, 0.2), signal.butter(3, 0.45)
    sets = [signal.butter(3, w) for w in (0.25, 0.3, 0.4)]
    hz = [500.0, 3000.0]

    def response_of(ff, fb):
        return _single(hip, ff, fb, seed=0)._nodes[-1].get_frequency_response(hz)[0]

    def check(ctxs, want):
        assert mixed.bucket_report(ctxs) == [[0, 1, 2]]
        batch = mixed._merge(ctxs)
        iir = [n for n in batch._nodes if isinstance(n, waa.api.IIRFilterNode)][0]
        for i, st in enumerate(want):
            assert np.array_equal(iir.get_frequency_response(hz, instance=i)[0], response_of(*st)), i
        line = iir_lines(batch)[0]
        batch.close()
        return iir, line

    def with_override(ctor, own, seed):
        c = _single(hip, *ctor, seed=seed)
        if own is not None:
            c._nodes[-1].set_coefficients(*own, instance=0)
        return c

    # the same constructor set, three different instance-0 sets
    iir, line = check([with_override(base, sets[i], i) for i in range(3)], sets)
    assert iir.per_instance and "coef=per-instance(3)" in line
    # unequal constructor sets, two of them overridden; the third renders with its constructor's
    iir, line = check([with_override(base, sets[0], 0), with_override(other, sets[1], 1), with_override(other, None, 2)], [sets[0], sets[1], other])
    assert "coef=per-instance(3)" in line
    # overrides that all equal one set: shared again, with THAT set
    iir, line = check([with_override(base, sets[2], 0), with_override(other, sets[2], 1), with_override(sets[2], None, 2)], [sets[2]] * 3)
    assert not iir.per_instance and "per-instance" not in line
    # the padded length of the effective set decides the bucket
    assert mixed.bucket_report([with_override(base, signal.butter(5, 0.3), 0), with_override(base, None, 1)]) == [[0], [1]]


# -------------------------------------------------------------------------------------------------------------- CPU: registers
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_per_instance_kernel_forms_keep_their_registers(tmp_path):
    """waa_iir_stream.hip and waa_iir_inst.hip compiled to ISA, read like tests/test_kernel_resources.py reads it.  The per-instance lane forms (every
    order: the cost rule sends any order there once a batch has more than 64 K streams) spill nothing and use no scratch memory.
    The per-instance scan forms for NS <= 8 spill no vector register and reserve not one byte of scratch memory more than the
    shared forms: those reserve 224 bytes for the copy of the source's descriptor that the slow (generic) loader indexes, whatever
    the order and since before this form existed — the coefficient and matrix offsets add nothing to it."""
    res = {}
    for src in ("waa_iir_stream.hip", "waa_iir_inst.hip"):  # the shared forms; the per-instance forms (a code object of their own)
        out = str(tmp_path / (src + ".s"))
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fgpu-flush-denormals-to-zero",
                               "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out], stderr=subprocess.DEVNULL)
        for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.wavefront_size", open(out).read(), re.S):
            get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(2)).group(1))  # noqa: E731
            res[m.group(1)] = {"vgpr": get("vgpr_count"), "spill": get("vgpr_spill_count"), "sgpr_spill": get("sgpr_spill_count"),
                               "scratch": get("private_segment_fixed_size")}
    one = lambda key: [v for n, v in res.items() if key in n]  # noqa: E731
    for ns in range(1, 20):
        k = one(f"iir_lane_kernelILi{ns}ELb1E")
        assert len(k) == 1 and k[0]["spill"] == 0 and k[0]["sgpr_spill"] == 0 and k[0]["scratch"] == 0 and k[0]["vgpr"] <= 256, (ns, k)
    for ns in range(1, 9):
        per, shared = one(f"iir_stream_kernelILi{ns}ELb1E"), one(f"iir_stream_kernelILi{ns}ELb0E")
        assert len(per) == 1 and len(shared) == 1, ns
        assert per[0]["spill"] == 0 and per[0]["vgpr"] <= 256, (ns, per)  # two wavefronts per SIMD, like the shared form
        assert per[0]["scratch"] == shared[0]["scratch"] and per[0]["sgpr_spill"] <= shared[0]["sgpr_spill"], (ns, per, shared)
    for m_ in (1, 2):
        for form in ("Lb0E", "Lb1E"):
            k = one(f"iir_row_kernelILi{m_}E{form}")
            assert len(k) == 1 and k[0]["spill"] == 0 and k[0]["scratch"] == 0, (m_, form, k)


# ------------------------------------------------------------------------------------------------------------------------ GPU
FRAMES_SCAN = TILE * 2 + 517   # two full tiles and a partial one: the state is carried


@gpu
@pytest.mark.parametrize("head", ["source", "gain"])
def test_scan_kernel_each_instance_its_own_order(hip, orc, head):
    """orders 1, 2, 4, 5, 6 in one node: differing lengths, zero padded to 6 states; once with the source as the kernel's plain
    input, once behind a Gain (a signal)"""
    noise = white_noise(5, 2, FRAMES_SCAN, seed0=31)
    got = render_device(hip, noise, SCAN_SETS, f"iir_stream states=6 in={'source' if head == 'source' else 'signal'}", head=head)
    assert_scan_parity(got, oracle_each(orc, noise, SCAN_SETS, head=head), f"scan kernel, input = {head}")


@gpu
def test_scan_kernel_no_crosstalk_between_instances(hip, orc):
    noise = np.repeat(white_noise(1, 2, FRAMES_SCAN, seed0=32), 5, axis=0)   # identical audio everywhere
    got = render_device(hip, noise, SCAN_SETS, "iir_stream states=6")
    assert_scan_parity(got, oracle_each(orc, noise, SCAN_SETS), "identical audio, five filters")
    for i in range(5):
        for j in range(i + 1, 5):
            assert np.abs(got[i] - got[j]).max() > 1e-3, (i, j)


@gpu
def test_scan_kernel_all_plus_overrides(hip, orc):
    noise = white_noise(4, 2, FRAMES_SCAN, seed0=33)
    shared, o1, o3 = signal.butter(3, 0.2), signal.butter(4, 0.5), signal.butter(1, 0.3)
    got = render_device(hip, noise, {1: o1, 3: o3}, "iir_stream states=4", shared=shared)
    assert_scan_parity(got, oracle_each(orc, noise, [shared, o1, shared, o3]), "ALL plus overrides on 1 and 3")


@gpu
@pytest.mark.parametrize("order", [1, 2])
def test_lane_kernel_is_bit_identical(hip, orc, order, monkeypatch):
    monkeypatch.setenv("WAA_IIR_EXACT", "1")
    noise = white_noise(70, 2, TILE + 300, seed0=order)  # 140 streams: more than two waves, the last one partial
    sets = [signal.butter(order, 0.1 + 0.8 * i / 70) for i in range(70)]
    got = render_device(hip, noise, sets, f"iir_exact(lane) states={order}")
    assert_bits(got, oracle_each(orc, noise, sets), f"lane kernel, order {order}")


@gpu
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("order", [5, 16, 17])
def test_row_kernel_is_bit_identical(hip, orc, order, channels, monkeypatch):
    """a wave's four rows span four (mono) or two (stereo) instances; 7 instances: the last wave is partial"""
    monkeypatch.setenv("WAA_IIR_EXACT", "1")
    noise = white_noise(7, channels, TILE + 300, seed0=order)
    sets = [signal.butter(order, 0.25 + 0.05 * i) for i in range(7)]
    got = render_device(hip, noise, sets, f"iir_exact(row) states={order}", channels=channels)
    assert_bits(got, oracle_each(orc, noise, sets, channels=channels), f"row kernel, order {order}, {channels} channel(s)")


@gpu
def test_one_ill_conditioned_instance_makes_the_node_exact(hip, orc):
    noise = white_noise(4, 2, TILE + 300, seed0=36)
    sets = [signal.butter(3, 0.3), signal.butter(11, 0.1), signal.butter(2, 0.4), signal.butter(6, 0.5)]
    got = render_device(hip, noise, sets, "iir_exact(row) states=11")
    assert_bits(got, oracle_each(orc, noise, sets), "mixed conditioning")


@gpu
def test_fir_like_and_unequal_lengths_mono_with_tail(hip, orc):
    """feedforward longer than feedback next to a plain first-order set; mono, the render longer than the source"""
    sets = [([0.2, -0.1, 0.05, 0.3, 0.1, -0.2], [2.0, -0.8]), ([0.3, 0.3], [1.0, -0.4]), ([0.5], [1.0])]
    noise = white_noise(3, 1, RQ * 9 + 11, seed0=77)
    kw = dict(length=TILE * 2 + 100, channels=1)
    got = render_device(hip, noise, sets, "iir_stream states=5 in=source:1ch", **kw)
    assert_scan_parity(got, oracle_each(orc, noise, sets, **kw), "FIR-like and first order")


def _order3_sets(n):
    return [signal.butter(3, 0.15 + 0.12 * i) for i in range(n)]


def _dynamic_counts_graph(be, sets, device=-1):
    """the graph of test_dynamic_counts.py::test_filter_starts_its_second_channel_from_zero[iir]"""
    k = len(sets)  # (one context for the oracle)
    c = waa.OfflineAudioContext(2, RQ * 90 + 50, SR, n_instances=k, binding=be, device=device)
    mono = c.create_buffer_source()
    stereo = c.create_buffer_source()
    c._test_sources = (mono, stereo)
    f = c.create_iir_filter(*sets[0])
    if k > 1:
        for i, s in enumerate(sets):
            f.set_coefficients(*s, instance=i)
    mono.connect(f)
    stereo.connect(f)
    f.connect(c.destination())
    return c


def _fill_dynamic(c, lo, hi):
    mono, stereo = c._test_sources
    frames = RQ * 90 + 50
    mono.set_buffer_batch(white_noise(3, 1, frames, seed0=11)[lo:hi] * 0.5, SR)
    stereo.set_buffer_batch(white_noise(3, 2, RQ * 30, seed0=12)[lo:hi] * 0.5, SR)
    mono.start_at(0.0)
    for i in range(lo, hi):
        stereo.start_at(RQ * 9.5 / SR + i * 300.0 / SR, instance=i - lo)


@gpu
def test_dynamic_counts_per_instance(hip, orc):
    sets = _order3_sets(3)
    c = _dynamic_counts_graph(hip, sets)
    _fill_dynamic(c, 0, 3)
    assert "dynamic-count group" in c.plan_describe()
    got = c.start_rendering_sync().data
    c.close()
    ref = []
    for i in range(3):
        c = _dynamic_counts_graph(orc, sets[i:i + 1])
        _fill_dynamic(c, i, i + 1)
        ref.append(c.start_rendering_sync().data[0])
        c.close()
    ref = np.stack(ref)
    scale = max(1.0, float(np.abs(ref).max()))
    assert rms_err(got, ref).max() <= 1e-6 * scale, rms_err(got, ref)
    assert np.abs(got - ref).max() <= 2e-5 * scale   # (the bars of test_dynamic_counts.py's _render)
    assert np.abs(ref[:, 0] - ref[:, 1]).max() > 1e-3


def _loop_graph(be, noise, sets, delay, a_rate_pan):
    n_inst, _, frames = noise.shape
    c = waa.OfflineAudioContext(2, frames, SR, n_instances=n_inst, binding=be)
    src = c.create_buffer_source()
    src.set_buffer_batch(noise * 0.5, SR)
    src.start_at(0.0)
    d = c.create_delay(0.2, delay_time=delay)
    f = c.create_iir_filter(*sets[0])
    if n_inst > 1:
        for i, s in enumerate(sets):
            f.set_coefficients(*s, instance=i)
    fb = c.create_gain(gain=0.5)
    src.connect(d)
    if a_rate_pan:
        pan = c.create_stereo_panner(pan=0.0)
        pan.pan.set_value_at_time(-1.0, 0.0).linear_ramp_to_value_at_time(1.0, frames / SR)
        d.connect(f).connect(pan).connect(fb).connect(d)
        pan.connect(c.destination())
    else:
        d.connect(f).connect(fb).connect(d)
        f.connect(c.destination())
    return c


@gpu
@pytest.mark.parametrize("delay,a_rate_pan,expect", [(0.003, True, "dynamic-count group"), (0.1, False, "iir_stream states=2")])
def test_feedback_loops_per_instance(hip, orc, delay, a_rate_pan, expect):
    """the short loop of test_dynamic_counts.py::test_loop_members_outside_the_static_loop_kernel_use_the_dynamic_path (the
    quantum-by-quantum kernel), and a loop whose delay (4800 frames) is longer than a block: the node-major IIR step"""
    frames = RQ * 90 + 50
    noise = white_noise(3, 2, frames, seed0=81)
    sets = [signal.butter(2, w) for w in (0.3, 0.15, 0.5)]
    c = _loop_graph(hip, noise, sets, delay, a_rate_pan)
    plan = c.plan_describe()
    assert expect in plan, plan
    if not a_rate_pan:
        assert "coef=per-instance(3)" in plan, plan
    got = c.start_rendering_sync().data
    c.close()
    ref = []
    for i in range(3):
        c = _loop_graph(orc, noise[i:i + 1], sets[i:i + 1], delay, a_rate_pan)
        ref.append(c.start_rendering_sync().data[0])
        c.close()
    ref = np.stack(ref)
    if not a_rate_pan:  # the scan kernel through the node-major step: the scan kernel's bars
        assert_scan_parity(got, ref, "loop with a 4800-frame delay")
        return
    scale = max(1.0, float(np.abs(ref).max()))
    assert rms_err(got, ref).max() <= 1e-6 * scale, rms_err(got, ref)
    assert np.abs(got - ref).max() <= 2e-5 * scale   # (dyn_kernel: the bars of test_dynamic_counts.py's _render)


@gpu
def test_rearm_keeps_the_coefficients(hip):
    from rearm import assert_differs, assert_same_bits, dense, other_dense, refill_from, render_again
    a, b2 = dense(5, 2, FRAMES_SCAN), other_dense(5, 2, FRAMES_SCAN)
    ctx, _ = graph(hip, a, SCAN_SETS)
    assert "coef=per-instance(5)" in iir_lines(ctx)[0]
    first = ctx.start_rendering_sync().data
    donor, _ = graph(hip, b2, SCAN_SETS)  # (never applied: only its audio is taken)
    assert refill_from(ctx, donor) == 1
    again = render_again(ctx)
    ctx.close()
    fresh = render_device(hip, b2, SCAN_SETS, "iir_stream states=6")
    assert_differs(again, first)
    assert_same_bits(again, fresh)


@gpu
def test_render_sharded_installs_each_sub_batch_its_slice(hip):
    """two sub-batches whose setup installs the sets [first, first + count): equal to the one-batch render"""
    sets = [signal.butter(1 + i % 4, 0.15 + 0.07 * i) for i in range(6)]
    noise = white_noise(6, 2, FRAMES_SCAN, seed0=41)
    want = render_device(hip, noise, sets, "iir_stream states=4")

    def build(n_instances, device, first=0):
        ctx = waa.OfflineAudioContext(2, FRAMES_SCAN, SR, n_instances=n_instances, binding=hip, device=device)
        src = ctx.create_buffer_source()
        iir = ctx.create_iir_filter(*sets[first])
        for i in range(n_instances):
            iir.set_coefficients(*sets[first + i], instance=i)
        src.connect(iir).connect(ctx.destination())
        src.start()
        return ctx, src

    out = np.zeros_like(want)
    from web_audio_api_rs_amd.sharding import render_sharded
    info = render_sharded(build, noise, out, devices=[0], sub_batches=2, sample_rate=SR, pass_first=True)
    assert len(info["shards"]) == 2, info
    assert np.array_equal(out, want)
