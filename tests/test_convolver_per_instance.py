"""ConvolverNode with one impulse response per context of a batch (waa_node_desc.i[1] = 1; waa_conv_inst.hip).

CPU part: api.py's refusals, plan-only batches (block size, plan note, refusals of the C ABI), the mirror maps of
waa_conv_mirror.hpp against bin maps written independently in numpy, and the resources of the new kernels.

GPU part (-m gpu): the reference is the oracle rendered ONE CONTEXT PER INSTANCE with that instance's response (the oracle's
binding keeps one response per batch).  Bar: the project's convolver-vs-oracle bar (tests/test_gpu_parity.py) — RMS <= 1e-6 per
instance and channel, max |d| <= 2e-6.  Sources and normalised responses are of comparable level in every case."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import web_audio_api_rs_amd as waa
from graphs import assert_all_finite, assert_le, rms_err, t1, white_noise

RQ = 128
SR = 48000.0
FRAMES = RQ * 96 + 11
TOL_RMS, TOL_MAX = 1e-6, 2e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-audio-api-rs_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
HIPCC = "/opt/rocm/bin/hipcc"
gpu = pytest.mark.gpu


def _decaying_ir(n_ch, frames, seed=3, tau=0.3):
    rng = np.random.default_rng(seed)
    t = np.arange(frames) / max(frames, 1)
    return (rng.uniform(-1, 1, (n_ch, frames)) * np.exp(-t / tau)).astype(np.float32)


def _irs(n_inst, n_ch, frames, seed0=100):
    """[n_inst, n_ch, frames]: a different decaying-noise response per instance"""
    return np.stack([_decaying_ir(n_ch, frames, seed=seed0 + 7 * i) for i in range(n_inst)])


def per_inst(binding, noise, irs, length=None, normalize=True, with_biquad=False, device=-1, table=True):
    """src -> [Biquad] -> Convolver -> destination with context i convolving with irs[i]; table=False: irs is ONE response
    [n_ch, frames], set the shared way (i[1] = 0)"""
    n_inst = noise.shape[0]
    ctx = waa.OfflineAudioContext(2, length or noise.shape[2], SR, n_instances=n_inst, binding=binding, device=device)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(noise, SR)
    conv = ctx.create_convolver(disable_normalization=not normalize)
    if table:
        conv.set_buffer_batch(irs, SR)
    else:
        conv.set_buffer(waa.AudioBuffer(irs, SR))
    node = src
    if with_biquad:
        node = src.connect(ctx.create_biquad_filter(type_="lowpass", frequency=200.0, q=1.0))
    node.connect(conv).connect(ctx.destination())
    src.start()
    return ctx, conv


def render_device(hip, noise, irs, what, **kw):
    ctx, _ = per_inst(hip, noise, irs, **kw)
    out = ctx.start_rendering_sync().data
    ctx.close()
    assert_all_finite(out, what)
    return out


def oracle_each(orc, noise, irs, length=None, normalize=True, with_biquad=False):
    """the oracle, one context per instance, each with its own response"""
    outs = []
    for i in range(noise.shape[0]):
        ctx, _ = per_inst(orc, noise[i:i + 1], irs[i], length=length, normalize=normalize, with_biquad=with_biquad, table=False)
        outs.append(ctx.start_rendering_sync().data[0])
        ctx.close()
    return np.stack(outs)


def assert_parity(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    r = rms_err(got, ref)
    m = np.abs(got.astype(np.float64) - ref).max()
    print(f"{what}: worst RMS {r.max():.3e} (bar {TOL_RMS:.0e}), max |d| {m:.3e} (bar {TOL_MAX:.0e})")
    assert_le(r.max(), TOL_RMS, what + ": RMS per instance and channel")
    assert_le(m, TOL_MAX, what + ": max |d|")


# ----------------------------------------------------------------------------------------------------------------- CPU: api.py
def _ctx(binding, n_inst=3, frames=RQ * 8):
    ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=n_inst, binding=binding, device=waa.PLAN_ONLY)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(white_noise(n_inst, 2, frames), SR)
    conv = ctx.create_convolver()
    src.connect(conv).connect(ctx.destination())
    src.start()
    return ctx, conv


def test_api_per_instance_buffers_and_refusals(hip, orc):
    ctx, conv = _ctx(hip)
    assert not conv.per_instance
    conv.set_buffer(waa.AudioBuffer(_decaying_ir(2, 300, 1), SR))           # ALL
    assert not conv.per_instance
    conv.set_buffer(waa.AudioBuffer(_decaying_ir(2, 300, 2), SR), instance=1)  # overrides instance 1: per-instance mode
    g = ctx.graph_desc()
    assert conv.per_instance and g.nodes[conv.id].i[1] == 1
    assert any("per-instance" in l for l in ctx.plan_describe().splitlines() if l.startswith("convolver"))
    ctx.close()
    # set_buffer_batch
    ctx, conv = _ctx(hip)
    conv.set_buffer_batch(_irs(3, 2, 300), SR)
    assert conv.per_instance and "per-instance" in ctx.plan_describe()
    ctx.close()
    with pytest.raises(waa.WaaError) as e:
        _ctx(hip)[1].set_buffer_batch(_irs(2, 2, 300), SR)  # (two responses for three contexts)
    assert e.value.status == 1
    # differing channel counts
    ctx, conv = _ctx(hip)
    conv.set_buffer(waa.AudioBuffer(_decaying_ir(2, 300), SR))
    conv.set_buffer(waa.AudioBuffer(_decaying_ir(1, 300), SR), instance=2)
    with pytest.raises(waa.WaaError) as e:
        ctx.prepare()
    assert e.value.status == 4 and "channel count" in str(e.value) and "instance 2" in str(e.value)
    # differing lengths
    ctx, conv = _ctx(hip)
    conv.set_buffer(waa.AudioBuffer(_decaying_ir(2, 300), SR))
    conv.set_buffer(waa.AudioBuffer(_decaying_ir(2, 301), SR), instance=0)
    with pytest.raises(waa.WaaError) as e:
        ctx.prepare()
    assert e.value.status == 4 and "length" in str(e.value)
    # an instance without any buffer
    ctx, conv = _ctx(hip)
    conv.set_buffer(waa.AudioBuffer(_decaying_ir(2, 300), SR), instance=0)
    conv.set_buffer(waa.AudioBuffer(_decaying_ir(2, 300), SR), instance=2)
    with pytest.raises(waa.WaaError) as e:
        ctx.prepare()
    assert e.value.status == 4 and "instance 1" in str(e.value)
    # the oracle keeps one response per batch: refused, not rendered with instance 0's response
    ctx = waa.OfflineAudioContext(2, RQ * 8, SR, n_instances=3, binding=orc)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(white_noise(3, 2, RQ * 8), SR)
    conv = ctx.create_convolver()
    conv.set_buffer_batch(_irs(3, 2, 300), SR)
    src.connect(conv).connect(ctx.destination())
    src.start()
    with pytest.raises(waa.WaaError) as e:
        ctx.start_rendering_sync()
    assert e.value.status == 4 and "one response per batch" in str(e.value)


# ------------------------------------------------------------------------------------------------ CPU: plan-only batches (C ABI)
def _conv_lines(ctx):
    lines = [l for l in ctx.plan_describe().splitlines() if l.startswith("convolver")]
    ctx.close()
    return lines


def test_plan_note_and_block_size_follow_the_longest_trimmed_response(hip):
    noise = white_noise(2, 2, FRAMES)
    # instance 0 padded with zeros behind tap 100, instance 1 full length: the longest trim (20000) decides
    irs = _irs(2, 2, 20000)
    irs[0, :, 100:] = 0.0
    irs[0, :, 99] = irs[1, :, 89] = 0.5   # (taps that survive the 1e-6 trim whatever the noise drew there)
    irs[1, :, -1] = 0.05
    conv = _conv_lines(per_inst(hip, noise, irs, device=waa.PLAN_ONLY)[0])
    assert len(conv) == 1 and "per-instance" in conv[0] and "fft B=2048 N=4096 P=10" in conv[0] and "ir_len=20000" in conv[0], conv
    # every instance short: the direct FIR, with the longest of them
    irs[1, :, 90:] = 0.0
    conv = _conv_lines(per_inst(hip, noise, irs, device=waa.PLAN_ONLY)[0])
    assert len(conv) == 1 and "per-instance" in conv[0] and "direct FIR taps=100" in conv[0], conv
    # all instances all-zero: the existing zero fill
    conv = _conv_lines(per_inst(hip, noise, np.zeros((2, 2, 500), np.float32), device=waa.PLAN_ONLY)[0])
    assert len(conv) == 1 and conv[0].endswith("all-zero impulse response -> zero fill"), conv
    # one all-zero instance among others: planned like the others, its output cleared behind the inverse transform
    irs = _irs(2, 2, 3000)
    irs[1] = 0.0
    conv = _conv_lines(per_inst(hip, noise, irs, device=waa.PLAN_ONLY)[0])
    assert "fft B=128 N=256 P=24" in conv[0] and "per-instance" in conv[0] and "2 output channel(s)" in conv[1], conv


def test_shared_mode_plans_are_described_as_before(hip):
    """i[1] = 0: the same graph through the shared call and through the table form with one response everywhere — the first is
    today's plan text; the second differs from it in the convolver's lines only (and says per-instance there)"""
    noise = white_noise(3, 2, FRAMES)
    for n_taps in (60, 3000, 49153):
        ir = _decaying_ir(2, n_taps)
        strip = lambda text: [re.sub(r" \| timing:.*", "", l) for l in text.splitlines()]  # noqa: E731 (the timing of the plan itself)
        ctx_a, _ = t1(hip, noise, ir, with_biquad=False, device=waa.PLAN_ONLY)
        ctx_b, conv_b = per_inst(hip, noise, ir, table=False, device=waa.PLAN_ONLY)
        a, bb = strip(ctx_a.plan_describe()), strip(ctx_b.plan_describe())
        g = ctx_b.graph_desc()
        assert g.nodes[conv_b.id].i[1] == 0
        ctx_a.close()
        ctx_b.close()
        assert a == bb and not any("per-instance" in l for l in a), (a, bb)
        ctx_c, _ = per_inst(hip, noise, np.broadcast_to(ir, (3,) + ir.shape), device=waa.PLAN_ONLY)
        c = strip(ctx_c.plan_describe())
        ctx_c.close()
        assert [l for l in c if not l.startswith("convolver")] == [l for l in a if not l.startswith("convolver")]
        ca, cc = [l for l in a if l.startswith("convolver")], [l for l in c if l.startswith("convolver")]
        assert len(ca) == len(cc) == 1 and cc[0] == ca[0] + " per-instance impulse responses", (ca, cc)


def _raw_batch(hip, n_inst, i1, frames=RQ * 8):
    """BufferSource -> Convolver(i[1] = i1) -> destination through the C ABI, plan-only"""
    nodes = (waa.api.NodeDesc * 3)()
    nodes[0].kind, nodes[1].kind, nodes[2].kind = waa.api.NODE_DESTINATION, waa.api.NODE_BUFFER_SOURCE, waa.api.NODE_CONVOLVER
    nodes[2].i[1] = i1
    edges = (waa.api.EdgeDesc * 2)()
    edges[0].from_, edges[0].to = 1, 2
    edges[1].from_, edges[1].to = 2, 0
    g = waa.api.GraphDesc(3, nodes, 2, edges)
    h = C.c_void_p()
    hip.check(hip.batch_create(C.byref(g), n_inst, 2, frames, SR, waa.PLAN_ONLY, C.byref(h)))
    return h


def test_abi_refusals(hip):
    FP = C.POINTER(C.c_float)
    n_inst, taps = 3, 200
    irs = _irs(n_inst, 2, taps)
    h = _raw_batch(hip, n_inst, 1)
    try:
        table = (FP * (n_inst * 2))()
        for i in range(n_inst):
            for c in range(2):
                table[i * 2 + c] = irs[i, c].ctypes.data_as(FP)
        table[2 * 2 + 1] = None  # instance 2, channel 1
        with pytest.raises(waa.WaaError) as e:
            hip.check(hip.convolver_set_buffer(h, 2, table, 2, taps, SR))
        assert e.value.status == 1 and "instance 2" in str(e.value) and "channel 1" in str(e.value), str(e.value)
        table[2 * 2 + 1] = irs[2, 1].ctypes.data_as(FP)
        with pytest.raises(waa.WaaError) as e:
            hip.check(hip.convolver_set_buffer(h, 2, table, 3, taps, SR))
        assert e.value.status == 2 and "1, 2 or 4 channels" in str(e.value)
        with pytest.raises(waa.WaaError) as e:
            hip.check(hip.convolver_set_buffer(h, 2, table, 2, taps, 44100.0))
        assert e.value.status == 2 and "sample rate" in str(e.value)
        pcm = np.zeros((taps, 2), np.int16)
        with pytest.raises(waa.WaaError) as e:
            hip.check(hip.convolver_set_buffer_pcm16(h, 2, pcm.ctypes.data_as(C.POINTER(C.c_int16)), 2, taps, SR))
        assert e.value.status == 4 and "per instance" in str(e.value)
        hip.check(hip.convolver_set_buffer(h, 2, table, 2, taps, SR))
    finally:
        hip.batch_destroy(h)
    with pytest.raises(waa.WaaError) as e:
        _raw_batch(hip, n_inst, 2)
    assert e.value.status == 1


def test_per_instance_mode_without_a_buffer_passes_through(hip):
    h = _raw_batch(hip, 2, 1)
    try:
        need = C.c_size_t()
        hip.check(hip.plan_describe(h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value + 1)
        hip.check(hip.plan_describe(h, buf, need.value + 1, None))
        assert not any(l.startswith("convolver") for l in buf.value.decode().splitlines())
    finally:
        hip.batch_destroy(h)


def test_refused_in_a_delay_loop_and_in_a_dynamic_count_plan(hip):
    n_inst, frames = 2, RQ * 40
    # a convolver inside a Delay loop
    ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=n_inst, binding=hip, device=waa.PLAN_ONLY)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(white_noise(n_inst, 2, frames), SR)
    mix = ctx.create_gain(gain=1.0)
    conv = ctx.create_convolver()
    conv.set_buffer_batch(_irs(n_inst, 2, 100), SR)
    dly = ctx.create_delay(max_delay_time=1.0, delay_time=0.5)
    fb = ctx.create_gain(gain=0.3)
    src.connect(mix).connect(conv).connect(dly).connect(fb).connect(mix)
    conv.connect(ctx.destination())
    src.start()
    with pytest.raises(waa.WaaError) as e:
        ctx.plan_describe()
    assert e.value.status == 4 and f"ConvolverNode {conv.id}" in str(e.value) and "feedback loop" in str(e.value), str(e.value)
    # the (2, 1) routing with a source that ends early: a dynamic-count plan
    noise = white_noise(n_inst, 2, RQ * 25)
    ctx, conv = per_inst(hip, noise, _irs(n_inst, 1, 1500), length=frames, device=waa.PLAN_ONLY)
    with pytest.raises(waa.WaaError) as e:
        ctx.plan_describe()
    assert e.value.status == 4 and f"ConvolverNode {conv.id}" in str(e.value) and "per-quantum channel" in str(e.value), str(e.value)
    # (the same graph with one shared response is such a plan, and is rendered)
    ctx, _ = per_inst(hip, noise, _decaying_ir(1, 1500), length=frames, device=waa.PLAN_ONLY, table=False)
    assert "dynamic-count group" in ctx.plan_describe()
    ctx.close()


# ----------------------------------------------------------------------------------------------------------- CPU: the mirror maps
def _bins(order, n):
    """bin held by position p, written here from the transforms' definitions (not from the header)"""
    p = np.arange(n, dtype=np.int64)
    if order == 0:  # radix-4 DIF with (0, 2, 1, 3) slots = radix-2 DIF: bit reversal
        bits = n.bit_length() - 1
        out = np.zeros(n, np.int64)
        for b in range(bits):
            out |= ((p >> b) & 1) << (bits - 1 - b)
        return out
    k3, k1, k2 = p // 1024, (p // 32) % 32, p % 32  # waa_fft3.hpp: position k3 * 1024 + k1 * 32 + k2
    return k1 + 32 * k2 + 1024 * k3


@pytest.fixture(scope="module")
def mirror_tool(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++")
    out = tmp_path_factory.mktemp("mirror") / "conv_mirror_table"
    subprocess.check_call([CLANG, "-O2", "-std=c++17", os.path.join(ROOT, "tools", "conv_mirror_table.cpp"), "-o", str(out)])
    return str(out)


@pytest.mark.parametrize("order,n", [(0, 256), (0, 1024), (0, 4096), (0, 16384), (1, 16384)])
def test_mirror_maps(mirror_tool, order, n):
    table = np.array(subprocess.check_output([mirror_tool, str(order), str(n.bit_length() - 1)]).split(), np.int64).reshape(-1, 2)
    assert np.array_equal(table[:, 0], np.arange(n))
    mir = table[:, 1]
    assert mir.min() >= 0 and mir.max() < n
    assert np.array_equal(mir[mir], np.arange(n)), "not an involution"
    bins = _bins(order, n)
    assert sorted(bins) == list(range(n))
    assert np.array_equal(bins[mir], (n - bins) % n)
    fixed = np.flatnonzero(mir == np.arange(n))
    assert sorted(bins[fixed]) == [0, n // 2]


# ------------------------------------------------------------------------------------------------ CPU: resources of the new kernels
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_per_instance_kernels_fit_their_register_budgets(tmp_path):
    """waa_conv_inst.hip compiled to ISA: no product instantiation spills or touches scratch memory.  Register ceilings read off the
    build (gfx950, 512 registers per SIMD lane): the window form for P <= 12 needs 152 — three wavefronts per SIMD (<= 168); for
    P <= 16 (192) and P <= 24 (228) two wavefronts per SIMD (<= 256), the floor the kernel was sized for: both response columns
    and both windows stay in registers; the general form (4-channel responses, P <= 8) needs 122 — four wavefronts (<= 128)."""
    out = str(tmp_path / "waa_conv_inst.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fgpu-flush-denormals-to-zero",
                           "--cuda-device-only", "-S", os.path.join(CSRC, "waa_conv_inst.hip"), "-o", out], stderr=subprocess.DEVNULL)
    res = {}
    # (one metadata block per kernel, keys in alphabetical order: .agpr_count opens it, .wavefront_size closes it)
    for m in re.finditer(r"- \.agpr_count:\s+(\d+)(.*?)\.wavefront_size", open(out).read(), re.S):
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(2)).group(1))  # noqa: E731
        name = re.search(r"\.name:\s+(\S+)", m.group(2)).group(1)
        res[name] = dict(vgpr=get("vgpr_count"), agpr=int(m.group(1)), spill=get("vgpr_spill_count"), scratch=get("private_segment_fixed_size"))
    ceilings = {"conv_inst_win_kernelILi8ELi12E": 168, "conv_inst_win_kernelILi8ELi16E": 256, "conv_inst_win_kernelILi4ELi24E": 256,
                "conv_inst_mac_kernelILi16ELi8E": 128, "conv_inst_direct_kernel": 128}
    for key, ceiling in ceilings.items():
        k = [v for n, v in res.items() if key in n]
        assert len(k) == 1, (key, sorted(res))
        assert k[0]["spill"] == 0 and k[0]["scratch"] == 0 and k[0]["vgpr"] + k[0]["agpr"] <= ceiling, (key, k[0], ceiling)
    assert len(res) == len(ceilings), sorted(res)


# ------------------------------------------------------------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("ir_len,n_inst", [
    (1, 3), (128, 3),            # direct FIR
    (129, 2),                    # B = 128
    (3073, 5),                   # B = 512, P = 7
    (12289, 3),                  # B = 2048, P = 7
    (20000, 4),                  # B = 2048, P = 10: the window form
    (49153, 3),                  # the three-pass transforms, P = 7
    (70000, 2),                  # the three-pass transforms, P = 9: the window form
    (1900, 3), (2900, 2),        # B = 128, P = 15 and P = 23: the window form's other two instantiations
])
def test_every_path_odd_and_even_batches(hip, orc, ir_len, n_inst):
    noise = white_noise(n_inst, 2, FRAMES)
    irs = _irs(n_inst, 2, ir_len)
    got = render_device(hip, noise, irs, f"ir_len {ir_len}")
    assert_parity(got, oracle_each(orc, noise, irs), f"ir_len {ir_len}, {n_inst} instances")


@gpu
@pytest.mark.parametrize("in_ch,ir_ch", [(1, 1), (1, 2), (2, 2), (2, 4), (1, 4), (2, 1)])
def test_routing(hip, orc, in_ch, ir_ch):
    """convolver.rs:384-466; the source runs the whole render, so the plan stays static; normalisation on"""
    noise = white_noise(4, in_ch, FRAMES)
    irs = _irs(4, ir_ch, 1500, seed0=in_ch * 10 + ir_ch)
    got = render_device(hip, noise, irs, f"routing ({in_ch}, {ir_ch})")
    assert_parity(got, oracle_each(orc, noise, irs), f"routing ({in_ch}, {ir_ch})")


@gpu
def test_normalisation_is_per_instance(hip, orc):
    noise = white_noise(4, 2, FRAMES)
    irs = _irs(4, 2, 1500) * np.array([1.0, 0.01, 30.0, 1.0], np.float32)[:, None, None]
    got = render_device(hip, noise, irs, "scaled responses")
    assert_parity(got, oracle_each(orc, noise, irs), "responses scaled 1, 0.01, 30, 1")
    # identical raw responses scaled 1 and 30, equal sources: the normalisation takes the scale out again
    same = np.repeat(white_noise(1, 2, FRAMES), 2, axis=0)
    ir = _decaying_ir(2, 1500, seed=5)
    got = render_device(hip, same, np.stack([ir, ir * np.float32(30.0)]), "one response scaled 1 and 30")
    d = np.abs(got[0].astype(np.float64) - got[1]).max()
    print(f"scale 1 against scale 30: max |d| {d:.3e}")
    assert_le(d, 2e-6, "scale 1 against scale 30")
    assert np.abs(got[0]).max() > 1e-2


@gpu
def test_per_instance_trims(hip, orc):
    noise = white_noise(4, 2, FRAMES)
    irs = _irs(4, 2, 20000)
    irs[1, :, 200:] = 0.0
    irs[2] = 0.0
    irs[3, 1] = 0.0
    got = render_device(hip, noise, irs, "trims")
    assert_parity(got, oracle_each(orc, noise, irs), "per-instance trims")
    assert not got[2].any(), "an all-zero response must give exact zeros"
    assert not got[3, 1].any() and np.abs(got[3, 0]).max() > 1e-2


@gpu
def test_no_crosstalk_inside_a_pair(hip, orc):
    irs = _irs(2, 2, 12289)
    for silent in (1, 0):
        noise = white_noise(2, 2, FRAMES)
        noise[silent] = 0.0
        got = render_device(hip, noise, irs, f"instance {silent} silent")
        loud = 1 - silent
        ref = oracle_each(orc, noise[loud:loud + 1], irs[loud:loud + 1])
        assert_parity(got[loud:loud + 1], ref, f"instance {loud} next to a silent partner")
        quiet = np.sqrt(np.mean(got[silent].astype(np.float64) ** 2, axis=-1)).max()
        print(f"silent instance {silent}: RMS {quiet:.3e}")
        assert_le(quiet, TOL_RMS, f"silent instance {silent}")


@gpu
@pytest.mark.parametrize("ir_len", [20000, 49153])
def test_one_response_everywhere_agrees_with_shared_mode(hip, ir_len):
    noise = white_noise(5, 2, FRAMES)
    ir = _decaying_ir(2, ir_len)
    shared = render_device(hip, noise, ir, "shared", table=False)
    each = render_device(hip, noise, np.broadcast_to(ir, (5,) + ir.shape), "per-instance")
    r = rms_err(each, shared).max()
    print(f"ir_len {ir_len}: per-instance against shared, worst RMS {r:.3e}")
    assert_le(r, TOL_RMS, "per-instance mode against shared mode")


@gpu
def test_biquad_in_front_at_the_three_pass_size(hip, orc):
    """t1-shaped graph.  The planner hands the Biquad to the forward transform only when the source's AudioBuffer can be read in
    place, i.e. holds whole render quanta (shared responses alike): the buffer is 97 quanta, the render the usual 96 and 11 frames"""
    noise = white_noise(3, 2, RQ * 97)
    irs = _irs(3, 2, 49153)
    ctx, _ = per_inst(hip, noise, irs, with_biquad=True, length=FRAMES)
    conv = [l for l in ctx.plan_describe().splitlines() if l.startswith("convolver")]
    assert len(conv) == 1 and "the Biquad in front, in the forward transform" in conv[0] and "per-instance" in conv[0], conv
    assert "in the impulse response" not in ctx.plan_describe()
    got = ctx.start_rendering_sync().data
    ctx.close()
    assert_all_finite(got, "Biquad in front")
    assert_parity(got, oracle_each(orc, noise, irs, with_biquad=True, length=FRAMES), "Biquad -> Convolver, per-instance responses")


@gpu
def test_rearm_keeps_the_responses(hip):
    from rearm import assert_differs, assert_same_bits, dense, other_dense, refill_from, render_again
    irs = _irs(3, 2, 20000)
    a, b2 = dense(3, 2, FRAMES), other_dense(3, 2, FRAMES)
    ctx, _ = per_inst(hip, a, irs)
    first = ctx.start_rendering_sync().data
    donor, _ = per_inst(hip, b2, irs)  # (never applied: only its audio is taken)
    assert refill_from(ctx, donor) == 1
    again = render_again(ctx)
    ctx.close()
    fresh = render_device(hip, b2, irs, "fresh batch")
    assert_all_finite(again, "re-armed render")
    assert_differs(again, first)
    assert_same_bits(again, fresh)


@gpu
def test_exact_linear_convolution(hip, orc_lib):
    """the mathematical definition (f64 direct convolution), two different mono responses"""
    frames, ir_len = RQ * 64, 5000
    noise = white_noise(2, 1, frames)
    irs = _irs(2, 1, ir_len)
    out = render_device(hip, noise, irs, "exact")
    FP, DP = C.POINTER(C.c_float), C.POINTER(C.c_double)
    orc_lib.orc_convolver_normalization_scale.restype = C.c_float
    orc_lib.orc_convolver_normalization_scale.argtypes = [C.POINTER(FP), C.c_uint32, C.c_uint64, C.c_float]
    orc_lib.orc_convolve_exact.argtypes = [FP, C.c_uint64, FP, C.c_uint64, DP, C.c_uint64]
    for i in range(2):
        chans = (FP * 1)(irs[i, 0].ctypes.data_as(FP))
        scale = orc_lib.orc_convolver_normalization_scale(chans, 1, ir_len, SR)
        h = (irs[i, 0] * np.float32(scale)).astype(np.float32)
        ye = np.zeros(frames, np.float64)
        x = np.ascontiguousarray(noise[i, 0])
        orc_lib.orc_convolve_exact(x.ctypes.data_as(FP), frames, h.ctypes.data_as(FP), ir_len, ye.ctypes.data_as(DP), frames)
        for c in range(2):  # mono source + mono response -> mono, up-mixed to both destination channels
            r = np.sqrt(np.mean((out[i, c] - ye) ** 2))
            print(f"instance {i} channel {c}: RMS against the f64 convolution {r:.3e}")
            assert_le(r, TOL_RMS, f"instance {i} channel {c}")
