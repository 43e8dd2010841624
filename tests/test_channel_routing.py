"""ChannelSplitterNode / ChannelMergerNode (the reference's src/node/channel_splitter.rs, channel_merger.rs): output and input
ports in the C ABI, the planner and api.py; the route launch (csrc/waa_route.hip) and the splitter's output views.

The oracle cannot build these graphs (it has no ports), so the expected values come from (a) the reference's own unit tests,
re-typed; (b) channel selection, which is exact; (c) oracle renders of the port-free MONO sub-graphs, put together per channel
in numpy, with the down-mixes to mono restated in numpy f32 (tests/routing_model.py).  Every context of every batch is compared
and a non-finite sample on either side fails the case.

Bounds.  Channel selection, sums of two signals and the 2 -> 1 down-mix are one or two correctly rounded f32 operations: bit
equality.  The 4 -> 1 and 6 -> 1 down-mixes are compared at rel RMS 1e-6 per context (rms(a - b) / rms(b), the project's usual
f32 bound, tests/test_iir.py) — they are bit-equal too where the expression order matches, which the test prints.  Compositions
with Biquad / Gain / Delay / Convolver against the oracle: rel RMS 1e-6 per context and output channel.

Shapes: 3 contexts with different audio, 44100 Hz, 4396 frames (two full 2048-frame tiles plus 300: neither a whole render
quantum nor a whole tile); one case at 100 frames."""
import numpy as np
import pytest

import routing_model as rm
import web_audio_api_rs_amd as waa
from graphs import white_noise
from rearm import assert_differs, assert_same_bits, refill_from

SR = 44100.0
N_INST = 3
LENGTH = 2 * 2048 + 300
RQ = 128


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def context(be, n_out, length=LENGTH, device=-1, n_inst=N_INST, sr=SR):
    return waa.OfflineAudioContext(n_out, length, sr, n_instances=n_inst, binding=be, device=device)


def noise_source(ctx, n_ch, seed0, frames=None):
    """a BufferSource with one AudioBuffer per context; returns (node, audio [n_inst, n_ch, frames])"""
    audio = white_noise(ctx.n_instances, n_ch, frames or ctx.length, seed0=seed0)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(audio, ctx.sample_rate)
    src.start()
    return src, audio


def render(ctx):
    out = ctx.start_rendering_sync().data
    ctx.close()
    return out


def assert_finite(a, what):
    bad = ~np.isfinite(a)
    assert not bad.any(), f"{what} holds {int(bad.sum())} non-finite sample(s), the first at {tuple(int(v) for v in np.argwhere(bad)[0])}"


def assert_bits(got, want, what):
    """same bits in every context (x + 0.0 first: a zero compares as a zero whatever its sign)"""
    assert_finite(got, f"{what}: the device's output")
    assert_finite(want, f"{what}: the expected signal")
    assert_same_bits(np.ascontiguousarray(got) + np.float32(0.0), np.ascontiguousarray(want, np.float32) + np.float32(0.0), what=what)


def rel_rms(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    den = float(np.sqrt(np.mean(want ** 2)))
    assert den > 0.0, "the expected signal is all zeros: nothing to compare against"
    return float(np.sqrt(np.mean((got - want) ** 2))) / den


def assert_rel(got, want, what, bound=1e-6):
    """per context (first axis); every figure is printed before the first assertion"""
    assert got.shape == want.shape, (got.shape, want.shape)
    assert_finite(got, f"{what}: the device's output")
    assert_finite(want, f"{what}: the expected signal")
    figures = [rel_rms(got[i], want[i]) for i in range(got.shape[0])]
    for i, r in enumerate(figures):
        print(f"{what}, context {i}: rel RMS = {r:.3e} ({r / bound:.3f} of the bound {bound:.0e}), "
              f"{'bit-equal' if np.array_equal(got[i], want[i]) else 'not bit-equal'}")
    for i, r in enumerate(figures):
        assert r <= bound, f"{what}, context {i}: rel RMS {r:.3e} > {bound:.0e}"
    return max(figures)


def expect_error(status, text, fn):
    with pytest.raises(waa.WaaError) as e:
        fn()
    assert e.value.status == status and text in str(e.value), (e.value.status, str(e.value))
    return e.value


def plan_only(hip, n_out=2, length=LENGTH):
    return context(hip, n_out, length, device=waa.PLAN_ONLY)


# ---- CPU: messages ------------------------------------------------------------------------------------------------------------
SPLITTER_COUNT = "InvalidStateError - channel count of ChannelSplitterNode must be equal to number of outputs"
SPLITTER_MODE = "InvalidStateError - channel count of ChannelSplitterNode must be set to Explicit"
SPLITTER_INTERP = "InvalidStateError - channel interpretation of ChannelSplitterNode must be set to Discrete"
MERGER_COUNT = "InvalidStateError - channel count of ChannelMergerNode must be equal to 1"
MERGER_MODE = "InvalidStateError - channel count of ChannelMergerNode must be set to Explicit"


def test_api_defaults_and_port_counts(hip_product):
    ctx = plan_only(hip_product)
    sp, mg = ctx.create_channel_splitter(), ctx.create_channel_merger()
    assert (sp.number_of_inputs, sp.number_of_outputs) == (1, 6) and (mg.number_of_inputs, mg.number_of_outputs) == (6, 1)
    assert (sp.channel_count, sp.channel_count_mode, sp.channel_interpretation) == (6, "explicit", "discrete")
    assert (mg.channel_count, mg.channel_count_mode, mg.channel_interpretation) == (1, "explicit", "speakers")
    assert waa.NODE_CHANNEL_SPLITTER == 14 and waa.NODE_CHANNEL_MERGER == 15 and sp.kind == 14 and mg.kind == 15
    sp2 = ctx.create_channel_splitter(2)  # channel_splitter.rs:222-235
    assert sp2.number_of_outputs == 2 and sp2.channel_count == 2
    assert ctx.create_channel_merger(4, channel_interpretation="discrete").channel_interpretation == "discrete"
    assert ctx.create_gain().number_of_outputs == 1 and ctx.create_gain().number_of_inputs == 1


@pytest.mark.parametrize("ports", [0, 33])
def test_api_port_count_out_of_range(hip_product, ports):
    ctx = plan_only(hip_product)
    text = f"IndexSizeError - Invalid number of channels: {ports} is outside range [1, 32]"
    expect_error(1, text, lambda: ctx.create_channel_splitter(ports))
    expect_error(1, text, lambda: ctx.create_channel_merger(ports))


def test_api_channel_config_messages(hip_product):
    ctx = plan_only(hip_product)
    expect_error(3, SPLITTER_COUNT, lambda: ctx.create_channel_splitter(2, channel_count=3))
    expect_error(3, SPLITTER_COUNT, lambda: ctx.create_channel_splitter(channel_count=7))  # channel_splitter.rs:237-247
    expect_error(3, SPLITTER_MODE, lambda: ctx.create_channel_splitter(2, channel_count_mode="max"))
    expect_error(3, SPLITTER_INTERP, lambda: ctx.create_channel_splitter(2, channel_interpretation="speakers"))
    expect_error(3, MERGER_COUNT, lambda: ctx.create_channel_merger(2, channel_count=2))  # channel_merger.rs:183-193
    expect_error(3, MERGER_MODE, lambda: ctx.create_channel_merger(2, channel_count_mode="clamped-max"))
    sp, mg = ctx.create_channel_splitter(), ctx.create_channel_merger()
    expect_error(3, SPLITTER_COUNT, lambda: sp.set_channel_count(3))  # channel_splitter.rs:249-258
    expect_error(3, SPLITTER_MODE, lambda: sp.set_channel_count_mode("max"))
    expect_error(3, SPLITTER_INTERP, lambda: sp.set_channel_interpretation("speakers"))
    expect_error(3, MERGER_COUNT, lambda: mg.set_channel_count(3))  # channel_merger.rs:195-204
    expect_error(3, MERGER_MODE, lambda: mg.set_channel_count_mode("max"))
    sp.set_channel_count(6), sp.set_channel_count_mode("explicit"), sp.set_channel_interpretation("discrete")
    mg.set_channel_count(1), mg.set_channel_count_mode("explicit"), mg.set_channel_interpretation("discrete")
    assert mg.channel_interpretation == "discrete"


def test_api_connect_and_disconnect_check_both_ports(hip_product):
    ctx = plan_only(hip_product)
    sp, mg, g = ctx.create_channel_splitter(2), ctx.create_channel_merger(2), ctx.create_gain()
    expect_error(1, "IndexSizeError - output port 2 is out of bounds", lambda: sp.connect(g, 2))
    expect_error(1, "IndexSizeError - output port 1 is out of bounds", lambda: g.connect(mg, 1, 0))
    expect_error(1, "IndexSizeError - output port 1 is out of bounds", lambda: g.connect(g.gain, 1))
    expect_error(1, "IndexSizeError - input port 2 is out of bounds", lambda: g.connect(mg, 0, 2))
    expect_error(1, "IndexSizeError - input port 1 is out of bounds", lambda: sp.connect(g, 1, 1))
    sp.connect(g, 1)
    g.connect(mg, 0, 1)
    expect_error(1, "IndexSizeError - output port 2 is out of bounds", lambda: sp.disconnect_output(2))
    expect_error(1, "IndexSizeError - output port 1 is out of bounds", lambda: g.disconnect_dest_from_output(mg, 1))
    expect_error(1, "IndexSizeError - input port 2 is out of bounds", lambda: g.disconnect_dest_from_output_to_input(mg, 0, 2))
    expect_error(1, "InvalidAccessError - attempting to disconnect unconnected nodes", lambda: g.disconnect_dest_from_output_to_input(mg, 0, 0))
    g.disconnect_dest_from_output_to_input(mg, 0, 1)  # a valid input of a merger
    sp.disconnect_output(1)                           # a valid output of a splitter
    assert ctx._live == []


def _abi_graph(hip, tweak):
    """source -> splitter(2) -> gain -> merger(2) -> destination, `tweak(ctx, nodes)` applied before the batch is created"""
    ctx = plan_only(hip)
    src, _ = noise_source(ctx, 2, 1)
    sp, mg, g = ctx.create_channel_splitter(2), ctx.create_channel_merger(2), ctx.create_gain()
    src.connect(sp)
    sp.connect(g, 1)
    g.connect(mg, 0, 1)
    mg.connect(ctx.destination())
    tweak(ctx, dict(src=src, sp=sp, mg=mg, g=g))
    return ctx


def _force_config(node, **kw):
    node._explicit_config = True
    for k, v in kw.items():
        setattr(node, k, v)


@pytest.mark.parametrize("text,status,tweak", [
    ("IndexSizeError - Invalid number of channels: 33 is outside range [1, 32]", 1, lambda c, n: setattr(n["sp"], "number_of_outputs", 33)),
    ("IndexSizeError - Invalid number of channels: -1 is outside range [1, 32]", 1, lambda c, n: setattr(n["mg"], "number_of_inputs", -1)),
    ("IndexSizeError - Invalid number of channels: 33 is outside range [1, 32]", 1, lambda c, n: setattr(n["mg"], "number_of_inputs", 33)),
    (SPLITTER_COUNT, 3, lambda c, n: _force_config(n["sp"], channel_count=3)),
    (SPLITTER_MODE, 3, lambda c, n: _force_config(n["sp"], channel_count_mode="max")),
    (SPLITTER_INTERP, 3, lambda c, n: _force_config(n["sp"], channel_interpretation="speakers")),
    (MERGER_COUNT, 3, lambda c, n: _force_config(n["mg"], channel_count=2)),
    (MERGER_MODE, 3, lambda c, n: _force_config(n["mg"], channel_count_mode="clamped-max")),
    ("IndexSizeError - output port 2 is out of bounds", 1, lambda c, n: c._edges.append((n["sp"].id, 2, n["g"].id, 0))),
    ("IndexSizeError - input port 2 is out of bounds", 1, lambda c, n: c._edges.append((n["g"].id, 0, n["mg"].id, 2))),
    # the old rule still holds for every other kind: a GainNode has one output and one input
    ("IndexSizeError - output port 1 is out of bounds", 1, lambda c, n: c._edges.append((n["g"].id, 1, n["mg"].id, 0))),
    ("IndexSizeError - input port 1 is out of bounds", 1, lambda c, n: c._edges.append((n["sp"].id, 0, n["g"].id, 1))),
])
def test_abi_creation_messages(hip_product, text, status, tweak):
    ctx = _abi_graph(hip_product, tweak)
    expect_error(status, text, ctx.prepare)


def test_abi_connect_and_disconnect_check_both_ports(hip_product):
    ctx = _abi_graph(hip_product, lambda c, n: None).prepare()
    b, h = ctx._b, ctx._handle
    src, sp, mg, g = 1, 2, 3, 4
    assert [type(n).__name__ for n in ctx._nodes[1:5]] == ["AudioBufferSourceNode", "ChannelSplitterNode", "ChannelMergerNode", "GainNode"]
    for fn in (b.connect, b.disconnect):
        expect_error(1, "IndexSizeError - output port 2 is out of bounds", lambda: b.check(fn(h, sp, 2, g, 0)))
        expect_error(1, "IndexSizeError - output port 1 is out of bounds", lambda: b.check(fn(h, g, 1, mg, 0)))
        expect_error(1, "IndexSizeError - input port 2 is out of bounds", lambda: b.check(fn(h, g, 0, mg, 2)))
        expect_error(1, "IndexSizeError - input port 1 is out of bounds", lambda: b.check(fn(h, sp, 0, g, 1)))
    b.check(b.connect(h, sp, 0, mg, 0))
    b.check(b.disconnect(h, sp, 0, mg, 0))
    b.check(b.disconnect(h, g, 0, mg, 1))
    expect_error(1, "InvalidAccessError - attempting to disconnect unconnected nodes", lambda: b.check(b.disconnect(h, g, 0, mg, 1)))
    ctx.close()


# ---- CPU: plans -----------------------------------------------------------------------------------------------------------------
def test_plan_views_and_one_route_launch(hip_product):
    """stereo source -> splitter(2) -> one gain per output -> merger(2) -> destination plans without a device: the splitter is
    views of its producer's signal (no launch of its own), the merger is the one route launch"""
    ctx = plan_only(hip_product)
    src, _ = noise_source(ctx, 2, 1)
    sp, mg = ctx.create_channel_splitter(2), ctx.create_channel_merger(2)
    src.connect(sp)
    for k, gain in enumerate((0.5, 0.25)):
        g = ctx.create_gain(gain=gain)
        sp.connect(g, k)
        g.connect(mg, 0, k)
    mg.connect(ctx.destination())
    text = ctx.plan_describe()
    ctx.close()
    lines = text.splitlines()
    assert any(f"splitter node {sp.id}: 2 output(s), views of node {src.id}" in ln and "no launch" in ln for ln in lines), text
    assert not any("splitter node" in ln and "route launch" in ln for ln in lines), text
    assert sum("route_kernel" in ln for ln in lines) == 1 and text.count("route_kernel") == 1, text
    assert any(ln.startswith(f"merger node {mg.id}: 2 input(s) (speakers)") and "route_kernel" in ln for ln in lines), text


def test_plan_splitter_with_two_connections_is_a_route_launch(hip_product):
    ctx = plan_only(hip_product, 6)
    a, _ = noise_source(ctx, 2, 1)
    c, _ = noise_source(ctx, 6, 2)
    sp, mg = ctx.create_channel_splitter(6), ctx.create_channel_merger(6)
    a.connect(sp)
    c.connect(sp)
    for k in range(6):
        sp.connect(mg, k, k)
    mg.connect(ctx.destination())
    text = ctx.plan_describe()
    ctx.close()
    assert f"splitter node {sp.id}: 6 output(s), 2 connection(s), mixed by route launch -> route_kernel (8 term(s))" in text, text
    assert text.count("route_kernel") == 2, text


def test_refused_splitter_inside_a_feedback_loop(hip_product):
    ctx = plan_only(hip_product)
    src, _ = noise_source(ctx, 2, 1)
    g, sp, d = ctx.create_gain(gain=0.5), ctx.create_channel_splitter(2), ctx.create_delay()
    d.delay_time.value = 0.01
    src.connect(g).connect(sp)
    sp.connect(d, 1)
    d.connect(g)
    sp.connect(ctx.destination(), 0)
    err = expect_error(4, f"ChannelSplitterNode {sp.id} inside a feedback loop is out of scope", ctx.plan_describe)
    assert "static plans only" in str(err)
    ctx.close()


def test_refused_merger_where_the_replay_asks_for_exact_counts(hip_product):
    """a merger in front of an equal-power PannerNode whose sources stop mid-render: the merger's output goes from two channels to
    one silent channel (channel_merger.rs:160-168) in front of a node whose law depends on the count"""
    ctx = plan_only(hip_product)
    mg, pan = ctx.create_channel_merger(2), ctx.create_panner()
    for k in range(2):
        s, _ = noise_source(ctx, 1, 10 + k)
        s.stop_at(0.05)
        s.connect(mg, 0, k)
    mg.connect(pan).connect(ctx.destination())
    err = expect_error(4, f"ChannelMergerNode {mg.id} in a graph that needs exact per-quantum channel counts", ctx.plan_describe)
    assert "static plans only" in str(err)
    ctx.close()


# ---- CPU: the model against hand-computed values ----------------------------------------------------------------------------------
def test_routing_model_hand_computed():
    f = np.float32
    col = lambda *v: np.array(v, f).reshape(-1, 1)  # noqa: E731 (one frame, one value per channel)
    assert rm.down_mix_to_mono(col(0.25, 0.75))[0] == f(0.5)
    assert rm.down_mix_to_mono(col(1.0, 2.0, 3.0, 4.0))[0] == f(2.5)
    # 6 -> 1: sqrt(0.5) * (1 + 1) + 0.5 + 0.5 * (2 + 4) = 1.41421354 + 3.5
    got = rm.down_mix_to_mono(col(1.0, 1.0, 0.5, 100.0, 2.0, 4.0))[0]
    assert got == f(np.float64(f(np.sqrt(f(0.5)))) * 2.0 + 3.5) and abs(float(got) - 4.914213562) < 1e-6
    assert rm.down_mix_to_mono(col(0.25, 0.75), "discrete")[0] == f(0.25)
    assert rm.down_mix_to_mono(col(1.0, 2.0, 3.0, 4.0, 5.0, 6.0), "discrete")[0] == f(1.0)
    assert rm.down_mix_to_mono(col(7.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0))[0] == f(7.0)  # 8 -> 1: above six channels, channel 0
    assert rm.down_mix_to_mono(col(3.0, 1.0, 1.0))[0] == f(3.0)                            # no speakers rule for 3 -> 1
    assert rm.merger_port([col(0.25, 0.75), col(0.125)])[0] == f(0.625)
    m = rm.merger([[col(1.0)], [], [col(2.0, 4.0)]], 1)
    assert m.shape == (3, 1) and m[:, 0].tolist() == [1.0, 0.0, 3.0]
    s = rm.splitter([np.array([[1.0], [2.0]], f), np.array([[10.0], [20.0], [30.0]], f)], 4, 1)
    assert s[:, 0].tolist() == [11.0, 22.0, 30.0, 0.0]


# ---- GPU 1: the reference's three unit tests, re-typed ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reference_test_splitter(hip):
    """channel_splitter.rs:261-282"""
    ctx = context(hip, 1, 128, sr=48000.0)
    sp = ctx.create_channel_splitter(2)
    sp.connect(ctx.destination(), 1, 0)
    src = ctx.create_buffer_source()
    src.set_buffer(waa.AudioBuffer(np.array([[1.0], [-1.0]], np.float32), 48000.0))
    src.set_loop(True)
    src.start()
    src.connect(sp)
    out = render(ctx)
    assert out.shape == (N_INST, 1, 128)
    assert_bits(out, np.full((N_INST, 1, 128), -1.0, np.float32), "test_splitter")


def _two_constants_into_a_merger(hip, length):
    ctx = context(hip, 2, length, sr=48000.0)
    mg = ctx.create_channel_merger(2)
    mg.connect(ctx.destination())
    srcs = []
    for k, v in enumerate((2.0, 3.0)):
        s = ctx.create_constant_source()
        s.offset.value = v
        s.connect(mg, 0, k)
        s.start()
        srcs.append(s)
    return ctx, srcs


@pytest.mark.gpu
def test_reference_test_merge(hip):
    """channel_merger.rs:207-231"""
    ctx, _ = _two_constants_into_a_merger(hip, 128)
    out = render(ctx)
    want = np.empty((N_INST, 2, 128), np.float32)
    want[:, 0], want[:, 1] = 2.0, 3.0
    assert_bits(out, want, "test_merge")


@pytest.mark.gpu
def test_reference_test_merge_disconnect(hip):
    """channel_merger.rs:234-271: output 0 of src2 is disconnected at a suspend point half-way"""
    length = 4 * 128
    ctx, (_, src2) = _two_constants_into_a_merger(hip, length)
    ctx.suspend_sync(length / 48000.0 / 2.0, lambda c: src2.disconnect())
    out = render(ctx)
    want = np.empty((N_INST, 2, length), np.float32)
    want[:, 0] = 2.0
    want[:, 1, :length // 2] = 3.0
    want[:, 1, length // 2:] = 0.0
    assert_bits(out, want, "test_merge_disconnect")


# ---- GPU 2: every output of a splitter in one render ----------------------------------------------------------------------------------
def reversing_graph(be, c, n, length=LENGTH, audio=None):
    """C-channel source -> splitter(N) -> output k to merger(N) input N-1-k -> N-channel destination"""
    ctx = context(be, n, length)
    if audio is None:
        src, audio = noise_source(ctx, c, 0x5711 + 100 * c + n)
    else:
        src = ctx.create_buffer_source()
        src.set_buffer_batch(audio, SR)
        src.start()
    sp, mg = ctx.create_channel_splitter(n), ctx.create_channel_merger(n)
    src.connect(sp)
    for k in range(n):
        sp.connect(mg, k, n - 1 - k)
    mg.connect(ctx.destination())
    return ctx, audio


def reversed_channels(audio, n):
    n_inst, c, frames = audio.shape
    want = np.zeros((n_inst, n, frames), np.float32)
    for k in range(min(c, n)):
        want[:, n - 1 - k] = audio[:, k]
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("c,n,length", [(1, 1, LENGTH), (2, 2, LENGTH), (2, 6, LENGTH), (6, 2, LENGTH), (6, 6, LENGTH), (8, 8, LENGTH),
                                        (4, 32, LENGTH), (32, 32, LENGTH), (2, 2, 100)])
def test_splitter_every_output(hip, c, n, length):
    ctx, audio = reversing_graph(hip, c, n, length)
    out = render(ctx)
    want = reversed_channels(audio, n)
    assert_bits(out, want, f"splitter({n}) behind a {c}-channel source")
    for k in range(c, n):
        assert not out[:, n - 1 - k].any(), f"output {k} of the splitter lies beyond the source's {c} channels and is not exactly zero"


# ---- GPU 3: a splitter whose input sums two connections -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_splitter_with_two_connections(hip):
    ctx = context(hip, 6)
    a, stereo = noise_source(ctx, 2, 0x21)
    b, six = noise_source(ctx, 6, 0x61)
    sp, mg = ctx.create_channel_splitter(6), ctx.create_channel_merger(6)
    a.connect(sp)
    b.connect(sp)
    for k in range(6):
        sp.connect(mg, k, k)
    mg.connect(ctx.destination())
    out = render(ctx)
    want = np.stack([rm.splitter([stereo[i], six[i]], 6, LENGTH) for i in range(N_INST)])
    assert_bits(out, want, "splitter(6) behind a stereo and a 5.1 source")


# ---- GPU 4: the merger's down-mixes -------------------------------------------------------------------------------------------------
MERGER_WIDTHS = (1, 2, 4, 6, 8)  # input ports 0 .. 4; port 5 stays unconnected


def merger_graph(be, interpretation):
    ctx = context(be, 6)
    kw = {} if interpretation == "speakers" else dict(channel_interpretation=interpretation)
    mg = ctx.create_channel_merger(6, **kw)
    audio = []
    for port, width in enumerate(MERGER_WIDTHS):
        s, a = noise_source(ctx, width, 0x700 + width)
        s.connect(mg, 0, port)
        audio.append(a)
    mg.connect(ctx.destination())
    return ctx, audio


@pytest.mark.gpu
def test_merger_down_mixes_speakers(hip):
    ctx, audio = merger_graph(hip, "speakers")
    out = render(ctx)
    want = np.stack([rm.merger([[a[i]] for a in audio] + [[]], LENGTH) for i in range(N_INST)])
    for port, width in enumerate(MERGER_WIDTHS):
        if width in (4, 6):
            r = assert_rel(out[:, port], want[:, port], f"merger input {port} ({width} -> 1, speakers)")
            print(f"worst ratio to the bound, {width} -> 1: {r / 1e-6:.3f}")
        else:
            assert_bits(out[:, port], want[:, port], f"merger input {port} ({width} -> 1, speakers)")
    assert not out[:, 5].any(), "the unconnected input 5 is not exactly zero"


@pytest.mark.gpu
def test_merger_down_mixes_discrete(hip):
    ctx, audio = merger_graph(hip, "discrete")
    out = render(ctx)
    for port, a in enumerate(audio):
        assert_bits(out[:, port], a[:, 0], f"merger input {port} ({a.shape[1]} channels, discrete)")
    assert not out[:, 5].any(), "the unconnected input 5 is not exactly zero"


@pytest.mark.gpu
def test_merger_input_with_two_connections(hip):
    ctx = context(hip, 2)
    mg = ctx.create_channel_merger(2)
    a, stereo = noise_source(ctx, 2, 0x22)
    b, mono = noise_source(ctx, 1, 0x11)
    a.connect(mg, 0, 1)
    b.connect(mg, 0, 1)
    mg.connect(ctx.destination())
    out = render(ctx)
    want = np.zeros((N_INST, 2, LENGTH), np.float32)
    for i in range(N_INST):
        want[i, 1] = rm.merger_port([stereo[i], mono[i]])
    assert_bits(out, want, "merger input fed by a stereo and a mono source")


# ---- GPU 5: composition against the oracle ------------------------------------------------------------------------------------------
IR = (np.random.default_rng(0x1F).uniform(-1.0, 1.0, (1, 300)) * np.exp(-np.arange(300) / 60.0)).astype(np.float32)


def _stereo_audio():
    return white_noise(N_INST, 2, LENGTH, seed0=0x5E0)


def _mono_source(ctx, audio, ch):
    s = ctx.create_buffer_source()
    s.set_buffer_batch(np.ascontiguousarray(audio[:, ch:ch + 1]), SR)
    s.start()
    return s


def _lowpass(ctx):
    return ctx.create_biquad_filter(type_="lowpass", frequency=1200.0, q=0.9)


def _half_then_delay(ctx, src):
    d = ctx.create_delay()
    d.delay_time.value = 0.01
    src.connect(ctx.create_gain(gain=0.5)).connect(d)
    return d


@pytest.fixture(scope="module")
def oracle_parts(orc):
    """the mono sub-graphs on the oracle, rendered once: name -> [n_inst, frames]"""
    audio = _stereo_audio()
    parts = {}

    def mono(name, build):
        ctx = context(orc, 1)
        build(ctx)
        parts[name] = render(ctx)[:, 0]
        assert_finite(parts[name], f"oracle part {name}")

    mono("lowpass(ch0)", lambda c: _mono_source(c, audio, 0).connect(_lowpass(c)).connect(c.destination()))
    mono("delay(0.5 ch1)", lambda c: _half_then_delay(c, _mono_source(c, audio, 1)).connect(c.destination()))

    def fan_out(c):
        _half_then_delay(c, _mono_source(c, audio, 1)).connect(c.destination())
        _mono_source(c, audio, 0).connect(c.create_gain(gain=0.25)).connect(c.destination())
    mono("delay(0.5 ch1) + 0.25 ch0", fan_out)

    def modulated(c):
        g = c.create_gain()
        _mono_source(c, audio, 0).connect(g).connect(c.destination())
        _mono_source(c, audio, 1).connect(g.gain)
    mono("ch0 * (1 + ch1)", modulated)

    def convolved(c):
        cv = c.create_convolver()
        cv.set_buffer(waa.AudioBuffer(IR, SR))
        _mono_source(c, audio, 1).connect(cv).connect(c.destination())
    mono("conv(ch1)", convolved)
    return audio, parts


def _composition(hip, audio, variant):
    """stereo source -> splitter(2); output 0 -> lowpass -> merger input 1; output 1 -> (variant) -> merger input 0"""
    ctx = context(hip, 2)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(audio, SR)
    src.start()
    sp, mg = ctx.create_channel_splitter(2), ctx.create_channel_merger(2)
    src.connect(sp)
    lp = _lowpass(ctx)
    sp.connect(lp, 0)
    lp.connect(mg, 0, 1)
    if variant in ("plain", "fan-out"):
        d = ctx.create_delay()
        d.delay_time.value = 0.01
        g = ctx.create_gain(gain=0.5)
        sp.connect(g, 1)
        g.connect(d).connect(mg, 0, 0)
        if variant == "fan-out":  # output 0 feeds a second consumer
            q = ctx.create_gain(gain=0.25)
            sp.connect(q, 0)
            q.connect(mg, 0, 0)
    elif variant == "param":  # output 1 drives a GainNode's gain
        g = ctx.create_gain()
        sp.connect(g, 0)
        sp.connect(g.gain, 1)
        g.connect(mg, 0, 0)
    else:  # a node-major consumer behind output 1
        cv = ctx.create_convolver()
        cv.set_buffer(waa.AudioBuffer(IR, SR))
        sp.connect(cv, 1)
        cv.connect(mg, 0, 0)
    mg.connect(ctx.destination())
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("variant,left", [("plain", "delay(0.5 ch1)"), ("fan-out", "delay(0.5 ch1) + 0.25 ch0"), ("param", "ch0 * (1 + ch1)"),
                                          ("convolver", "conv(ch1)")])
def test_composition_against_the_oracle(hip, oracle_parts, variant, left):
    audio, parts = oracle_parts
    out = render(_composition(hip, audio, variant))
    assert out.shape == (N_INST, 2, LENGTH)
    r0 = assert_rel(out[:, 0], parts[left], f"{variant}: channel 0 = {left}")
    r1 = assert_rel(out[:, 1], parts["lowpass(ch0)"], f"{variant}: channel 1 = lowpass(ch0)")
    print(f"{variant}: worst ratio to the bound = {max(r0, r1) / 1e-6:.3f}")


# ---- GPU 6: re-arm ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rearm_with_new_audio(hip):
    first_audio = white_noise(N_INST, 2, LENGTH, seed0=0xA1)
    next_audio = white_noise(N_INST, 2, LENGTH, seed0=0xB2)
    ctx, _ = reversing_graph(hip, 2, 2, audio=first_audio)
    first = ctx.start_rendering_sync().data
    donor, _ = reversing_graph(hip, 2, 2, audio=next_audio)
    assert refill_from(ctx, donor) == 1
    from rearm import render_again
    again = render_again(ctx)
    fresh = render(donor)
    ctx.close()
    assert_finite(again, "the re-armed render")
    assert_same_bits(again, fresh)
    assert_same_bits(fresh, reversed_channels(next_audio, 2), what="the fresh render")
    assert_differs(again, first)


# ---- outputs beyond the producer's channels behind a consumer that is no merger: the bus is materialised ---------------------------
def beyond_graph(be, device=-1):
    """stereo source -> splitter(6); output 1 -> merger input 0; output 3 (beyond the source's channels) -> Gain 0.5 -> merger
    input 1; output 0 -> Gain whose gain (0.5) also takes output 4 (beyond as well) as its audio-rate input -> merger input 2"""
    ctx = context(be, 3, device=device)
    src, audio = noise_source(ctx, 2, 0xBE)
    sp, mg = ctx.create_channel_splitter(6), ctx.create_channel_merger(3)
    src.connect(sp)
    sp.connect(mg, 1, 0)
    g = ctx.create_gain(gain=0.5)
    sp.connect(g, 3)
    g.connect(mg, 0, 1)
    m = ctx.create_gain(gain=0.5)
    sp.connect(m, 0)
    sp.connect(m.gain, 4)
    m.connect(mg, 0, 2)
    mg.connect(ctx.destination())
    return ctx, audio, sp


def test_plan_silent_output_into_a_gain_materialises_the_bus(hip_product):
    ctx, _, sp = beyond_graph(hip_product, waa.PLAN_ONLY)
    text = ctx.plan_describe()
    ctx.close()
    assert f"splitter node {sp.id}: 6 output(s), 1 connection(s), mixed by route launch -> route_kernel (2 term(s))" in text, text
    assert "views of node" not in text, text
