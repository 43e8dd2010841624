"""waa_batch_rearm — "same graph, new audio", the serving path (waa_render_sharded re-arms every sub-batch after the first when
reuse_batches is set, and bench.py's e2e record does so by default) — on NEW audio: a rendered batch is re-armed, refilled with
audio B and rendered, and must equal a fresh batch of the same graph on B bit for bit (tests/rearm.py).  A re-render of the same
audio cannot see a kernel or a plan that keeps something derived from the audio it rendered first; this can.

- random graphs (tests/test_fuzz_graphs.py, both generators) over three (A -> B) audio pairs, B also against the oracle;
- every bench.py workload with an input, fed as the bench feeds it (a device tensor adopted by the source, overwritten in place);
- a plan that holds values rendered from the graph at plan time (a source's playbackRate / detune, a panner's position driven from
  the graph) is refused, whatever the modulator reads;
- the contract's edges: refills of another shape or kind, a per-instance source, a source left as it was, suspend points, PCM that
  is decoded and resampled."""
import ctypes

import numpy as np
import pytest

import web_audio_api_rs_amd as waa
from bench_workloads import ELSEWHERE, FRAMES, HRTF_PER_CONTEXT, HRTF_PER_CONTEXT_ROUTE, SR, WORKLOADS, load_bench
from graphs import rms_err
from rearm import (PAIRS, RQ, assert_differs, assert_same_bits, dense, first_difference, live_quanta, modulated_graph, other_dense,
                   refill_from, render_again, sparse, sparsify)
from test_fuzz_graphs import build_random_graph


N_PLAIN, N_FROZEN = 40, 24  # random graphs per audio pair, of the plain and of the frozen-state generator


def _batch_filled_seeds(binding, frozen, count):
    """the first `count` seeds of the generator whose graph has a batch-filled BufferSource (a graph of oscillators and constant
    sources has no audio to change); the graphs are only described on `binding`, nothing is planned"""
    seeds, seed = [], 0
    while len(seeds) < count:
        ctx, _ = build_random_graph(binding, seed, frozen=frozen)
        if any(isinstance(nd, waa.AudioBufferSourceNode) and nd._batch is not None for nd in ctx._nodes):
            seeds.append(seed)
        seed += 1
    return seeds


@pytest.fixture(scope="module")
def random_seeds(orc):
    """{frozen: seed list}.  (A fixture, not a module constant: describing a graph without a binding loads the product library, and
    at collection time that would bypass conftest's build of a missing or stale library.)"""
    return {False: _batch_filled_seeds(orc, False, N_PLAIN), True: _batch_filled_seeds(orc, True, N_FROZEN)}


# ---- CPU: the generator's audio argument changes nothing but the audio; the patterns are what they say --------------------------

def _graph_bytes(ctx):
    g = ctx.graph_desc()
    nodes = bytes((waa.api.NodeDesc * g.n_nodes).from_address(ctypes.addressof(g.nodes.contents)))
    edges = bytes((waa.api.EdgeDesc * g.n_edges).from_address(ctypes.addressof(g.edges.contents))) if g.n_edges else b""
    return nodes, edges


def _params_and_schedules(ctx):
    """everything else a node of the mirror holds that the graph description does not: param values, automation, value blocks,
    start / stop times, loops"""
    out = []
    for nd in ctx._nodes:
        for p in getattr(nd, "params", []):
            out.append((nd.id, p._pid, repr(sorted(p._const.items())), repr(p._events), repr(p._blocks)))
        out.append((nd.id, repr(getattr(nd, "_starts", None)), repr(getattr(nd, "_stops", None)), repr(getattr(nd, "_loop", None))))
    return out


@pytest.mark.parametrize("frozen", [False, True])
def test_generator_audio_argument_keeps_every_graph(orc, frozen):
    """build_random_graph(..., audio=...) draws what it always drew: the same graph description, the same params and schedules,
    the same buffer shapes; under the default the batch arrays are bit-identical to white_noise's"""
    for seed in range(60):
        plain, d0 = build_random_graph(orc, seed, frozen=frozen)
        default, d1 = build_random_graph(orc, seed, frozen=frozen, audio=dense)
        other, d2 = build_random_graph(orc, seed, frozen=frozen, audio=sparse)
        assert d0 == d1 == d2
        assert _graph_bytes(plain) == _graph_bytes(default) == _graph_bytes(other), seed
        assert _params_and_schedules(plain) == _params_and_schedules(default) == _params_and_schedules(other), seed
        for a, b, c in zip(plain._nodes, default._nodes, other._nodes):
            if isinstance(a, waa.AudioBufferSourceNode) and a._batch is not None:
                assert a._batch[1] == b._batch[1] == c._batch[1]
                assert np.array_equal(a._batch[0].view(np.uint32), b._batch[0].view(np.uint32)), seed
                assert c._batch[0].shape == a._batch[0].shape and not np.array_equal(c._batch[0], a._batch[0])


def test_sparse_pattern():
    """instance 0 silent; every other instance has whole silent quanta at a pattern of its own and runs of silence longer than a
    convolver segment; what is kept is the noise"""
    n, nq = 6, 82
    x = other_dense(n, 2, nq * RQ - 40)
    s = sparsify(x)
    keep = live_quanta(n, nq)
    assert not s[0].any() and not keep[0].any()
    for i in range(1, n):
        assert keep[i].any() and not keep[i].all()
        runs, cur = [], 0
        for k in keep[i]:
            cur = 0 if k else cur + 1
            runs.append(cur)
        assert max(runs) * RQ > 1024
        for q in range(nq):
            seg = slice(q * RQ, (q + 1) * RQ)
            if keep[i, q]:
                assert np.array_equal(s[i, :, seg], x[i, :, seg])
            else:
                assert not s[i, :, seg].any() and not np.signbit(s[i, :, seg]).any()
        for j in range(1, i):
            assert not np.array_equal(keep[i], keep[j])
    assert np.array_equal(sparse(n, 2, nq * RQ - 40), s)


def test_first_difference_names_the_sample():
    a = other_dense(3, 2, 300)
    b = a.copy()
    assert first_difference(a, b) is None
    b[2, 1, 77] = np.nextafter(b[2, 1, 77], np.float32(2))
    b[2, 1, 90] += np.float32(0.5)
    assert first_difference(a, b)[1] == (2, 1, 77)
    with pytest.raises(AssertionError, match=r"\(instance, channel, frame\) \(2, 1, 77\)"):
        assert_same_bits(b, a)
    z = np.zeros((1, 1, 4), np.float32)
    assert first_difference(z, -z) is not None  # +0.0 and -0.0 differ in their bits
    with pytest.raises(AssertionError, match="nothing was refilled"):
        assert_differs(a, a.copy())


def test_every_bench_workload_with_an_input_is_covered():
    bench = load_bench()
    names = {n for n, w in WORKLOADS.items() if w.has_input} | set(ELSEWHERE)
    assert names == set(bench.ALG_BYTES) - {"osc", "fm"} == {n for n, _ in BENCH_CASES if n != "hrtf"} | {"hrtf"}


# ---- random graphs (-m gpu) -----------------------------------------------------------------------------------------------------

def _rearm_random_graph(hip, orc, seed, pair, frozen):
    audio_a, audio_b = PAIRS[pair]
    ctx, descr = build_random_graph(hip, seed, frozen=frozen, audio=audio_a)
    descr = f"seed {seed}: {descr}"
    donor = None
    try:
        try:
            first = ctx.start_rendering_sync().data
        except waa.WaaError as e:
            if e.status == 4:
                pytest.skip(f"out of scope on the device path: {e} [{descr}]")
            raise
        donor, _ = build_random_graph(hip, seed, frozen=frozen, audio=audio_b)
        assert refill_from(ctx, donor) > 0, descr
        got = render_again(ctx)
        want = donor.start_rendering_sync().data
    finally:
        ctx.close()
        if donor is not None:
            donor.close()
    assert_same_bits(got, want, f"[{descr}] the re-armed render")
    assert_differs(got, first, f"[{descr}] the re-armed render")
    co, _ = build_random_graph(orc, seed, frozen=frozen, audio=audio_b)
    try:
        o = co.start_rendering_sync().data
    finally:
        co.close()
    # (test_random_graph_parity's bounds)
    assert np.isfinite(o).all(), descr
    scale = max(1.0, float(np.abs(o).max()))
    assert rms_err(got, o).max() <= 1e-6 * scale, f"{descr}: rms {rms_err(got, o).max():.3g}"
    assert np.abs(got - o).max() <= 2e-5 * scale, f"{descr}: max |d| {np.abs(got - o).max():.3g}"


@pytest.mark.gpu
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("k", range(N_PLAIN))
def test_random_graph_rearmed_on_new_audio(hip, orc, random_seeds, k, pair):
    """k: the k-th seed of the plain generator whose graph has a batch-filled source"""
    _rearm_random_graph(hip, orc, random_seeds[False][k], pair, frozen=False)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("k", range(N_FROZEN))
def test_random_graph_rearmed_on_new_audio_frozen_state_nodes(hip, orc, random_seeds, k, pair):
    """oversampled WaveShapers (their frozen resampler state over silent quanta) and HRTF panners (the exact-zeros form, the tail
    counter) on audio whose zeros fall elsewhere; k: the k-th seed of the frozen-state generator with a batch-filled source"""
    _rearm_random_graph(hip, orc, random_seeds[True][k], pair, frozen=True)


# ---- every bench workload with an input, as the bench feeds it (-m gpu) ----------------------------------------------------------

BENCH_CASES = [(n, False) for n in sorted({n for n, w in WORKLOADS.items() if w.has_input} | set(ELSEWHERE))] + [("hrtf", True)]
# contexts per batch: 64, or where 64 would change the route the test asserts, the fewest that keep it (echo: the LDS-ring kernel
# from 256 contexts on)
BENCH_CONTEXTS = {"echo": 256}


def _fill(torch, t, pattern, seed):
    """overwrite the [n, 2, FRAMES] device tensor in place: uniform noise of `seed`, and for "sparse" the sparse pattern's quanta
    set to +0.0"""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    t.uniform_(-1.0, 1.0, generator=gen)
    if pattern == "sparse":
        n = t.shape[0]
        keep = torch.from_numpy(live_quanta(n, FRAMES // RQ)).to("cuda")
        t.view(n, 2, FRAMES // RQ, RQ).masked_fill_(~keep[:, None, :, None], 0.0)


def _render(ctx, pull):
    """render (planning first if needed), the analyser pull if any, the download"""
    ctx.prepare()
    ctx._b.check(ctx._b.render(ctx._handle))
    ctx.sync()
    bins = None
    if pull:
        an = next(nd for nd in ctx._nodes if isinstance(nd, waa.AnalyserNode))
        bins = an.get_float_frequency_data_all()
    out = np.empty((ctx.n_instances, ctx.number_of_channels, ctx.length), np.float32)
    ctx._b.check(ctx._b.download_all(ctx._handle, waa.api._fp(out)))
    return out, bins


@pytest.fixture(scope="module")
def bench():
    return load_bench()


@pytest.mark.gpu
@pytest.mark.parametrize("name,per_context", BENCH_CASES)
def test_bench_workload_rearmed_on_new_audio(hip, bench, name, per_context, monkeypatch):
    """bench.build_workload's graph on a device tensor the source adopts: render on noise A; then twice — re-arm, overwrite the
    SAME tensor with the next audio (sparse, then other dense noise), adopt the same pointer again, render — and each render must
    equal a fresh batch on that audio bit for bit (c4: its batched analyser pull too)"""
    import torch
    if per_context:
        monkeypatch.setenv(HRTF_PER_CONTEXT, "1")
    else:
        monkeypatch.delenv(HRTF_PER_CONTEXT, raising=False)
    n = BENCH_CONTEXTS.get(name, 64)
    pull = name == "c4"
    noise = torch.empty((n, 2, FRAMES), dtype=torch.float32, device="cuda")
    ctx = fresh = None
    # (the batches and the tensor go on every path: a failure's traceback would otherwise keep up to a GB of device memory alive)
    try:
        _fill(torch, noise, "dense", 0xB0E)
        torch.cuda.synchronize()
        ctx, src = bench.build_workload(waa, hip, name, n, FRAMES, 0, noise.data_ptr())
        prev, _ = _render(ctx, pull)
        route = HRTF_PER_CONTEXT_ROUTE if per_context else WORKLOADS[name].route if name in WORKLOADS else None
        if route is not None:
            plan = ctx.plan_describe()
            assert route in plan, plan
        hb, h = ctx._b, ctx._handle
        for k, pattern in enumerate(("sparse", "dense")):
            hb.check(hb.batch_rearm(h))
            _fill(torch, noise, pattern, 0xB0F + k)
            torch.cuda.synchronize()  # (torch wrote on its own stream)
            hb.check(hb.source_adopt_device(h, src.id, noise.data_ptr(), 2, FRAMES, SR))
            got, got_bins = _render(ctx, pull)
            fresh, _ = bench.build_workload(waa, hip, name, n, FRAMES, 0, noise.data_ptr())
            want, want_bins = _render(fresh, pull)
            fresh.close()
            fresh = None
            what = f"{name} ({n} contexts): the render after re-arm {k + 1} ({pattern} audio)"
            assert_same_bits(got, want, what)
            if pull:
                assert_same_bits(got_bins, want_bins, f"{name}: the analyser pull after re-arm {k + 1}", axes=("instance", "bin"))
            assert_differs(got, prev, what)
            prev = got
    finally:
        for c in (ctx, fresh):
            if c is not None:
                c.close()
        del noise
        torch.cuda.empty_cache()


# ---- a plan that holds values rendered at plan time is not re-armed (-m gpu) ----------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("modulator", ["source", "oscillator"])
@pytest.mark.parametrize("target", ["playback_rate", "detune", "position_x"])
def test_rearm_refuses_a_plan_with_values_rendered_at_plan_time(hip, target, modulator):
    """a source's playbackRate / detune or a panner's position driven from the graph is rendered when the batch is planned (one
    value per quantum and instance): new audio in a re-armed batch would render with the old audio's values, so the re-arm is an
    InvalidStateError — whether the modulator reads the refilled source or not"""
    n, frames = 4, RQ * 40 + 9

    def build(audio):
        ctx, src = modulated_graph(hip, n, frames, (target,), modulator)
        src.set_buffer_batch(audio(n, 2, frames), SR)
        return ctx

    ctx = build(dense)
    first = ctx.start_rendering_sync().data
    assert "modulated from the graph: the modulating subgraph was rendered at plan time" in ctx.plan_describe()
    donor = build(sparse)
    try:
        refill_from(ctx, donor)
    except waa.WaaError as e:
        assert e.status == 3 and "InvalidStateError" in str(e) and "rendered from the graph at plan time" in str(e), e
    else:
        got = render_again(ctx)
        want = donor.start_rendering_sync().data
        assert_same_bits(got, want, f"the re-armed render ({target} driven by the {modulator})")
        assert_differs(got, first)
        pytest.fail(f"re-armed a plan whose {target} values were rendered from the graph at plan time")
    finally:
        ctx.close()
        donor.close()


# ---- the contract's edges (-m gpu) ---------------------------------------------------------------------------------------------

def _pcm16(x):
    """[n, ch, frames] in [-1, 1) -> interleaved 16-bit PCM [n, frames, ch]"""
    return np.ascontiguousarray(np.round(np.transpose(x, (0, 2, 1)) * 32767.0).astype(np.int16))


@pytest.mark.gpu
def test_rearmed_refills_of_another_shape_or_kind_are_refused(hip):
    """after a re-arm, a source takes only buffers of the channel count, rate and kind (f32 / 16-bit PCM) it was planned with, a
    source whose buffer was set per instance takes none; the refusals change nothing, and the refills that fit then render what a
    fresh batch renders"""
    n, frames = 4, RQ * 20 + 3

    def build(a_f32, a_pcm):
        ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=n, binding=hip)
        f32 = ctx.create_buffer_source().set_buffer_batch(a_f32, SR)
        pcm = ctx.create_buffer_source().set_buffer_pcm16_batch(a_pcm, SR)
        one = ctx.create_buffer_source().set_buffer(waa.AudioBuffer(dense(1, 2, frames, seed0=9)[0], SR), instance=1)
        flt = ctx.create_biquad_filter(type_="lowpass", frequency=900.0, q=1.0)
        for s in (f32, pcm, one):
            s.connect(flt)
            s.start()
        flt.connect(ctx.destination())
        return ctx, f32, pcm, one

    ctx, f32, pcm, one = build(dense(n, 2, frames), _pcm16(dense(n, 2, frames, seed0=5)))
    first = ctx.start_rendering_sync().data
    hb, h = ctx._b, ctx._handle
    hb.check(hb.batch_rearm(h))
    b32, bpcm = other_dense(n, 2, frames), _pcm16(sparse(n, 2, frames))
    mono, mono_pcm = np.ascontiguousarray(b32[:, :1]), np.ascontiguousarray(bpcm[:, :, :1])
    i16 = ctypes.POINTER(ctypes.c_int16)
    refused = [
        ("f32, one channel", lambda: hb.source_set_buffer_batch(h, f32.id, waa.api._fp(mono), 1, frames, SR)),
        ("f32, 44.1 kHz", lambda: hb.source_set_buffer_batch(h, f32.id, waa.api._fp(b32), 2, frames, 44100.0)),
        ("f32 source, PCM", lambda: hb.source_set_buffer_pcm16_batch(h, f32.id, bpcm.ctypes.data_as(i16), 2, frames, SR)),
        ("PCM source, f32", lambda: hb.source_set_buffer_batch(h, pcm.id, waa.api._fp(b32), 2, frames, SR)),
        ("PCM, one channel", lambda: hb.source_set_buffer_pcm16_batch(h, pcm.id, mono_pcm.ctypes.data_as(i16), 1, frames, SR)),
        ("PCM, 44.1 kHz", lambda: hb.source_set_buffer_pcm16_batch(h, pcm.id, bpcm.ctypes.data_as(i16), 2, frames, 44100.0)),
        ("per-instance source, batch", lambda: hb.source_set_buffer_batch(h, one.id, waa.api._fp(b32), 2, frames, SR)),
        ("per-instance source, instance 1",
         lambda: hb.source_set_buffer(h, one.id, 1, waa.api._chan_ptrs(b32[1]), 2, frames, SR)),
    ]
    for what, call in refused:
        with pytest.raises(waa.WaaError, match="InvalidStateError") as ei:
            hb.check(call())
        assert ei.value.status == 3, what
    hb.check(hb.source_set_buffer_batch(h, f32.id, waa.api._fp(b32), 2, frames, SR))
    hb.check(hb.source_set_buffer_pcm16_batch(h, pcm.id, bpcm.ctypes.data_as(i16), 2, frames, SR))
    got = render_again(ctx)
    ctx.close()
    fresh = build(b32, bpcm)[0]
    want = fresh.start_rendering_sync().data
    fresh.close()
    assert_same_bits(got, want)
    assert_differs(got, first)


@pytest.mark.gpu
def test_rearmed_batch_keeps_the_sources_it_was_not_given(hip):
    """two batch-filled sources, only one refilled: the rest of the batch is frozen, so the render equals a fresh batch with B
    for that source and A for the other"""
    n, frames = 5, RQ * 40 + 21

    def build(a1, a2):
        ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=n, binding=hip)
        s1 = ctx.create_buffer_source().set_buffer_batch(a1, SR)
        s2 = ctx.create_buffer_source().set_buffer_batch(a2, SR)
        s1.connect(ctx.create_biquad_filter(type_="lowpass", frequency=500.0, q=2.0)).connect(ctx.destination())
        s2.connect(ctx.create_delay(0.1, delay_time=0.011)).connect(ctx.destination())
        s1.start()
        s2.start()
        return ctx, s1

    a1, a2 = dense(n, 2, frames), sparse(n, 2, frames)
    ctx, s1 = build(a1, a2)
    first = ctx.start_rendering_sync().data
    b1 = other_dense(n, 2, frames, seed0=31)
    donor, _ = build(b1, other_dense(n, 2, frames, seed0=77))  # (its second source is not taken)
    assert refill_from(ctx, donor, only={s1.id}) == 1
    got = render_again(ctx)
    ctx.close()
    donor.close()
    fresh, _ = build(b1, a2)
    want = fresh.start_rendering_sync().data
    fresh.close()
    assert_same_bits(got, want)
    assert_differs(got, first)


@pytest.mark.gpu
def test_rearmed_batch_with_suspend_points_equals_a_fresh_one(hip, orc):
    """a batch rendered through suspend ranges (a gain value and a connection made at quantum 3, as in tests/test_suspend.py),
    re-armed with B, equals a fresh batch with the same suspend script on B (and the oracle)"""
    n, nq = 4, 30

    def build(be, audio):
        ctx = waa.OfflineAudioContext(2, RQ * nq - 17, SR, n_instances=n, binding=be)
        src = ctx.create_buffer_source().set_buffer_batch(audio(n, 2, RQ * nq), SR)
        flt = ctx.create_biquad_filter(type_="lowpass", frequency=900.0, q=2.0)
        gain = ctx.create_gain(gain=0.8)
        dly = ctx.create_delay(0.5)
        dly.delay_time.set_value(0.004)
        src.connect(flt).connect(gain).connect(ctx.destination())
        src.connect(dly)
        src.start()

        def q3(c):
            gain.gain.set_value(0.25)
            dly.connect(c.destination())

        ctx.suspend_sync(3 * RQ / SR, q3)
        return ctx

    ctx = build(hip, dense)
    first = ctx.start_rendering_sync().data
    assert "1 connection(s) made or cut at suspend points" in ctx.plan_describe()
    donor = build(hip, sparse)
    assert refill_from(ctx, donor) == 1
    got = render_again(ctx)
    ctx.close()
    want = donor.start_rendering_sync().data
    donor.close()
    assert_same_bits(got, want)
    assert_differs(got, first)
    co = build(orc, sparse)
    o = co.start_rendering_sync().data
    co.close()
    assert rms_err(got, o).max() <= 1e-6  # (test_gain_and_connection_mutated_at_suspend_points_match_the_oracle's bound)


@pytest.mark.gpu
def test_rearmed_pcm16_at_another_rate_equals_a_fresh_batch(hip):
    """16-bit PCM at 44.1 kHz into a 48 kHz context (the decode and the resampler on the device), re-armed with other PCM"""
    n, frames, pcm_frames = 5, RQ * 40, 4800

    def build(pcm):
        ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=n, binding=hip)
        src = ctx.create_buffer_source().set_buffer_pcm16_batch(pcm, 44100.0)
        src.connect(ctx.create_biquad_filter(type_="highpass", frequency=300.0, q=0.7)).connect(ctx.destination())
        src.start()
        return ctx

    ctx = build(_pcm16(dense(n, 2, pcm_frames)))
    first = ctx.start_rendering_sync().data
    donor = build(_pcm16(sparse(n, 2, pcm_frames)))
    assert refill_from(ctx, donor) == 1
    got = render_again(ctx)
    ctx.close()
    want = donor.start_rendering_sync().data
    donor.close()
    assert_same_bits(got, want)
    assert_differs(got, first)
