"""AudioBufferSourceNode schedules through every reader, against the oracle.

The playhead of audio_buffer_source.rs:422-845 is restated twice — as the oracle's quantum loop and as the host replay of
waa_schedule.cpp, which turns a schedule into per-frame records (prev, next, k) — and four pieces of device code turn the records
into samples: resample_kernel (window path and gather path), the source loaders of chain_kernel, the streaming loader of the
Biquad / IIR kernels and the loader of biquad_lanes.

* CPU (marker `measure`): thousands of generated schedules (source_schedules.schedule_case) are planned on plan-only batches, the
  uploaded records are fetched (waa_debug_source_records), evaluated in numpy float64 the way the readers do and compared with the
  oracle's render: decides between the replay and the readers when a device test fails.
* GPU (marker `gpu`): the same cases through each reader; every test first proves from the profile slots which kernel ran.

Bounds.  Source only: one f32 spacing of the larger magnitude per sample — both sides round the same f64 expression once, only
fused against unfused arithmetic can move the rounding, by one step; an index error is ~1e-2 on white noise.  Behind a curve or a
filter: what the reader's older tests hold (1e-6 max and RMS for the interpreter / resample kernel, 1e-6 RMS for Biquad and IIR)."""
import numpy as np
import pytest

import web_audio_api_rs_amd as waa
from graphs import assert_all_finite, assert_le, rms_err, white_noise
from source_schedules import (FRAMES, RQ, assert_within_one_spacing, case_buffer, case_records, evaluate_records, expect_silence, make_case,
                              ran, record_kinds, schedule_case, source_graph, source_records)
from source_schedules import render as render_on

SR = 48000.0
LENGTH = RQ * 24 + 5      # 12 sub-tiles of 256 frames and a last one of 5 frames (two tiles: the second one partial)
N_SEEDS = 2500
TOL = 1e-6
ALL_KINDS = {"fast", "fast-loop", "slow next>=0", "slow next==-1", "slow next==-2", "silent"}


def check_sound(oracle_out, cases):
    """the oracle's render is not silent — per context — unless silence is the expected result"""
    for i, case in enumerate(cases):
        assert bool(oracle_out[i].any()) != expect_silence(case), (i, case)


# =========================================================================== CPU: the planner's records against the oracle
@pytest.mark.measure
def test_records_reproduce_the_oracle(hip, orc):
    """N_SEEDS generated schedules: the records the plan uploads, evaluated in float64 and rounded once, against the oracle's
    render on white noise — one f32 spacing at every sample, every value finite, every record kind reached, and silence exactly
    where the inputs say so.  (Run once over 4000 seeds: no mismatch, 3988 renders bit-identical; every case renders finite in
    the oracle.)"""
    kinds, identical = set(), 0
    for seed in range(N_SEEDS):
        case = schedule_case(seed)
        buf = case_buffer(case)
        want = render_on(orc, [case], [buf])
        check_sound(want, [case])
        rec = case_records(hip, case)
        kinds |= record_kinds(*rec)
        identical += assert_within_one_spacing(evaluate_records(rec, buf, case["length"]), want[0], f"seed {seed}: {case}")
    assert kinds == ALL_KINDS, sorted(ALL_KINDS - kinds)
    print(f"{N_SEEDS} schedules, {identical} bit-identical, record kinds {sorted(kinds)}")


def last_frame_case(**kw):
    return make_case(frames=1000, rate=-1.0, loop=True, offset=(1000 - 0.5) / SR, **kw)


@pytest.mark.measure
def test_reverse_loop_in_the_last_frame_is_a_zero_sample(hip, orc):
    """Pins a DEFINITION of this project, not the reference: a looping source played in reverse whose playhead sits in the
    buffer's last frame makes the reference index one past the buffer (audio_buffer_source.rs:795-797, a panic); oracle and
    product define the missing sample as 0.  The generator never draws this; here it is: the loop is the whole buffer, the
    offset half a frame before its end — the first output is half the last sample."""
    case = last_frame_case()
    buf = case_buffer(case)
    want = render_on(orc, [case], [buf])[0]
    rec = case_records(hip, case)
    assert (rec[1][0], rec[2][0], rec[3][0]) == (999, -1, 0.5)
    assert np.array_equal(want[:, 0], (0.5 * buf[:, 999].astype(np.float64)).astype(np.float32))
    assert_within_one_spacing(evaluate_records(rec, buf, case["length"]), want, "reverse loop from the last frame")


def _records_call(lib, ctx, node, instance):
    import ctypes as C
    nq = (ctx.length + RQ - 1) // RQ
    mode, prev, nxt, k = (C.c_uint32 * nq)(), (C.c_int64 * (nq * RQ))(), (C.c_int64 * (nq * RQ))(), (C.c_double * (nq * RQ))()
    fn = lib.lib.waa_debug_source_records
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    lib.check(fn(ctx._handle, node, instance, mode, prev, nxt, k))


@pytest.mark.measure
def test_records_are_handed_out_for_planned_sources_only(hip, hip_product):
    """the accessor hands back the host tables of a plan: it refuses a batch without a plan, a node that is no source and an
    instance the batch does not have; the product library does not export it"""
    case = make_case()
    ctx, src = source_graph(hip, [case], [case_buffer(case)], device=waa.PLAN_ONLY)
    ctx.prepare()
    with pytest.raises(waa.api.WaaError, match="no plan"):
        _records_call(hip, ctx, src.id, 0)
    source_records(hip, ctx, src)
    with pytest.raises(waa.api.WaaError, match="no source table"):
        _records_call(hip, ctx, ctx.destination().id, 0)
    with pytest.raises(waa.api.WaaError, match="instance"):
        _records_call(hip, ctx, src.id, 1)
    ctx.close()
    assert not hasattr(hip_product.lib, "waa_debug_source_records")


@pytest.mark.gpu
@pytest.mark.measure
def test_records_are_refused_on_a_device_batch(hip):
    """... and a batch with a device: its tables are device memory"""
    case = make_case(length=RQ)
    ctx, src = source_graph(hip, [case], [case_buffer(case)])
    ctx.plan_describe()
    with pytest.raises(waa.api.WaaError, match="plan-only"):
        _records_call(hip, ctx, src.id, 0)
    ctx.close()


# =========================================================================== GPU
def both(hip, orc, slot, cases, buffers, not_slot=None, adopt=None, **kw):
    """(device render, oracle render) of one batch with the same calls; the device render must have run `slot` (and not
    `not_slot`).  adopt: a resident torch tensor the device's source adopts in place of `buffers`."""
    want = render_on(orc, cases, buffers, **kw)
    ctx, src = source_graph(hip, cases, None if adopt is not None else buffers, **kw)
    if adopt is not None:
        src.adopt_device_buffer(adopt.data_ptr(), adopt.shape[1], adopt.shape[2], cases[0]["buffer_rate"])
    ctx.profile()
    got = ctx.start_rendering_sync().data
    ctx.sync()  # (folds the launches' event pairs into the profile)
    assert ran(ctx, slot) > 0, (slot, ctx.profile_entries())
    if not_slot is not None:
        assert ran(ctx, not_slot) == 0, (not_slot, ctx.profile_entries())
    ctx.close()
    check_sound(want, cases)
    return got, want


def close_behind_a_curve(got, want, what):
    assert_all_finite(got, what)
    assert_le(np.abs(got.astype(np.float64) - want).max(), TOL, what)
    assert_le(rms_err(got, want).max(), TOL, what)


def close_behind_a_filter(got, want, what):
    assert_all_finite(got, what)
    assert_le(rms_err(got, want).max(), TOL, what)


def cos_curve(n):
    i = np.arange(n, dtype=np.float32)
    return np.cos(np.float32(np.pi) + i * np.float32(np.pi) / np.float32(max(n - 1, 1))).astype(np.float32)


def shaper_tail(curve):
    return lambda ctx, src: src.connect(ctx.create_wave_shaper(curve=curve))


def subtile_spans(rec, frames):
    """per 256-frame sub-tile: the span of buffer frames resample_kernel's wave would have to hold in its window (lowest frame
    named, aligned down to 4, to the highest), 0 for a sub-tile without a live record"""
    mode, prev, nxt, _ = rec
    fmode = np.repeat(mode, RQ)
    p = prev.copy()
    p[fmode == 3] %= frames
    p[(fmode == 1) & (p >= frames)] = -1
    p[fmode == 0] = -1
    pad = (-p.size) % 256
    p, n = np.pad(p, (0, pad), constant_values=-1), np.pad(nxt, (0, pad), constant_values=-1)
    spans = []
    for s in range(p.size // 256):
        ps, ns = p[s * 256:(s + 1) * 256], n[s * 256:(s + 1) * 256]
        live = ps >= 0
        if not live.any():
            spans.append(0)
            continue
        a = np.where(ns == -2, ps - 1, ps)[live]
        b = np.where(ns >= 0, ns, ps)[live]
        lo, hi = min(a.min(), b.min()), max(a.max(), b.max(), ps[live].max())
        spans.append(int(hi - (lo & ~3) + 1))
    return spans


RATES_A = ["foreign", 0.0, 1e-3, 0.37, 0.999, 1.0, 1.5, 1.96, 1.98, 1.99, 2.0, 2.01, 3.25, 8.0]
WCAP = 512


def shared_case(rate, reverse, channels, frames=5001):
    """part a: a looping source (forward: the whole buffer; reverse: up to the last frame but one, started in the middle)"""
    buffer_rate = 38000.0 if rate == "foreign" else SR
    rate = 1.0 if rate == "foreign" else rate
    if reverse:
        end = (frames - 1) / buffer_rate
        return make_case(frames=frames, channels=channels, buffer_rate=buffer_rate, rate=-rate, loop=True, loop_end=end, offset=0.5 * end, length=LENGTH)
    return make_case(frames=frames, channels=channels, buffer_rate=buffer_rate, rate=rate, loop=True, length=LENGTH)


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("curve", [False, True])
def test_resample_kernel_shared_schedule(hip, hip_measure, orc, curve, channels):
    """resample_kernel (slot asserted; chain_kernel must not run), one schedule for all contexts: every rate of the list forward
    and in reverse, on per-context buffers and on one shared AudioBuffer, 1 / 7 / 8 / 9 / 19 contexts in turn (one partial group,
    one full, a partial one behind full ones), mono and stereo, with and without the 2048-point curve.  The 5001-frame buffer
    (frames % 4 == 1) wraps inside the render at rates from 1.96 on, and the render's last sub-tile holds 5 frames: for the
    rates 1.96 .. 2.01 the spans of a plan-only twin's records show sub-tiles on both sides of the window's 512 frames.
    Without the curve every render was bit-identical to the oracle on the MI355X: asserted."""
    combos = [(r, rev, sh) for r in RATES_A for rev in (False, True) for sh in (False, True) if not (rev and r == 0.0)]
    tail = shaper_tail(cos_curve(2048)) if curve else None
    for idx, (rate, reverse, share) in enumerate(combos):
        n = [1, 7, 8, 9, 19][idx % 5]
        case = shared_case(rate, reverse, channels)
        noise = white_noise(n, channels, case["frames"], first=idx)
        buffers = waa.AudioBuffer(noise[0], case["buffer_rate"]) if share else noise
        if rate in (1.96, 1.98, 1.99, 2.0, 2.01) and not share:
            spans = [s for s in subtile_spans(case_records(hip_measure, case), case["frames"]) if s > 0]
            assert min(spans) <= WCAP < max(spans), (rate, reverse, spans)
        got, want = both(hip, orc, "resample_kernel", [case] * n, buffers, not_slot="chain_kernel", tail=tail)
        what = f"rate {rate} reverse {reverse} shared buffer {share} n {n}"
        if curve:
            close_behind_a_curve(got, want, what)
        else:
            assert_within_one_spacing(got, want, what)
            assert np.array_equal(got, want), what


MIXED = {
    "A": dict(frames=4999, rate=1.5, loop=True),
    "B": dict(frames=5003, rate=0.37, loop=True, loop_start=1000.37 / SR, loop_end=1003.87 / SR, offset=500.0 / SR, when=(RQ + 37.25) / SR),
    "C": dict(frames=257, rate=-1.0, loop=True, loop_start=10.0 / SR, loop_end=200.5 / SR, offset=100.0 / SR, when=1.5 / SR),
}


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,channels", [("AB" * 9 + "A", 2), ("A" * 8 + "B" * 3 + "C" * 8, 2), ("A" * 8 + "B" * 3 + "C" * 8, 1)])
def test_resample_kernel_mixed_schedules_within_a_group(hip, orc, pattern, channels):
    """resample_kernel (slot asserted), 19 contexts whose rate, loop points, offset, `when` and buffer length differ per context:
    A B A B ... (every group reloads its records context by context) and A x 8, B x 3, C x 8 (the first group is uniform and
    takes the window path, the second changes schedule twice, the third starts inside a run of C).  B loops over 3.5 frames
    between frames from a start in the second quantum, C is a reverse loop on a 257-frame buffer.  Bit-identical on the MI355X."""
    protos = {k: make_case(channels=channels, length=LENGTH, **v) for k, v in MIXED.items()}
    cases = [protos[k] for k in pattern]
    buffers = [white_noise(1, channels, c["frames"], first=100 + i)[0] for i, c in enumerate(cases)]
    got, want = both(hip, orc, "resample_kernel", cases, buffers, not_slot="chain_kernel")
    assert_within_one_spacing(got, want, pattern)
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("loop", [False, True])
def test_resample_kernel_buffer_ends_and_tiny_buffers(hip, orc, loop):
    """resample_kernel (slot asserted), 9 contexts, buffers of every length of the generator's list (1 .. 5 frames, lengths on
    both sides of a 256-frame sub-tile, frames % 4 of 1, 2, 3) at the rates 0.37, 1.5 and -1.0.  Not looping: the offset puts
    the buffer's end (reverse: its start) inside the render, so the extrapolated record and the silence behind it fall inside a
    sub-tile.  Looping: short buffers wrap many times per wave (reverse loops from three frames on: they end a frame early).
    Bit-identical on the MI355X."""
    for frames in FRAMES:
        for rate in (0.37, 1.5, -1.0):
            dur = frames / SR
            if not loop:
                offset = max(0.0, dur - 1500.3 * rate / SR) if rate > 0 else min(dur - 0.5 / SR, 1500.3 / SR)
                case = make_case(frames=frames, rate=rate, offset=offset, when=1.5 / SR, length=LENGTH)
            elif rate > 0:
                case = make_case(frames=frames, rate=rate, loop=True, length=LENGTH)
            elif frames >= 3:
                end = (frames - 1) / SR
                case = make_case(frames=frames, rate=rate, loop=True, loop_end=end, offset=0.5 * end, length=LENGTH)
            else:
                continue
            got, want = both(hip, orc, "resample_kernel", [case] * 9, white_noise(9, 2, frames, first=frames), not_slot="chain_kernel")
            what = f"{frames} frames at rate {rate}, loop {loop}"
            assert_within_one_spacing(got, want, what)
            assert np.array_equal(got, want), what


@pytest.mark.gpu
def test_reverse_loop_in_the_last_frame_on_the_device(hip, orc):
    """the product-defined 0 sample (see test_reverse_loop_in_the_last_frame_is_a_zero_sample: a definition, not the reference)
    through resample_kernel, 9 contexts"""
    case = last_frame_case()
    got, want = both(hip, orc, "resample_kernel", [case] * 9, white_noise(9, 2, case["frames"]), not_slot="chain_kernel")
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("rate,loop", [(1.5, True), (1.0, False)])
def test_resample_kernel_unaligned_adopted_buffer(hip, orc, rate, loop):
    """resample_kernel (slot asserted) on ONE adopted device array of 5 x 2 x 4097 frames: the channel stride is the frame count,
    frames % 4 == 1, so every second row starts off a 16-byte boundary and no vector load may be used.  Rate 1.5 looping; rate
    1.0 not looping (the fast track, whose contiguous-tile path needs alignment too).  Bit-identical on the MI355X."""
    import torch
    n, frames = 5, 4097
    noise = white_noise(n, 2, frames, first=40)
    resident = torch.from_numpy(noise).cuda()
    case = make_case(frames=frames, rate=rate, loop=loop, length=LENGTH)
    got, want = both(hip, orc, "resample_kernel", [case] * n, noise, not_slot="chain_kernel", adopt=resident)
    del resident
    assert_within_one_spacing(got, want, f"rate {rate}")
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [1, 2, 3, 2047, 8192, 8193])
def test_curve_sizes(hip, orc, size):
    """WaveShaper curves of 1, 2, 3, 2047 and 8192 points in resample_kernel's LDS copy, 8193 points on the interpreter
    (chain_kernel: slots asserted both ways); 9 contexts, rate 1.5 looping, stereo"""
    case = make_case(frames=4999, rate=1.5, loop=True, length=LENGTH)
    curve = cos_curve(size) if size > 1 else np.array([0.25], np.float32)
    slot, other = ("resample_kernel", "chain_kernel") if size <= 8192 else ("chain_kernel<2>", "resample_kernel")
    got, want = both(hip, orc, slot, [case] * 9, white_noise(9, 2, case["frames"], first=size), not_slot=other, tail=shaper_tail(curve))
    close_behind_a_curve(got, want, f"curve of {size} points")


@pytest.mark.gpu
def test_curve_clamps_on_extrapolated_samples(hip, orc):
    """A source that is not looping extrapolates behind its last frame (2 * prev - the frame before, audio_buffer_source.rs:
    806-816): with the last two frames at -0.9, 0.95 (channel 0) and 0.9, -0.95 (channel 1) the samples in front of the curve
    leave [-1, 1] on both sides (checked on the oracle without the curve) and both clamps of the curve are hit (its end
    values, chosen distinct, appear in the render).  resample_kernel, slot asserted; 9 contexts, rate 0.37."""
    frames = 1000
    case = make_case(frames=frames, rate=0.37, offset=(frames - 300) / SR, length=LENGTH)
    noise = white_noise(9, 2, frames, first=70)
    noise[:, 0, -2:] = (-0.9, 0.95)
    noise[:, 1, -2:] = (0.9, -0.95)
    bare = render_on(orc, [case] * 9, noise)
    assert bare[:, 0].max() > 1.5 and bare[:, 1].min() < -1.5
    curve = np.linspace(-0.8, 0.6, 257).astype(np.float32)
    got, want = both(hip, orc, "resample_kernel", [case] * 9, noise, not_slot="chain_kernel", tail=shaper_tail(curve))
    assert (want[:, 0] == curve[-1]).any() and (want[:, 1] == curve[0]).any()
    close_behind_a_curve(got, want, "clamped curve")


def gain_tail(ctx, src):
    return src.connect(ctx.create_gain(gain=0.7))


def biquad_tail(ctx, src):
    return src.connect(ctx.create_biquad_filter(type_="lowpass", frequency=900.0, q=1.0)).connect(ctx.create_gain(gain=0.5))


def iir_tail(ctx, src):
    return src.connect(ctx.create_iir_filter([0.2, 0.3, 0.1], [1.0, -0.5, 0.2]))


def lanes_tail(ctx, src):
    flt = ctx.create_biquad_filter(type_="peaking", frequency=900.0, q=2.0, gain=4.0)
    flt.frequency.set_value_at_time(200.0, 0.0)
    flt.frequency.exponential_ramp_to_value_at_time(6000.0, ctx.length / ctx.sample_rate)
    return src.connect(flt)


LOADERS = {
    # name: (tail, channels (None: drawn), slot that must run, slot that must not, comparison)
    "interpreter": (gain_tail, None, "chain_kernel", "resample_kernel", close_behind_a_curve),
    "interpreter-4ch": (None, 4, "chain_kernel<4+>", "resample_kernel", assert_within_one_spacing),
    "biquad-stream": (biquad_tail, None, "biquad_stream_kernel", "chain_kernel", close_behind_a_filter),
    "iir-stream": (iir_tail, None, "iir_stream_kernel", "chain_kernel", close_behind_a_filter),
    "biquad-lanes": (lanes_tail, None, "biquad_lanes_kernel", "chain_kernel", close_behind_a_filter),
}


@pytest.mark.gpu
@pytest.mark.parametrize("loader", sorted(LOADERS))
def test_generated_schedules_through_the_other_loaders(hip, orc, loader):
    """40 seeds of the generator, 9 contexts each — one schedule for all in the even seeds, nine schedules (and nine buffer
    lengths) in the odd ones — through source -> Gain(0.7) (chain_kernel's sub-tile loader), a 4-channel source -> destination
    (chain_kernel<4+>'s tile loader), source -> Biquad(constant) -> Gain (the streaming loader), source -> IIR (the same loader
    in the IIR kernel) and source -> Biquad with a per-frame frequency (biquad_lanes' loader); the slot is asserted per render."""
    tail, channels, slot, not_slot, compare = LOADERS[loader]
    for seed in range(40):
        first = schedule_case(9000 + seed, channels=channels)
        if seed % 2:
            cases = [first] + [schedule_case(9000 + 100 * seed + j, length=first["length"], channels=first["channels"], sr=first["sr"]) for j in range(1, 9)]
        else:
            cases = [first] * 9
        buffers = [case_buffer(c, i) for i, c in enumerate(cases)]
        got, want = both(hip, orc, slot, cases, buffers, not_slot=not_slot, tail=tail)
        compare(got, want, f"{loader} seed {seed}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["blocks", "ramp"])
def test_resample_kernel_rate_automation(hip, orc, form):
    """playbackRate per quantum on 9 contexts (resample_kernel, slot asserted): value blocks that jump between rates on both
    sides of the window's capacity (and through 0), and a linear ramp 0.5 -> 2.5 that crosses it mid-render.
    An automated source has one schedule per context: the group of 8 reloads its records per context, the ninth context is a
    group of its own and takes the window path while the span allows.  Bit-identical on the MI355X."""
    case = make_case(frames=5001, rate=1.0, loop=True, length=LENGTH)
    nq = (LENGTH + RQ - 1) // RQ

    def setup(ctx, src):
        if form == "blocks":
            src.playback_rate.set_block(0, np.array([0.5, 1.99, 2.01, 1.0, 0.0, 1.5, 3.25, 1.98] * 4, np.float32)[:nq])
        else:
            src.playback_rate.set_value_at_time(0.5, 0.0)
            src.playback_rate.linear_ramp_to_value_at_time(2.5, LENGTH / SR)

    got, want = both(hip, orc, "resample_kernel", [case] * 9, white_noise(9, 2, case["frames"], first=90), not_slot="chain_kernel", setup=setup)
    assert_within_one_spacing(got, want, form)
    assert np.array_equal(got, want)
