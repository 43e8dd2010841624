"""The launch list the planner hands to the executor, step by step, for a corpus of graphs that reaches every StepKind and
every loop form: kind, loop group, quantum-block group, prologue flag, the echo fusions' marks, profile slots, the groups'
block sizes (WAA_PLAN_LAUNCHES=1, measurement build) behind the plan's own text.  The expected texts under
tests/golden/launch_lists/ were written by the planner as it was before its kinds had names (Step::kind a bare int) with the
same dump patched in, so any refactor of the planner's kind handling has to reproduce them to the byte.  Plan-only batches, no
GPU — except the one kind a plan-only batch cannot reach (Timeline: automation is replayed on the device only when there is
one), whose graph is planned on the GPU."""
import hashlib
import os
import re

import numpy as np
import pytest

import web_audio_api_rs_amd as waa
from graphs import c2, c4, c5, garage_like_ir, t1, white_noise
from test_fuzz_graphs import build_random_graph

pytestmark = pytest.mark.measure
RQ, SR = 128, 48000.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_lists")
# waa_host.hpp, enum StepKind
KIND_NAMES = ["chain", "biquad_stream", "conv_fft", "zero_fill", "conv_direct", "biquad_coefs", "iir_stream", "delay", "loop", "osc",
              "dyn", "conv_codes", "biquad_hp", "panner_geom", "timeline", "link", "qgemm", "hrtf", "biquad_tile_digest",
              "biquad_lanes", "os_fft", "compressor", "route"]
CURVE = np.tanh(np.linspace(-2.5, 2.5, 129)).astype(np.float32)


def _ctx(be, n=3, frames=2048 * 8, n_out=2, device=waa.PLAN_ONLY):
    return waa.OfflineAudioContext(n_out, frames, SR, n_instances=n, binding=be, device=device)


def _source(c, n_ch=2, frames=None, seed0=0xA0D10, scale=1.0):
    s = c.create_buffer_source()
    s.set_buffer_batch(white_noise(c.n_instances, n_ch, frames or c.length, seed0=seed0) * np.float32(scale), SR)
    s.start()
    return s


def _decaying_ir(n_ch, taps, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (n_ch, taps)) * np.exp(-np.arange(taps) / (0.3 * taps))[None, :]).astype(np.float32)


# ---- the graphs (each builder: binding -> context) ----------------------------------------------------------------------
def g_c2(be):
    return c2(be, white_noise(3, 2, 480000), device=waa.PLAN_ONLY)[0]


def g_t1(be):
    return t1(be, white_noise(5, 2, 480000), garage_like_ir(), device=waa.PLAN_ONLY)[0]


def g_c4(be):
    return c4(be, white_noise(5, 2, 480000), garage_like_ir(), device=waa.PLAN_ONLY)[0]


def g_c5(be):
    ctx = c5(be, white_noise(2, 2, 5000), length=RQ * 50)[0]
    ctx.device = waa.PLAN_ONLY
    return ctx


def _echo_loop(be, delay_time, shaper=False, **kw):
    """source -> Delay <-> [WaveShaper ->] Gain, the delay into the destination (kw: n / frames / device of the batch, as for every
    builder below that takes it — tests/test_batch_sizes.py renders them at other batch sizes)"""
    c = _ctx(be, **kw)
    s = _source(c)
    d = c.create_delay(1.0, delay_time=delay_time)
    s.connect(d)
    head = d.connect(c.create_wave_shaper(curve=np.float32([-1.0, 0.0, 1.0]))) if shaper else d
    head.connect(c.create_gain(gain=0.5)).connect(d)
    d.connect(c.destination())
    return c


def g_echo_ring(be, **kw):      # block-scheduled (2400 frames > a tile), one launch of the LDS-ring kernel
    return _echo_loop(be, 0.05, **kw)


def g_echo_ring_tail(be):       # ... whose line has one reader, dry + wet: the fused tail
    c = _ctx(be)
    s = _source(c)
    d = c.create_delay(1.0, delay_time=0.05)
    s.connect(d)
    d.connect(c.create_gain(gain=0.5)).connect(d)
    d.connect(c.destination())
    s.connect(c.destination())
    return c


def g_loop_kernel(be, **kw):    # 132 frames: below the ring kernel's smallest chunk
    return _echo_loop(be, 0.00275, **kw)


def g_loop_kernel_shaper(be):   # 480 frames around a WaveShaper: planned for the ring, does not qualify, planned again
    return _echo_loop(be, 0.01, shaper=True)


def g_two_block_loops(be):      # two block-scheduled loops in a row: an echo on the ring kernel, then one around a WaveShaper
    c = _ctx(be)
    s = _source(c)
    d1, d2 = c.create_delay(1.0, delay_time=0.05), c.create_delay(1.0, delay_time=0.06)
    s.connect(d1)
    d1.connect(c.create_gain(gain=0.5)).connect(d1)
    d1.connect(d2)
    d2.connect(c.create_wave_shaper(curve=np.float32([-1.0, 0.0, 1.0]))).connect(c.create_gain(gain=0.4)).connect(d2)
    d2.connect(c.destination())
    return c


def g_block_loop_automated(be):
    """a block-scheduled loop whose Biquad is a-rate automated and whose gain is modulated from outside the loop: coefficient
    tables, digests and the param's summing chain run once in front of the blocks"""
    c = _ctx(be)
    s = _source(c)
    d = c.create_delay(1.0, delay_time=0.05)
    bq = c.create_biquad_filter(type_="bandpass", frequency=800.0, q=1.5)
    bq.frequency.set_value_at_time(300.0, 0.0).exponential_ramp_to_value_at_time(4000.0, 0.3)
    g = c.create_gain(gain=0.35)
    lfo = c.create_oscillator(type_="sine", frequency=7.0)
    lfo.connect(c.create_gain(gain=0.1)).connect(g.gain)
    lfo.start()
    s.connect(d)
    d.connect(bq).connect(g).connect(d)
    bq.connect(c.destination())
    return c


def g_filtered_echo_tail(be):
    """source -> Delay -> Biquad -> Gain -> back, filter + source into the destination (tests/test_cycles.py): the ring kernel's
    BQ form with the tail fused"""
    n, frames = 6, 2048 * 11 + 77
    c = _ctx(be, n=n, frames=frames)
    s = _source(c, seed0=37)
    delay, bq, fb = c.create_delay(0.4), c.create_biquad_filter(type_="lowpass", frequency=2500.0), c.create_gain()
    delays = (np.float64([2064, 2065.5, 3000.25, 4800, 9000.75, 14328]) / 48000.0).astype(np.float32)
    gains = np.float32([0.5, -0.7, 0.9, 0.3, 0.6, -0.95])
    for i in range(n):
        delay.delay_time.set_value(delays[i], instance=i)
        fb.gain.set_value(gains[i], instance=i)
    s.connect(delay)
    delay.connect(bq).connect(fb).connect(delay)
    bq.connect(c.destination())
    s.connect(c.destination())
    return c


def g_feed_forward_echo(be):    # 256 contexts: one per CU, the ring kernel with nothing fed back
    c = _ctx(be, n=256, frames=2048 * 2)
    s = c.create_buffer_source()
    s.set_buffer_batch(np.zeros((256, 1, 2048 * 2), np.float32), SR)
    s.start()
    s.connect(c.destination())
    s.connect(c.create_delay(0.4, delay_time=0.1)).connect(c.create_gain(gain=0.5)).connect(c.destination())
    return c


def g_delay_gather(be, **kw):   # a delay in front of a convolver keeps the gather kernel
    c = _ctx(be, **kw)
    s = _source(c)
    d = c.create_delay(1.0, delay_time=0.05)
    s.connect(d).connect(c.create_convolver(buffer=waa.AudioBuffer(np.ones((1, 300), np.float32), SR))).connect(c.destination())
    return c


def _frozen_loop(be, kind, delay_time, **kw):
    """a burst -> Delay -> oversampled WaveShaper / HRTF panner -> Gain -> back (tests/test_frozen_loops.py): dynamic counts, the
    loop cut at the node and launched quantum block by quantum block"""
    c = _ctx(be, **{"frames": RQ * 70 + 33, **kw})
    n = c.n_instances
    s = c.create_buffer_source()
    s.set_buffer_batch(white_noise(n, 2, RQ * 20 + 7, seed0=5) * np.float32(0.6), SR)
    d = c.create_delay(0.1, delay_time=delay_time)
    f = (c.create_panner(panning_model="HRTF", position=(0.8, 0.3, -0.6)) if kind == "hrtf"
         else c.create_wave_shaper(curve=CURVE, oversample=kind))
    s.connect(d)
    d.connect(f).connect(c.create_gain(gain=0.45)).connect(d)
    f.connect(c.destination())
    for i in range(n):
        s.start_at((i % 14) * 211.0 / SR, instance=i)
    return c


def g_qloop_shaper_2x(be, **kw):
    return _frozen_loop(be, "2x", 0.01, **kw)


def g_qloop_hrtf(be, **kw):
    return _frozen_loop(be, "hrtf", 0.01, **kw)


def g_qloop_automated(be):
    """... with an a-rate delayTime, an automated Biquad and a gain modulated from outside: their launches run once in front of
    the quantum blocks"""
    n, frames = 3, RQ * 70 + 33
    c = _ctx(be, n=n, frames=frames)
    s = _source(c, frames=RQ * 40, seed0=21, scale=0.5)
    d = c.create_delay(0.05, delay_time=0.01)
    d.delay_time.set_value_at_time(0.004, 0.0).linear_ramp_to_value_at_time(0.03, frames / SR)
    sh = c.create_wave_shaper(curve=CURVE, oversample="2x")
    bq = c.create_biquad_filter(type_="bandpass", frequency=800.0, q=1.5)
    bq.frequency.set_value_at_time(300.0, 0.0).exponential_ramp_to_value_at_time(4000.0, frames / SR)
    g = c.create_gain(gain=0.35)
    lfo = c.create_oscillator(type_="sine", frequency=7.0)
    lfo.connect(c.create_gain(gain=0.1)).connect(g.gain)
    lfo.start()
    s.connect(d)
    d.connect(sh).connect(bq).connect(g).connect(d)
    bq.connect(c.destination())
    return c


def g_qloop_conv_and_shaper(be, **kw):
    c = _ctx(be, **{"frames": RQ * 70 + 33, **kw})
    s = _source(c, frames=RQ * 30, seed0=33, scale=0.4)
    d = c.create_delay(0.1, delay_time=0.005)
    cv = c.create_convolver(buffer=waa.AudioBuffer(_decaying_ir(2, 300, 7), SR))
    sh = c.create_wave_shaper(curve=CURVE, oversample="2x")
    s.connect(d)
    d.connect(cv).connect(sh).connect(c.create_gain(gain=0.25)).connect(d)
    sh.connect(c.destination())
    return c


def g_qloop_long_conv_refused(be):  # partitions that span several quanta in a short loop: status 4
    c = _ctx(be, n=1, frames=RQ * 70 + 33)
    s = _source(c, frames=RQ * 9 + 3)
    d = c.create_delay(0.1, delay_time=0.003)
    cv = c.create_convolver(buffer=waa.AudioBuffer(_decaying_ir(2, 5000, 1), SR))
    s.connect(d)
    d.connect(cv).connect(c.create_gain(gain=0.3)).connect(d)
    cv.connect(c.destination())
    return c


def g_oversampled_shaper(be, **kw):  # outside any loop, static counts: the transform form in one launch (under WAA_OS_MATRIX: two qgemm stages)
    c = _ctx(be, **{"frames": RQ * 40, **kw})
    _source(c).connect(c.create_wave_shaper(curve=CURVE, oversample="4x")).connect(c.destination())
    return c


def g_listener_automated_in_a_loop(be, **kw):  # ... the panner inside a block-scheduled loop: the geometry runs once in front of the blocks
    c = _ctx(be, **kw)
    c.listener().position_x.set_value_at_time(0.0, 0.0).linear_ramp_to_value_at_time(1.0, 0.3)
    s = _source(c)
    d = c.create_delay(1.0, delay_time=0.05)
    s.connect(d)
    d.connect(c.create_panner(panning_model="equalpower", position=(1.0, 0.0, -1.0))).connect(c.create_gain(gain=0.4)).connect(d)
    d.connect(c.destination())
    return c


def g_biquad_k_rate(be):
    ctx, nodes = c2(be, white_noise(1, 2, RQ * 20), device=waa.PLAN_ONLY)
    nodes["biquad"].frequency.set_block(0, np.linspace(100, 1000, 20).astype(np.float32))
    return ctx


def g_biquad_a_rate_shared(be):  # one shared coefficient table: coefs, hp digest, tile digests, lanes
    ctx, nodes = c2(be, white_noise(3, 2, 2048 * 3 + 50), device=waa.PLAN_ONLY)
    nodes["biquad"].frequency.set_value_at_time(10.0, 0.0).exponential_ramp_to_value_at_time(10000.0, 0.05)
    return ctx


def g_iir(be, **kw):
    c = _ctx(be, **{"frames": RQ * 64, **kw})
    _source(c).connect(c.create_iir_filter([0.2, 0.3, 0.1], [1.0, -0.5, 0.2])).connect(c.destination())
    return c


def g_fm_pair(be, **kw):
    c = _ctx(be, **{"frames": RQ * 40, **kw})
    mod, idx, car = c.create_oscillator(type_="sine", frequency=110.0), c.create_gain(gain=300.0), c.create_oscillator(type_="sine", frequency=440.0)
    for i in range(c.n_instances):
        car.detune.set_value(25.0 * (i % 14), instance=i)
    mod.connect(idx).connect(car.frequency)
    car.connect(c.destination())
    mod.start()
    car.start_at(0.001)
    return c


def g_compressor(be, **kw):
    c = _ctx(be, **{"n": 2, "frames": RQ * 64, **kw})
    _source(c).connect(c.create_dynamics_compressor()).connect(c.destination())
    return c


def g_compressor_behind_an_echo_loop(be):  # a kind the echo-tail fusion does not know: the fusion leaves the whole plan alone
    c = _ctx(be)
    s = _source(c)
    d = c.create_delay(1.0, delay_time=0.05)
    s.connect(d)
    d.connect(c.create_gain(gain=0.5)).connect(d)
    mix = c.create_gain(gain=1.0)
    d.connect(mix)
    s.connect(mix)
    mix.connect(c.create_dynamics_compressor()).connect(c.destination())
    return c


def g_splitter_merger(be, **kw):  # swap the channels: splitter -> merger
    c = _ctx(be, **{"frames": RQ * 30, **kw})
    s = _source(c)
    sp, mg = c.create_channel_splitter(2), c.create_channel_merger(2)
    s.connect(sp)
    sp.connect(mg, 0, 1)
    sp.connect(c.create_gain(gain=0.5), 1).connect(mg, 0, 0)
    mg.connect(c.destination())
    return c


def g_merger_behind_an_echo_loop(be):
    c = _ctx(be)
    s = _source(c, n_ch=1)
    d = c.create_delay(1.0, delay_time=0.05)
    s.connect(d)
    d.connect(c.create_gain(gain=0.5)).connect(d)
    mg = c.create_channel_merger(2)
    d.connect(mg, 0, 0)
    s.connect(mg, 0, 1)
    mg.connect(c.destination())
    return c


def _per_instance_conv(be, taps, **kw):
    c = _ctx(be, **{"frames": RQ * 40, **kw})
    conv = c.create_convolver()
    conv.set_buffer_batch(np.stack([_decaying_ir(2, taps, 100 + 7 * (i % 14)) for i in range(c.n_instances)]), SR)
    _source(c).connect(conv).connect(c.destination())
    return c


def g_per_instance_conv_direct(be, **kw):
    return _per_instance_conv(be, 100, **kw)


def g_per_instance_conv_fft(be, **kw):
    return _per_instance_conv(be, 1500, **kw)


def g_block_loop_zero_conv(be, **kw):  # the fill inside a block-scheduled loop: once in front of the blocks
    c = _ctx(be, **{"frames": 2048 * 6, **kw})
    s = _source(c)
    d = c.create_delay(0.1, delay_time=0.06)
    cv = c.create_convolver(buffer=waa.AudioBuffer(np.zeros((2, 64), np.float32), SR))
    s.connect(d)
    d.connect(cv).connect(c.create_gain(gain=0.3)).connect(d)
    d.connect(c.destination())
    return c


def g_misordered_refused(be):   # (with WAA_DEBUG_REVERSE_PLAN: the validator's refusal and its message)
    c = _ctx(be, n=2, frames=RQ * 40)
    s = _source(c)
    conv = c.create_convolver(buffer=waa.AudioBuffer(white_noise(1, 2, 300)[0], SR))
    s.connect(c.create_biquad_filter(type_="lowpass", frequency=500.0)).connect(conv).connect(c.create_stereo_panner(pan=0.3)).connect(c.destination())
    return c


def g_timeline(be, device=waa.PLAN_ONLY, **kw):
    """a gain with another automation per context: replayed on the device where there is one (StepKind::Timeline), evaluated on
    the host by a plan-only batch"""
    c = _ctx(be, **{"frames": RQ * 40, **kw}, device=device)
    g = c.create_gain(gain=0.5)
    for i in range(c.n_instances):
        k = i % 14
        g.gain.set_value_at_time(0.1 * (k + 1), 0.0, instance=i).linear_ramp_to_value_at_time(1.0, 0.05 + 0.01 * k, instance=i)
    _source(c).connect(g).connect(c.destination())
    return c


# name -> (builder, measurement switches on top of WAA_PLAN_LAUNCHES)
NAMED = {
    "c2": (g_c2, {}), "t1": (g_t1, {}), "c4": (g_c4, {}), "c5": (g_c5, {}),
    "echo_ring": (g_echo_ring, {}), "echo_ring_tail": (g_echo_ring_tail, {}),
    "loop_kernel": (g_loop_kernel, {}), "loop_kernel_shaper": (g_loop_kernel_shaper, {}),
    "two_block_loops": (g_two_block_loops, {}), "block_loop_automated": (g_block_loop_automated, {}),
    "block_loop_zero_conv": (g_block_loop_zero_conv, {}), "listener_automated_in_a_loop": (g_listener_automated_in_a_loop, {}),
    "filtered_echo_tail": (g_filtered_echo_tail, {}), "feed_forward_echo": (g_feed_forward_echo, {}), "delay_gather": (g_delay_gather, {}),
    "qloop_shaper_2x": (g_qloop_shaper_2x, {}), "qloop_hrtf": (g_qloop_hrtf, {}), "qloop_automated": (g_qloop_automated, {}),
    "qloop_conv_and_shaper": (g_qloop_conv_and_shaper, {}),
    "qloop_long_conv_refused": (g_qloop_long_conv_refused, {}), "frozen_loop_refused": (g_qloop_shaper_2x, {"WAA_NO_FROZEN_LOOPS": "1"}),
    "oversampled_shaper_matrix": (g_oversampled_shaper, {"WAA_OS_MATRIX": "1"}),
    "biquad_k_rate": (g_biquad_k_rate, {}), "biquad_a_rate_shared": (g_biquad_a_rate_shared, {}), "iir": (g_iir, {}),
    "fm_pair": (g_fm_pair, {}),
    "compressor": (g_compressor, {}), "compressor_behind_an_echo_loop": (g_compressor_behind_an_echo_loop, {}),
    "splitter_merger": (g_splitter_merger, {}), "merger_behind_an_echo_loop": (g_merger_behind_an_echo_loop, {}),
    "per_instance_conv_direct": (g_per_instance_conv_direct, {}), "per_instance_conv_fft": (g_per_instance_conv_fft, {}),
}


# ---- one small graph per planner branch that no graph above reaches (branches.txt) -----------------------------------------
def g_frozen_fan_in(be):        # an oversampled WaveShaper that sums two sources: its codes come out of the dynamic-count rendering
    c = _ctx(be)
    sh = c.create_wave_shaper(curve=CURVE, oversample="2x")
    _source(c).connect(sh)
    _source(c, seed0=7).connect(sh)
    sh.connect(c.destination())
    return c


def g_merger_falls_back(be):    # tests/test_channel_routing.py: both inputs of a merger in front of a panner stop mid-render
    c = _ctx(be)
    mg, pan = c.create_channel_merger(2), c.create_panner()
    for k in range(2):
        s = _source(c, n_ch=1, seed0=10 + k)
        s.stop_at(0.05)
        s.connect(mg, 0, k)
    mg.connect(pan).connect(c.destination())
    return c


def g_mono_shaper_into_a_wide_downmix(be):
    """a 5.1 source that ends early -> WaveShaper with curve(0) != 0 -> stereo destination (tests/test_wide_channels.py, fuzz seed
    293): behind the source's end the shaper renders one channel where the static plan has six, into the 5.1 -> stereo matrix"""
    c = _ctx(be)
    _source(c, n_ch=6, frames=RQ * 20).connect(c.create_wave_shaper(curve=np.float32([0.5, 0.5, 0.5]))).connect(c.destination())
    return c


def g_bus_grows_input_by_input(be):
    """stereo (ends early), mono and 5.1 into one bus: with the stereo source the mono one reaches 5.1 through stereo (L and R),
    without it directly (C)"""
    c = _ctx(be)
    bus = c.create_gain(gain=0.7)
    _source(c, n_ch=6, seed0=3).connect(bus)   # (summed in processing order: the source made last comes first)
    _source(c, n_ch=1, seed0=2).connect(bus)
    _source(c, n_ch=2, frames=RQ * 20, seed0=1).connect(bus)
    bus.connect(c.destination())
    return c


def g_muted_cycle(be):          # tests/test_cycles.py: gain <-> gain without a DelayNode, the other source still renders
    c = _ctx(be)
    g1, g2 = c.create_gain(gain=0.5), c.create_gain(gain=0.5)
    _source(c).connect(g1).connect(g2).connect(g1)
    g2.connect(c.destination())
    _source(c, seed0=3).connect(c.destination())
    return c


def g_short_echo_ring(be):      # 480 frames, shorter than a tile: planned for the ring kernel, and it qualifies
    return _echo_loop(be, 0.01)


def g_biquad_in_the_forward_transform(be):  # tests/test_plan.py: per-context coefficients cannot go into the one impulse response
    ctx, nodes = t1(be, white_noise(3, 2, 480000), garage_like_ir(), device=waa.PLAN_ONLY, biquad_handle=True)
    nodes["biquad"].frequency.set_value(300.0, instance=2)
    return ctx


def g_zero_gain_silent_modulator_refused(be):  # a gain of 0 whose modulator starts late: the reference emits the silent block
    c = _ctx(be)
    g = c.create_gain(gain=0.0)
    lfo = c.create_oscillator(type_="sine", frequency=7.0)
    lfo.connect(g.gain)
    lfo.start_at(0.1)
    _source(c).connect(g).connect(c.destination())
    return c


def g_mixed_buffer_widths(be):  # tests/test_dynamic_counts.py: mono, stereo and quad AudioBuffers on the three contexts
    c = _ctx(be)
    s = c.create_buffer_source()
    for i, n_ch in enumerate((1, 2, 4)):
        s.set_buffer(waa.AudioBuffer(white_noise(1, n_ch, c.length // 2 + 17 * i, seed0=70 + i)[0] * np.float32(0.5), SR), instance=i)
    s.start_at(130.0 / SR)
    s.connect(c.create_stereo_panner(pan=0.2)).connect(c.destination())
    return c


def g_short_loop_around_an_iir(be):
    """tests/test_dynamic_counts.py: the static loop kernel does not cover an IIRFilter; its refusal plans the graph again with
    the dynamic-count kernel"""
    c = _ctx(be)
    s = _source(c)
    d = c.create_delay(0.05, delay_time=0.003)
    f = c.create_iir_filter([0.2, 0.3, 0.1], [1.0, -0.5, 0.2])
    s.connect(d)
    d.connect(f).connect(c.create_gain(gain=0.5)).connect(d)
    f.connect(c.destination())
    return c


# name -> (builder, measurement switches, what the branch writes into the text)
BRANCHES = {
    "frozen_fan_in": (g_frozen_fan_in, {}, "keeps frozen state over silent quanta and is not fed by a single source"),
    "merger_falls_back": (g_merger_falls_back, {"WAA_STATIC_CHANNEL_COUNTS": "1"}, "comes from a ChannelMergerNode whose output falls back to one silent channel"),
    "merger_falls_back_refused": (g_merger_falls_back, {}, "in a graph that needs exact per-quantum channel counts (dyn_kernel) is out of scope"),
    "mono_shaper_into_a_wide_downmix": (g_mono_shaper_into_a_wide_downmix, {}, "with a rule that does not commute with the speakers up-mix made upstream"),
    "bus_grows_input_by_input": (g_bus_grows_input_by_input, {}, "sums signals of different widths whose up-mixes depend on the order"),
    "muted_cycle": (g_muted_cycle, {}, "is part of a cycle without a DelayNode: muted"),
    "short_echo_ring": (g_short_echo_ring, {}, "(a feedback delay shorter than a tile: the ring kernel walks it in chunks shorter than the delay)"),
    "biquad_in_the_forward_transform": (g_biquad_in_the_forward_transform, {}, "filtered by the forward transform's input stage"),
    "zero_gain_silent_modulator_refused": (g_zero_gain_silent_modulator_refused, {}, "while the audio-rate input of the param is silent"),
    "mixed_buffer_widths": (g_mixed_buffer_widths, {}, "dynamic-count group"),
    "short_loop_around_an_iir": (g_short_loop_around_an_iir, {}, "dynamic-count group"),
}


# ---- the item tables of the dynamic-count plan (dyn_items.txt): one small graph per line of waa_plan_dyn.cpp that the graphs above
# ---- do not execute (measured with gcov on the planner as it was before plan_dynamic_groups was split)
def _burst(c, n_ch=2, frames=RQ * 20, start=0.0, seed0=5):
    """a source that ends long before the render does: the count of its signal changes mid-render"""
    s = c.create_buffer_source()
    s.set_buffer_batch(white_noise(c.n_instances, n_ch, frames, seed0=seed0) * np.float32(0.5), SR)
    s.start_at(start)
    return s


def _mono_and_burst(c, n_ch=2, seed0=30):
    """a mono source that plays throughout and a wider one that joins late and ends early, to be summed by a count-sensitive node"""
    return _source(c, n_ch=1, seed0=seed0, scale=0.5), _burst(c, n_ch, RQ * 30, RQ * 12 / SR, seed0 + 1)


def _gain_modulated_from_its_loop(be, n_mod=1, outside=False):
    """tests/test_cycles.py: src -> Delay -> Gain(g) -> back, Delay -> Gain(depth) -> g.gain, n_mod times; outside: an LFO on g.gain
    too, made first so that the param sums it last"""
    c = _ctx(be)
    lfo = c.create_oscillator(type_="sine", frequency=7.0) if outside else None
    s = _source(c)
    d = c.create_delay(1.0, delay_time=0.01)
    g = c.create_gain(gain=0.3)
    s.connect(d)
    d.connect(g).connect(d)
    for _ in range(n_mod):
        d.connect(c.create_gain(gain=0.2)).connect(g.gain)
    if outside:
        lfo.connect(g.gain)
        lfo.start()
    d.connect(c.destination())
    return c


def g_dyn_gain_modulated_from_its_loop(be):
    return _gain_modulated_from_its_loop(be)


def g_dyn_gain_param_with_five_loop_inputs_refused(be):
    return _gain_modulated_from_its_loop(be, n_mod=5)


def g_dyn_gain_param_from_inside_and_outside_refused(be):
    return _gain_modulated_from_its_loop(be, outside=True)


def g_dyn_filter_param_from_its_loop_refused(be):   # tests/test_cycles.py
    c = _ctx(be)
    s = _source(c)
    d = c.create_delay(1.0, delay_time=0.01)
    bq = c.create_biquad_filter(type_="lowpass", frequency=800.0)
    s.connect(d)
    d.connect(bq).connect(c.create_gain(gain=0.3)).connect(d)
    d.connect(c.create_gain(gain=200.0)).connect(bq.frequency)
    d.connect(c.destination())
    return c


def _conv_behind_a_group(be, ir):
    """tests/test_dynamic_counts.py: stereo burst, silence, a mono source, a second stereo burst into a convolver"""
    c = _ctx(be)
    conv = c.create_convolver(buffer=waa.AudioBuffer(ir, SR))
    for s in (_burst(c, 2, RQ * 6, RQ * 2 / SR, 61), _burst(c, 1, RQ * 10, RQ * 20 / SR, 62), _burst(c, 2, RQ * 8, RQ * 26 / SR, 63)):
        s.connect(conv)
    conv.connect(c.destination())
    return c


def g_dyn_conv_mono_response_stereo_input(be):   # channel 1 in compacted time
    return _conv_behind_a_group(be, _decaying_ir(1, 1700, 64))


def g_dyn_conv_response_with_zero_segments(be):  # exact zeros inside the response and below 1e-6 at its end: the noise floor's segment masks
    ir = _decaying_ir(2, 4000, 65)
    ir[0, 1024:2048] = 0.0
    ir[1, 2048:3072] = 0.0
    ir[:, 3500:] = 0.0
    return _conv_behind_a_group(be, ir)


def g_dyn_analyser(be):
    c = _ctx(be)
    pan, an = c.create_stereo_panner(pan=0.3), c.create_analyser()
    for s in _mono_and_burst(c):
        s.connect(pan)
    pan.connect(an).connect(c.destination())
    return c


def g_dyn_shaper_without_a_curve(be):
    c = _ctx(be)
    sh = c.create_wave_shaper()
    for s in _mono_and_burst(c):
        s.connect(sh)
    sh.connect(c.create_stereo_panner(pan=0.25)).connect(c.destination())
    return c


def g_dyn_hrtf_behind_its_group(be):
    c = _ctx(be)
    pn = c.create_panner(panning_model="HRTF", position=(0.8, 0.3, -0.6))
    g = c.create_gain(gain=0.8)
    _burst(c).connect(g)
    _burst(c, 1, RQ * 30, RQ * 5 / SR, 6).connect(g)
    g.connect(pn).connect(c.destination())
    return c


def g_dyn_equal_power_panner(be):   # both laws of the PannerNode
    c = _ctx(be)
    pn = c.create_panner(distance_model="inverse", ref_distance=1.0, position=(1.5, 0.0, -1.0))
    for s in _mono_and_burst(c):
        s.connect(pn)
    pn.connect(c.destination())
    return c


def g_qloop_many_modulators_refused(be):   # the modulators' sum takes a launch that is not a param's own
    c = _ctx(be, frames=RQ * 70 + 33)
    d = c.create_delay(0.1, delay_time=0.01)
    sh = c.create_wave_shaper(curve=CURVE, oversample="2x")
    g = c.create_gain(gain=0.45)
    for k in range(10):
        lfo = c.create_oscillator(type_="sine", frequency=3.0 + k)
        lfo.connect(g.gain)
        lfo.start()
    _burst(c).connect(d)
    d.connect(sh).connect(g).connect(d)
    sh.connect(c.destination())
    return c


def g_dyn_oscillator_source(be):
    c = _ctx(be)
    osc = c.create_oscillator(type_="sawtooth", frequency=330.0)
    osc.start_at(RQ * 2.25 / SR)
    pan = c.create_stereo_panner(pan=-0.4)
    osc.connect(pan)
    _burst(c, start=RQ * 20 / SR).connect(pan)
    pan.connect(c.destination())
    return c


def g_dyn_param_driven_by_a_pending_member(be):  # the filter's group is launched first, then the param's summing chain, then the gain's
    c = _ctx(be)
    bq = c.create_biquad_filter(type_="lowpass", frequency=800.0)
    g = c.create_gain(gain=0.3)
    for s in _mono_and_burst(c):
        s.connect(bq)
    bq.connect(c.destination())
    bq.connect(g.gain)
    _burst(c, 1, RQ * 30, seed0=6).connect(g).connect(c.destination())
    return c


def g_qloop_pair_inside_one_segment(be):   # tests/test_frozen_loops.py: the breaking delay sits behind the node, writer and reader in one launch
    c = _ctx(be, frames=RQ * 70 + 33)
    mix = c.create_gain(gain=1.0)
    sh = c.create_wave_shaper(curve=CURVE, oversample="4x")
    d = c.create_delay(0.1, delay_time=0.02)
    _burst(c, 2, RQ * 25, seed0=12).connect(mix)
    mix.connect(sh).connect(c.create_gain(gain=0.5)).connect(d).connect(mix)
    sh.connect(c.destination())
    return c


def g_qloop_two_split_pairs(be):           # 480 and 960 frames across the cut: the shorter delay bounds the block (3 quanta)
    c = _ctx(be, frames=RQ * 70 + 33)
    s = _burst(c)
    sh = c.create_wave_shaper(curve=CURVE, oversample="2x")
    g = c.create_gain(gain=0.3)
    for t in (0.02, 0.01):
        d = c.create_delay(0.1, delay_time=t)
        s.connect(d)
        d.connect(sh)
        g.connect(d)
    sh.connect(g)
    sh.connect(c.destination())
    return c


def g_qloop_conv_mono_response_refused(be):
    c = _ctx(be, frames=RQ * 70 + 33)
    d = c.create_delay(0.1, delay_time=0.005)
    cv = c.create_convolver(buffer=waa.AudioBuffer(_decaying_ir(1, 300, 7), SR))
    _burst(c).connect(d)
    d.connect(cv).connect(c.create_gain(gain=0.25)).connect(d)
    cv.connect(c.destination())
    return c


def g_dyn_pipeline_with_a_loop_and_a_pair(be):   # a delay pair in front of a short loop around an IIR filter: neither is cut
    c = _ctx(be)
    d0 = c.create_delay(0.05, delay_time=0.002)
    d = c.create_delay(0.05, delay_time=0.003)
    f = c.create_iir_filter([0.2, 0.3, 0.1], [1.0, -0.5, 0.2])
    _burst(c).connect(c.create_biquad_filter(type_="lowpass", frequency=900.0)).connect(d0).connect(d)
    d.connect(f).connect(c.create_gain(gain=0.5)).connect(d)
    f.connect(c.create_stereo_panner(pan=0.2)).connect(c.create_biquad_filter(type_="highpass", frequency=200.0)).connect(c.destination())
    return c


def g_dyn_wide_source_into_a_convolver(be):   # (the convolver's channel config keeps its input stereo)
    c = _ctx(be, n_out=4)
    cv = c.create_convolver(buffer=waa.AudioBuffer(_decaying_ir(4, 300, 7), SR))
    _burst(c, 4).connect(cv).connect(c.destination())
    return c


def g_dyn_nine_inputs_refused(be):
    c = _ctx(be)
    pan = c.create_stereo_panner(pan=0.1)
    for k in range(9):
        _burst(c, 1 + k % 2, RQ * (10 + k), RQ * k / SR, 20 + k).connect(pan)
    pan.connect(c.destination())
    return c


def _filter_chain(be, n_ch, n_filters):
    c = _ctx(be, n_out=n_ch)
    head = c.create_biquad_filter(type_="lowpass", frequency=5000.0)
    for s in _mono_and_burst(c, n_ch):
        s.connect(head)
    for _ in range(n_filters - 1):
        head = head.connect(c.create_biquad_filter(type_="lowpass", frequency=5000.0))
    head.connect(c.destination())
    return c


def g_dyn_49_members_refused(be):
    return _filter_chain(be, 2, 48)


def g_dyn_local_memory_refused(be):  # 5.1 signals: 40 items do not fit 160 KB
    return _filter_chain(be, 6, 39)


# the graphs above that plan a dynamic-count group, and those made for the lines they leave out
DYN_ITEMS = {name: NAMED[name] for name in ("qloop_shaper_2x", "qloop_hrtf", "qloop_automated", "qloop_conv_and_shaper")}
DYN_ITEMS.update({name: BRANCHES[name][:2] for name in ("frozen_fan_in", "mono_shaper_into_a_wide_downmix", "bus_grows_input_by_input",
                                                        "mixed_buffer_widths", "short_loop_around_an_iir")})
DYN_ITEMS.update({
    "gain_modulated_from_its_loop": (g_dyn_gain_modulated_from_its_loop, {}),
    "conv_mono_response_stereo_input": (g_dyn_conv_mono_response_stereo_input, {}),
    "conv_response_with_zero_segments": (g_dyn_conv_response_with_zero_segments, {}),
    "conv_without_the_noise_floor": (g_dyn_conv_response_with_zero_segments, {"WAA_NO_CONV_NOISE_FLOOR": "1"}),
    "analyser": (g_dyn_analyser, {}), "shaper_without_a_curve": (g_dyn_shaper_without_a_curve, {}),
    "hrtf_behind_its_group": (g_dyn_hrtf_behind_its_group, {}), "oscillator_source": (g_dyn_oscillator_source, {}),
    "equal_power_panner": (g_dyn_equal_power_panner, {}),
    "param_driven_by_a_pending_member": (g_dyn_param_driven_by_a_pending_member, {}),
    "qloop_pair_inside_one_segment": (g_qloop_pair_inside_one_segment, {}), "qloop_two_split_pairs": (g_qloop_two_split_pairs, {}),
    "qloop_one_quantum": (g_qloop_two_split_pairs, {"WAA_LOOP_ONE_QUANTUM": "1"}),
    "short_loop_around_an_iir_one_stage": (g_short_loop_around_an_iir, {"WAA_DYN_STAGES": "1"}),
    "pipeline_with_a_loop_and_a_pair": (g_dyn_pipeline_with_a_loop_and_a_pair, {}),
    "wide_source_into_a_convolver": (g_dyn_wide_source_into_a_convolver, {}), "nine_inputs_refused": (g_dyn_nine_inputs_refused, {}),
    "49_members_refused": (g_dyn_49_members_refused, {}), "local_memory_refused": (g_dyn_local_memory_refused, {}),
    "filter_param_from_its_loop_refused": (g_dyn_filter_param_from_its_loop_refused, {}),
    "gain_param_with_five_loop_inputs_refused": (g_dyn_gain_param_with_five_loop_inputs_refused, {}),
    "gain_param_from_inside_and_outside_refused": (g_dyn_gain_param_from_inside_and_outside_refused, {}),
    "qloop_conv_mono_response_refused": (g_qloop_conv_mono_response_refused, {}),
    "qloop_frozen_node_refused": (g_qloop_hrtf, {"WAA_NO_FROZEN_LOOPS": "1"}),
    "qloop_matrix_shaper_refused": (g_qloop_shaper_2x, {"WAA_OS_MATRIX": "1"}),
    "qloop_many_modulators_refused": (g_qloop_many_modulators_refused, {}),
})


def random_graph(seed, frozen):
    def build(be):
        c, _ = build_random_graph(be, seed, frozen=frozen)
        c.device = waa.PLAN_ONLY
        return c
    return build


# the 60 seeds of test_random_graphs_plan_on_cpu, plain and with frozen-state nodes
RANDOM = {f"seed {seed}{' frozen' if frozen else ''}": (random_graph(seed, frozen), {}) for frozen in (False, True) for seed in range(60)}


def describe(be, build, switches, setenv, delenv):
    """the plan text with the launch list behind it, the first line's timing tail cut off; a refusal as its status and message"""
    setenv("WAA_PLAN_LAUNCHES", "1")
    for k, v in switches.items():
        setenv(k, v)
    try:
        c = build(be)
        try:
            text = c.plan_describe()
        except waa.WaaError as e:
            text = f"refused with status {e.status}: {e}\n"
        c.close()
    finally:
        for k in switches:
            delenv(k)
    first, _, rest = text.partition("\n")
    return first.split(" | timing:")[0] + "\n" + rest


def _sections(text):
    out, name = {}, None
    for line in text.splitlines(keepends=True):
        if line.startswith("==== "):
            name = line[5:].rstrip("\n")
            out[name] = ""
        else:
            out[name] += line
    return out


def _kind_list(text):
    kinds = []
    for m in re.finditer(r"^launch \d+: kind (\d+) (\S+) ", text, re.M):
        assert KIND_NAMES[int(m.group(1))] == m.group(2), m.group(0)
        kinds.append(int(m.group(1)))
    return kinds


def named_text(be, setenv, delenv):
    """named.txt: the full text of every named graph, a section each"""
    return "".join(f"==== {name}\n{describe(be, build, switches, setenv, delenv)}" for name, (build, switches) in NAMED.items())


def random_line(name, text):
    """random.txt holds one line per random graph instead of its text (120 texts are 260 KB): the SHA-256 of the full text, which
    the comparison is made on, and the kinds of its launches in order, for a reader and for the coverage test"""
    what = "refused" if text.startswith("refused") else "kinds " + ",".join(str(k) for k in _kind_list(text))
    return f"{name}: sha256 {hashlib.sha256(text.encode()).hexdigest()} {what}\n"


def _golden(name):
    with open(os.path.join(GOLDEN, name + ".txt")) as f:
        return f.read()


def test_named_launch_lists_are_what_they_were(hip, monkeypatch):
    want = _sections(_golden("named"))
    assert list(want) == list(NAMED)
    for name, (build, switches) in NAMED.items():
        got = describe(hip, build, switches, monkeypatch.setenv, monkeypatch.delenv)
        assert got == want[name], name
        assert "\nlaunch 0: " in got or (name.endswith("_refused") and got.startswith("refused with status 4:")), got


def branches_text(be, setenv, delenv):
    """branches.txt: like named.txt, for BRANCHES"""
    return "".join(f"==== {name}\n{describe(be, build, switches, setenv, delenv)}" for name, (build, switches, _) in BRANCHES.items())


def test_branch_launch_lists_are_what_they_were(hip, monkeypatch):
    """the planner branches the named corpus does not reach, a graph each: the text says that the branch was taken, and is what
    the planner wrote before build_plan_rest was split into passes"""
    want = _sections(_golden("branches"))
    assert list(want) == list(BRANCHES)
    for name, (build, switches, phrase) in BRANCHES.items():
        got = describe(hip, build, switches, monkeypatch.setenv, monkeypatch.delenv)
        assert phrase in got, (name, got)
        assert got == want[name], name
        assert "\nlaunch 0: " in got or (name.endswith("_refused") and got.startswith("refused with status 4:")), got


def dyn_items_text(be, setenv, delenv):
    """dyn_items.txt: like named.txt, for DYN_ITEMS, with the item tables (WAA_PLAN_DYN_ITEMS=1) behind every text"""
    return "".join(f"==== {name}\n{describe(be, build, dict(switches, WAA_PLAN_DYN_ITEMS='1'), setenv, delenv)}"
                   for name, (build, switches) in DYN_ITEMS.items())


def test_dynamic_item_tables_are_what_they_were(hip, monkeypatch):
    """what the dynamic-count planner writes into the DynItem tables, the DynDescs and the ConvCodeDescs — which the launch list
    does not show — and its refusals with status and text: written by plan_dynamic_groups as it was while it was one function of
    700 lines, with the same dump patched in"""
    want = _sections(_golden("dyn_items"))
    assert list(want) == list(DYN_ITEMS)
    for name, (build, switches) in DYN_ITEMS.items():
        got = describe(hip, build, dict(switches, WAA_PLAN_DYN_ITEMS="1"), monkeypatch.setenv, monkeypatch.delenv)
        assert got == want[name], name
        if name.endswith("_refused"):
            assert got.startswith("refused with status 4:"), got
        else:
            assert re.search(r"^launch \d+ dyn: n_items=\d+ ", got, re.M) and re.search(r"^launch \d+ item 0: kind=", got, re.M), got


def test_random_launch_lists_are_what_they_were(hip, monkeypatch):
    want = _golden("random").splitlines(keepends=True)
    assert len(want) == len(RANDOM)
    planned = 0
    for (name, (build, switches)), line in zip(RANDOM.items(), want):
        got = describe(hip, build, switches, monkeypatch.setenv, monkeypatch.delenv)
        assert random_line(name, got) == line, got   # (the text that differs: compare with the same dump of the parent commit)
        assert got.startswith(("batch:", "refused with status 4:")), got
        planned += "\nlaunch 0: " in got
    assert planned >= 80


def test_the_validator_names_the_kind_it_refuses(hip, monkeypatch):
    """(a reversed launch list, as in tests/test_plan.py: the message keeps the number and says what it stands for)"""
    got = describe(hip, g_misordered_refused, {"WAA_DEBUG_REVERSE_PLAN": "1"}, monkeypatch.setenv, monkeypatch.delenv)
    assert re.fullmatch(r"refused with status 3: internal: launch 0 of the plan \(kind (\d+), (\w+)\) reads a buffer that a later launch produces\n", got), got
    m = re.search(r"kind (\d+), (\w+)", got)
    assert KIND_NAMES[int(m.group(1))] == m.group(2)


def test_the_corpus_reaches_every_kind_and_every_loop_form():
    """over the expected files, which the tests above hold the planner to (the device-planned Timeline graph:
    test_launch_list_of_device_side_automation)"""
    named = _golden("named")
    cpu = set(_kind_list(named))
    for line in _golden("random").splitlines():
        if " kinds " in line:
            cpu |= {int(k) for k in line.rsplit(" kinds ", 1)[1].split(",") if k}
    assert cpu == set(range(len(KIND_NAMES))) - {KIND_NAMES.index("timeline")}
    assert cpu | set(_kind_list(_golden("device"))) == set(range(len(KIND_NAMES)))
    launches = [l for l in named.splitlines() if l.startswith("launch ")]
    for form in ("group=0 ", "group=1 ", "qgroup=0 ", "prologue=1 ", "fused=1 ", "ff=1 ", "fb=0 ", "tail="):
        assert any(form in l and not (form == "tail=" and "tail=-1" in l) for l in launches), form
    for k, name in enumerate(KIND_NAMES):   # every kind that may run once in front of a loop's blocks does so somewhere
        if name in ("zero_fill", "biquad_coefs", "biquad_hp", "panner_geom", "biquad_tile_digest", "chain"):
            assert any(f"kind {k} {name} " in l and "prologue=1" in l for l in launches), name
    for name in ("dyn", "link", "hrtf", "os_fft", "conv_fft", "conv_codes"):   # the ranged kinds, each inside a quantum-blocked loop
        assert any(f" {name} " in l and "qgroup=-1" not in l and "prologue=0" in l for l in launches), name
    assert any(l.startswith("group_tiles: ") for l in named.splitlines()) and any(l.startswith("qgroup_quanta: ") for l in named.splitlines())


@pytest.mark.gpu
def test_launch_list_of_device_side_automation(hip, monkeypatch):
    """per-context automation is replayed on the device (StepKind::Timeline) only by a batch that has one"""
    got = describe(hip, lambda be: g_timeline(be, device=0), {}, monkeypatch.setenv, monkeypatch.delenv)
    assert got == _sections(_golden("device"))["timeline"]
    assert KIND_NAMES.index("timeline") in _kind_list(got)
