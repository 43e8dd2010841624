"""The graphs of tests/test_batch_sizes.py: the corpus of tests/test_launch_list.py (its builders, given a batch size, a length and a
device) and a few graphs of their own, every one built for a LIST of context indices `ids`: context k of the batch is context
ids[k] of an imagined big batch and gets the audio and the per-context values of that index.  So the device renders ids = 0 .. n-1
and the oracle any subset of them as a small batch of its own.

Per-context values (delay time, filter frequency, oscillator frequency, IIR set, impulse response, ...) are a function of
id % K, K = 14: neighbouring contexts never share a value, and context 0's value comes back only at 14, 28, ... — a kernel that
reads context i +- 1, or context 0 for everyone, renders something else.  The audio is white noise of seed0 + id (every context
its own) or, for the batches of more contexts than a grid has rows, of seed0 + id % K: periodic in the context index, so that the
65537 contexts cost the host K noise rows; K is even (the partners of a packed convolver pair repeat) and divides neither 65535
nor 65536 (a row that wraps lands on other audio).

The builders taken over from tests/test_launch_list.py (fm_pair, timeline, the frozen-state loops) give context k the value of
its POSITION k % K: they are rendered as whole ranges 0 .. n-1 only, never as a subset.

Kept apart from the test module so that the builders run on a box without a GPU (against the oracle and plan-only)."""
import contextlib

import numpy as np

import web_audio_api_rs_amd as waa
import test_launch_list as L
from graphs import c2, white_noise

K = 14
RQ, SR = 128, 48000.0
TWO_TILES = 2048 + 133        # tile kernels: two tiles, the second ragged
QUANTA = RQ * 5 + 37          # quantum-serial kinds: a few quanta and a remainder
OTHER_AUDIO = 1_000_003       # seed offset of the audio a context gets in the second render of the neighbour test


@contextlib.contextmanager
def audio_of(ids, periodic=False, other=None):
    """inside: white_noise(n, ...) as the builders of tests/test_launch_list.py (and of this module) call it returns the rows of
    the contexts `ids`; other = position in ids of the one context that gets other audio"""
    ids = np.asarray(ids, np.int64)
    key = ids % K if periodic else ids.copy()
    if other is not None:
        key[other] += OTHER_AUDIO
    uniq, inv = np.unique(key, return_inverse=True)

    def noise(n_inst, n_ch, frames, seed0=0xA0D10, first=0):
        assert n_inst == len(ids), (n_inst, len(ids))
        rows = np.stack([white_noise(1, n_ch, frames, seed0=seed0, first=first + int(k))[0] for k in uniq])
        return rows[inv]

    old = L.white_noise
    L.white_noise = noise
    try:
        yield
    finally:
        L.white_noise = old


def _each(param, ids, value_of):
    for k, i in enumerate(ids):
        param.set_value(float(np.float32(value_of(int(i) % K))), instance=k)


def _node(c, cls, which=0):
    return [n for n in c._nodes if isinstance(n, cls)][which]


def _kw(ids, device, **more):
    return dict(n=len(ids), device=device, **more)


# ---- the graphs: builder(be, ids, device, mono=False, frames=None) -> context (frames: another length than the graph's own) -------------------------------------------------------------
def b_gain(be, ids, device, mono=False, frames=None):
    """source -> Gain (one value per context) -> destination: the chain kernel"""
    c = L._ctx(be, **_kw(ids, device, frames=frames or TWO_TILES, n_out=1 if mono else 2))
    g = c.create_gain()
    _each(g.gain, ids, lambda k: 0.2 + 0.05 * k)
    L._source(c, n_ch=1 if mono else 2).connect(g).connect(c.destination())
    return c


def _c2(be, ids, device, mono, frames):
    ctx, nodes = c2(be, L.white_noise(len(ids), 1 if mono else 2, frames or TWO_TILES), device=device)
    return ctx, nodes["biquad"]


def b_c2(be, ids, device, mono=False, frames=None):
    """C2 with one cutoff per context: the streaming Biquad"""
    ctx, bq = _c2(be, ids, device, mono, frames)
    _each(bq.frequency, ids, lambda k: 200.0 * (1.0 + 0.25 * k))
    return ctx


def b_biquad_k_rate(be, ids, device, mono=False, frames=None):
    """... with one cutoff per context and quantum: the streaming kernel's k-rate form"""
    ctx, bq = _c2(be, ids, device, mono, frames)
    nq = ((frames or TWO_TILES) + RQ - 1) // RQ
    for k, i in enumerate(ids):
        bq.frequency.set_block(0, (np.linspace(100.0, 1000.0, nq) * (1.0 + 0.05 * (int(i) % K))).astype(np.float32), instance=k)
    return ctx


def b_biquad_a_rate_shared(be, ids, device, mono=False, frames=None):
    """... with ONE automated cutoff for the batch (a shared table has no per-context value): coefficient table, digests, lanes"""
    ctx, bq = _c2(be, ids, device, mono, frames)
    bq.frequency.set_value_at_time(10.0, 0.0).exponential_ramp_to_value_at_time(10000.0, 0.04)
    return ctx


def b_iir(be, ids, device, mono=False, frames=None):
    c = L._ctx(be, **_kw(ids, device, frames=frames or TWO_TILES, n_out=1 if mono else 2))
    f = c.create_iir_filter([0.2, 0.3, 0.1], [1.0, -0.5, 0.2])
    if len(ids) > 1:   # (one set per context; a batch of one keeps the shared set of context ids[0])
        for k, i in enumerate(ids):
            f.set_coefficients([0.2, 0.3, 0.1], [1.0, -0.5 + 0.02 * (int(i) % K), 0.2], instance=k)
    else:
        f.set_coefficients([0.2, 0.3, 0.1], [1.0, -0.5 + 0.02 * (int(ids[0]) % K), 0.2])
    L._source(c, n_ch=1 if mono else 2).connect(f).connect(c.destination())
    return c


def b_delay_gather(be, ids, device, mono=False, frames=None):
    """source -> Delay (one time per context) -> Convolver (300 taps: radix-4): a delay in front of a convolver keeps the gather"""
    nch = 1 if mono else 2
    c = L._ctx(be, **_kw(ids, device, frames=frames or TWO_TILES, n_out=nch))
    d = c.create_delay(0.1)
    _each(d.delay_time, ids, lambda k: 0.003 + 0.0011 * k + 0.37 / SR)
    L._source(c, n_ch=nch).connect(d).connect(c.create_convolver(buffer=waa.AudioBuffer(L._decaying_ir(nch, 300, 3), SR))).connect(c.destination())
    return c


# the shortest response of each convolver path (waa_plan_conv.cpp): <= 128 taps the direct FIR; 129 the first FFT size (B = 128,
# radix-4 in LDS); 49153 = 24 * 2048 + 1 the first that needs B = 8192, the three-pass transforms of waa_conv3.hip
TAPS = {"direct": 128, "r4": 129, "3pass": 24 * 2048 + 1}


def _conv_shared(path):
    def build(be, ids, device, mono=False, frames=None):
        nch = 1 if mono else 2
        c = L._ctx(be, **_kw(ids, device, frames=frames or TWO_TILES, n_out=nch))
        L._source(c, n_ch=nch).connect(c.create_convolver(buffer=waa.AudioBuffer(L._decaying_ir(nch, TAPS[path], 11), SR))).connect(c.destination())
        return c
    build.__doc__ = f"source -> Convolver, one response of {TAPS[path]} taps for the batch ({path})"
    return build


def _conv_inst(path):
    def build(be, ids, device, mono=False, frames=None):
        nch = 1 if mono else 2
        c = L._ctx(be, **_kw(ids, device, frames=frames or TWO_TILES, n_out=nch))
        conv = c.create_convolver()
        rows = np.stack([L._decaying_ir(nch, TAPS[path], 100 + 7 * k) for k in range(K)])
        if len(ids) > 1:
            conv.set_buffer_batch(rows[np.asarray(ids) % K], SR)
        else:
            conv.set_buffer(waa.AudioBuffer(rows[int(ids[0]) % K], SR))
        L._source(c, n_ch=nch).connect(conv).connect(c.destination())
        return c
    build.__doc__ = f"source -> Convolver, one response of {TAPS[path]} taps per context ({path})"
    return build


def _osc_ctx(be, ids, device, mono, frames):
    return L._ctx(be, **_kw(ids, device, frames=frames or TWO_TILES, n_out=1 if mono else 2))


def b_osc_par(be, ids, device, mono=False, frames=None):
    """one sawtooth, one frequency per context: the time-parallel kernel"""
    c = _osc_ctx(be, ids, device, mono, frames)
    o = c.create_oscillator(type_="sawtooth", frequency=220.0)
    _each(o.frequency, ids, lambda k: 110.0 * (1.0 + 0.21 * k))
    o.connect(c.destination())
    o.start_at(0.0007)
    return c


def _wave(k):
    rng = np.random.default_rng(900 + k)
    imag = (rng.uniform(-1, 1, 12) / np.arange(1, 13)).astype(np.float32)
    imag[0] = 0.0
    return waa.PeriodicWave(real=np.zeros(12, np.float32), imag=imag)


def b_osc_waves(be, ids, device, mono=False, frames=None):
    """one PeriodicWave and one frequency per context: the time-parallel kernel with the context's table staged in LDS"""
    c = _osc_ctx(be, ids, device, mono, frames)
    if len(ids) > 1:
        o = c.create_oscillator(frequency=220.0)
        for k, i in enumerate(ids):
            o.set_periodic_wave(_wave(int(i) % K), instance=k)
    else:
        o = c.create_oscillator(frequency=220.0, periodic_wave=_wave(int(ids[0]) % K))
    _each(o.frequency, ids, lambda k: 110.0 * (1.0 + 0.21 * k))
    o.connect(c.destination())
    o.start_at(0.0007)
    return c


OSC_TYPES = ("sine", "square", "sawtooth", "triangle")


def b_osc_types(be, ids, device, mono=False, frames=None):
    """one waveform type and one frequency per context: the time-parallel kernel of waa_osc_types.hip"""
    c = _osc_ctx(be, ids, device, mono, frames)
    types = [OSC_TYPES[(int(i) % K) % 4] for i in ids]
    o = c.create_oscillator(type_=types[0], frequency=220.0)
    if len(ids) > 1:
        o.set_type_batch(types)
    _each(o.frequency, ids, lambda k: 110.0 * (1.0 + 0.21 * k))
    o.connect(c.destination())
    o.start_at(0.0007)
    return c


def b_fm_pair(be, ids, device, mono=False, frames=None):
    return L.g_fm_pair(be, **_kw(ids, device, frames=frames or TWO_TILES, n_out=1 if mono else 2))


def comp_params(k):
    return dict(threshold=-30.0 - 1.5 * k, knee=float(3 * k), ratio=2.0 + k, attack=0.001 * (1 + k % 5), release=0.05 + 0.01 * k)


def b_compressor(be, ids, device, mono=False, frames=None):
    """source -> DynamicsCompressor, its five params one value per context"""
    c = L.g_compressor(be, **_kw(ids, device, frames=(frames or TWO_TILES) // RQ * RQ, n_out=1 if mono else 2))  # (whole quanta: the model's unit)
    comp = _node(c, waa.api.DynamicsCompressorNode)
    for name in ("threshold", "knee", "ratio", "attack", "release"):
        _each(getattr(comp, name), ids, lambda k, name=name: comp_params(k)[name])
    if mono:
        src = _node(c, waa.AudioBufferSourceNode)
        src._batch = (np.ascontiguousarray(src._batch[0][:, :1]), src._batch[1])
    return c


def b_timeline(be, ids, device, mono=False, frames=None):
    return L.g_timeline(be, **_kw(ids, device, frames=frames or QUANTA, n_out=1 if mono else 2))


def _hrtf(be, ids, device, frames, moving):
    c = L._ctx(be, **_kw(ids, device, frames=frames))
    pan = c.create_panner(panning_model="HRTF")
    for k, i in enumerate(ids):
        v = int(i) % K
        pan.position_x.set_value(float(np.cos(v)) * 2.0, instance=k)
        pan.position_z.set_value(float(np.sin(v)) * 2.0, instance=k)
    if moving:   # (one automated coordinate for the batch: the direction changes per quantum)
        pan.position_y.set_value_at_time(-0.5, 0.0).linear_ramp_to_value_at_time(0.8, frames / SR)
    else:
        _each(pan.position_y, ids, lambda k: 0.1 * (k % 11) - 0.5)
    L._source(c, n_ch=1).connect(pan).connect(c.destination())
    return c


def b_hrtf_static(be, ids, device, mono=False, frames=None):
    """mono source -> HRTF panner, one direction per context, 20 quanta: the transform form"""
    return _hrtf(be, ids, device, frames or RQ * 20 + 5, False)


def b_hrtf_short(be, ids, device, mono=False, frames=None):
    """... 6 quanta: fewer than a run of the transform form, the direct form with the host-interpolated pair (hrtf8_kernel)"""
    return _hrtf(be, ids, device, frames or QUANTA, False)


def b_hrtf_moving(be, ids, device, mono=False, frames=None):
    """... the direction automated: the direct form that interpolates per quantum (hrtf_kernel)"""
    return _hrtf(be, ids, device, frames or QUANTA, True)


def b_oversampled_shaper(be, ids, device, mono=False, frames=None):
    return L.g_oversampled_shaper(be, **_kw(ids, device, frames=frames or RQ * 20 + 37))


def _loop_gain(c, ids):
    _each(_node(c, waa.api.GainNode).gain, ids, lambda k: 0.3 + 0.03 * k)
    return c


def b_echo_ring(be, ids, device, mono=False, frames=None):
    """the echo loop of 2400 frames, one feedback gain per context: the LDS-ring kernel, one workgroup per context"""
    return _loop_gain(L.g_echo_ring(be, **_kw(ids, device, frames=frames or 2048 * 2 + 133)), ids)


def b_loop_kernel(be, ids, device, mono=False, frames=None):
    """... of 132 frames: the quantum-serial loop kernel, one wavefront per context"""
    return _loop_gain(L.g_loop_kernel(be, **_kw(ids, device, frames=frames or QUANTA)), ids)


def b_feed_forward_echo(be, ids, device, mono=False, frames=None):
    """source + Gain(0.5) * Delay(source), one delay time per context: from 256 contexts on the ring kernel with nothing fed back"""
    nch = 1 if mono else 2
    c = L._ctx(be, **_kw(ids, device, frames=frames or TWO_TILES, n_out=nch))
    s = L._source(c, n_ch=nch)
    d = c.create_delay(0.4)
    _each(d.delay_time, ids, lambda k: (1032.0 + 37.5 * k) / SR)   # (the ring's window starts at 1032 frames, tests/test_delay.py)
    s.connect(c.destination())
    s.connect(d).connect(c.create_gain(gain=0.5)).connect(c.destination())
    return c


def b_qloop_hrtf(be, ids, device, mono=False, frames=None):
    return L.g_qloop_hrtf(be, **_kw(ids, device, frames=frames or RQ * 30 + 33))


def b_qloop_shaper_2x(be, ids, device, mono=False, frames=None):
    return L.g_qloop_shaper_2x(be, **_kw(ids, device, frames=frames or RQ * 30 + 33))


def b_qloop_conv_and_shaper(be, ids, device, mono=False, frames=None):
    return L.g_qloop_conv_and_shaper(be, **_kw(ids, device, frames=frames or RQ * 40 + 33))


def b_splitter_merger(be, ids, device, mono=False, frames=None):
    return L.g_splitter_merger(be, **_kw(ids, device, frames=frames or TWO_TILES))


def b_listener_in_a_loop(be, ids, device, mono=False, frames=None):
    return L.g_listener_automated_in_a_loop(be, **_kw(ids, device, frames=frames or 2048 * 2 + 133))


def b_block_loop_zero_conv(be, ids, device, mono=False, frames=None):
    return L.g_block_loop_zero_conv(be, **_kw(ids, device, frames=frames or 2048 * 2 + 133))


def _resample_source(be, ids, device, mono=False, frames=None):
    """looping source at another rate, one playbackRate per context -> destination: the resampling-source kernel, 8 contexts per
    wavefront and 4 wavefronts per workgroup"""
    nch = 1 if mono else 2
    c = L._ctx(be, **_kw(ids, device, frames=frames or TWO_TILES, n_out=nch))
    s = c.create_buffer_source()
    s.set_buffer_batch(L.white_noise(len(ids), nch, 1500), SR)
    _each(s.playback_rate, ids, lambda k: 1.2 + 0.05 * k)
    s.set_loop(True)
    s.start()
    return c, s


def b_resample_plain(be, ids, device, mono=False, frames=None):
    c, s = _resample_source(be, ids, device, mono, frames)
    s.connect(c.destination())
    return c


def b_resample_shaper(be, ids, device, mono=False, frames=None):
    """... through a WaveShaper (the C5 shape: the curve staged in LDS by the same kernel)"""
    c, s = _resample_source(be, ids, device, mono, frames)
    i = np.arange(2048, dtype=np.float32)
    curve = np.cos(np.float32(np.pi) + i * np.float32(np.pi) / np.float32(2047)).astype(np.float32)
    s.connect(c.create_wave_shaper(curve=curve)).connect(c.destination())
    return c


DYN_QUANTA = 192   # launch_dyn: q_split = min(max(16384 / n_inst, 16), quanta / 6) — 193 quanta: 32 at 512 contexts, 31 at 513


def b_dyn_split(be, ids, device, mono=False, frames=None):
    """a stereo and a mono burst -> Gain (one value per context) -> HRTF panner, outside any loop (tests/test_launch_list.py's
    hrtf_behind_its_group, 193 quanta long): the dynamic-count groups keep no state, their quanta are spread over q_split
    workgroups per context"""
    c = L._ctx(be, **_kw(ids, device, frames=frames or RQ * DYN_QUANTA + 37))
    pn = c.create_panner(panning_model="HRTF", position=(0.8, 0.3, -0.6))
    g = c.create_gain()
    _each(g.gain, ids, lambda k: 0.4 + 0.04 * k)
    L._burst(c, frames=RQ * 60 + 9).connect(g)
    L._burst(c, 1, RQ * 90, RQ * 25 / SR, 6).connect(g)
    g.connect(pn).connect(c.destination())
    return c


def b_osc_post_gain(be, ids, device, mono=False, frames=None):
    """sawtooth -> Gain (one value per context) -> destination: the gain folded into the time-parallel kernel's store"""
    c = _osc_ctx(be, ids, device, mono, frames)
    o = c.create_oscillator(type_="sawtooth", frequency=220.0)
    _each(o.frequency, ids, lambda k: 110.0 * (1.0 + 0.21 * k))
    g = c.create_gain()
    _each(g.gain, ids, lambda k: 0.25 + 0.05 * k)
    o.connect(g).connect(c.destination())
    o.start_at(0.0007)
    return c


def b_conv_3pass_biquad(be, ids, device, mono=False, frames=None):
    """source -> Biquad (one cutoff per context) -> Convolver of 49153 taps, whole quanta so that the source is read in place: the
    filter is rendered by the forward transform's input stage (waa_conv3.hip: coefficients and state per context)"""
    nch = 1 if mono else 2
    c = L._ctx(be, **_kw(ids, device, frames=frames or 2048 + RQ, n_out=nch))
    bq = c.create_biquad_filter(type_="lowpass", frequency=2000.0, q=1.0)
    _each(bq.frequency, ids, lambda k: 1500.0 * (1.0 + 0.2 * k))
    L._source(c, n_ch=nch).connect(bq).connect(c.create_convolver(buffer=waa.AudioBuffer(L._decaying_ir(nch, TAPS["3pass"], 11), SR))).connect(c.destination())
    return c


def build(builder, be, ids, device=-1, mono=False, periodic=False, other=None, frames=None):
    """the graph `builder` for the contexts `ids` with their audio (white_noise as the builders of tests/test_launch_list.py call
    it is replaced while the builder runs: they are reused as they are); frames: another length than the graph's own"""
    ids = np.asarray(ids, np.int64)
    with audio_of(ids, periodic, other):
        return builder(be, ids, device, mono, frames)
