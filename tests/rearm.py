"""Helpers of the "same graph, new audio" tests (tests/test_rearm.py, tests/test_render_sharded.py): waa_batch_rearm keeps a
batch's plan, device buffers and tables and takes new AudioBuffers into the source buffers it was planned with.  A second render
of the SAME audio cannot see a kernel or a plan that keeps something derived from the audio it rendered first; a render of OTHER
audio, compared bit for bit with a fresh batch of the same graph on that audio, can.  Kept apart from the -m gpu modules so that
the audio patterns and the comparison run on a box without a GPU too.

Audio patterns: dense noise, other dense noise, and sparse noise — instance 0 all zeros, the other instances with whole render
quanta zeroed at a pattern of their own and a few runs of silence longer than a convolver segment (1024 frames): where the zeros
fall decides the convolver's zero / noise decisions, a DelayNode that has read only zeros, the HRTF panner's exact-zeros form."""
import ctypes

import numpy as np

import web_audio_api_rs_amd as waa
from graphs import white_noise

RQ = 128
SEGMENT = 1024  # a convolver segment (waa_conv.hip): the long silent runs of the sparse pattern are longer


def live_quanta(n_inst, n_quanta, seed=0x5A75E):
    """bool [n_inst, n_quanta]: the render quanta the sparse pattern keeps.  Instance 0 keeps none; instance i >= 1 drops about a
    third of its quanta at random (its own generator) and two runs of 9..16 quanta (1152..2048 frames) at places of its own."""
    keep = np.ones((n_inst, n_quanta), bool)
    keep[0] = False
    for i in range(1, n_inst):
        rng = np.random.default_rng(seed + i)
        keep[i] = rng.random(n_quanta) >= 0.35
        for _ in range(2):
            run = int(rng.integers(SEGMENT // RQ + 1, 2 * SEGMENT // RQ + 1))
            q0 = int(rng.integers(0, max(1, n_quanta - run)))
            keep[i, q0:q0 + run] = False
    return keep


def sparsify(x):
    """x [n_inst, channels, frames] with the sparse pattern applied: dropped quanta are +0.0 in every channel (a copy)"""
    x = np.array(x, copy=True)
    n_inst, _, frames = x.shape
    nq = (frames + RQ - 1) // RQ
    keep = live_quanta(n_inst, nq)
    for i in range(n_inst):
        for q in np.flatnonzero(~keep[i]):
            x[i, :, q * RQ:(q + 1) * RQ] = 0.0
    return x


def dense(n_inst, n_ch, frames, seed0=0xA0D10):
    """white noise (tests/graphs.py): the default audio of every generator"""
    return white_noise(n_inst, n_ch, frames, seed0=seed0)


def other_dense(n_inst, n_ch, frames, seed0=0xA0D10):
    """white noise of other seeds"""
    return white_noise(n_inst, n_ch, frames, seed0=seed0 + 0x2D5E1)


def sparse(n_inst, n_ch, frames, seed0=0xA0D10):
    """other white noise with the sparse pattern applied"""
    return sparsify(other_dense(n_inst, n_ch, frames, seed0))


# (audio A, audio B) of the re-arm tests
PAIRS = {"dense-dense": (dense, other_dense), "dense-sparse": (dense, sparse), "sparse-dense": (sparse, other_dense)}


def refill_from(ctx, donor, only=None):
    """waa_batch_rearm on the rendered context `ctx`, then every AudioBufferSourceNode of it that was filled batch-wise takes the
    audio of the same node of `donor` — the same builder run on other audio, never applied: `_batch` goes to
    source_set_buffer_batch, `_pcm` to source_set_buffer_pcm16_batch.  only: node ids to refill (default all).  Returns the
    number of sources refilled."""
    b, h = ctx._b, ctx._handle
    b.check(b.batch_rearm(h))
    n = 0
    for nd in ctx._nodes:
        if not isinstance(nd, waa.AudioBufferSourceNode) or (only is not None and nd.id not in only):
            continue
        dn = donor._nodes[nd.id]
        assert type(dn) is type(nd), (nd.id, type(nd), type(dn))
        if nd._batch is not None:
            data, sr = dn._batch
            b.check(b.source_set_buffer_batch(h, nd.id, waa.api._fp(data), data.shape[1], data.shape[2], sr))
            n += 1
        if nd._pcm is not None:
            pcm, sr = dn._pcm
            b.check(b.source_set_buffer_pcm16_batch(h, nd.id, pcm.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), pcm.shape[2],
                                                    pcm.shape[1], sr))
            n += 1
    return n


def render_again(ctx):
    """waa_render of a re-armed context and its download [n_inst, channels, length]"""
    b, h = ctx._b, ctx._handle
    b.check(b.render(h))
    out = np.empty((ctx.n_instances, ctx.number_of_channels, ctx.length), np.float32)
    b.check(b.download_all(h, waa.api._fp(out)))
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8, 8: np.uint64}[a.dtype.itemsize])


def first_difference(got, want):
    """None when got and want hold the same bits (NaNs compare too), else (number of differing elements, index of the first,
    its value in got, its value in want)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    diff = _bits(got) != _bits(want)
    if not diff.any():
        return None
    k = np.unravel_index(int(np.argmax(diff)), diff.shape)
    return int(diff.sum()), tuple(int(v) for v in k), got[k].item(), want[k].item()


def assert_same_bits(got, want, what="the re-armed render", axes=("instance", "channel", "frame")):
    """got == want bit for bit; otherwise the first difference is reported at its (instance, channel, frame) — `axes` names the
    dimensions — with both values"""
    d = first_difference(got, want)
    assert d is None, (f"{what} differs from a fresh batch on the same audio in {d[0]} of {got.size} elements; the first difference "
                       f"at ({', '.join(axes)}) {d[1]}: {d[2]!r}, fresh {d[3]!r}")


def assert_differs(got, first, what="the re-armed render"):
    """a refill that did nothing must not pass: the render on the new audio differs from the one on the old"""
    assert first_difference(got, first) is not None, f"{what} equals the render of the previous audio bit for bit: nothing was refilled"


def modulated_graph(be, n_inst, frames, targets=("playback_rate",), modulator="source", device=0, sr=48000.0):
    """(ctx, src): `src` is a BufferSource (stereo, filled by the caller) heard through Gain(0.5); two more BufferSources play a
    fixed buffer (the same for every instance), one straight to the destination, one through a PannerNode at (1, 0, -1).  The
    modulator — `src` itself or a 5 Hz sine oscillator — drives through a depth Gain each of `targets`: the first player's
    "playback_rate" (+-0.3) or "detune" (+-300 cents), the panner's "position_x" (+-0.3).  Those params are resolved by rendering
    the modulator at plan time.  (A source with a modulated rate feeding the panner would be nested modulation: out of scope.)"""
    ctx = waa.OfflineAudioContext(2, frames, sr, n_instances=n_inst, binding=be, device=device)
    src = ctx.create_buffer_source()
    src.connect(ctx.create_gain(gain=0.5)).connect(ctx.destination())
    fixed = waa.AudioBuffer(white_noise(1, 2, 2 * frames, seed0=0x91A7)[0] * 0.5, sr)
    player = ctx.create_buffer_source().set_buffer(fixed)
    player.connect(ctx.destination())
    voice = ctx.create_buffer_source().set_buffer(fixed)
    pan = ctx.create_panner(position=(1.0, 0.0, -1.0))
    voice.connect(pan).connect(ctx.destination())
    if modulator == "source":
        mod = src
    else:
        mod = ctx.create_oscillator(type_="sine", frequency=5.0)
        mod.start()
    for t in targets:
        depth = ctx.create_gain(gain=300.0 if t == "detune" else 0.3)
        mod.connect(depth).connect({"playback_rate": player.playback_rate, "detune": player.detune, "position_x": pan.position_x}[t])
    src.start()
    player.start()
    voice.start()
    return ctx, src
