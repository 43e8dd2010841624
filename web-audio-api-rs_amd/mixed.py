"""Many independent OfflineAudioContexts of DIFFERENT shapes -> as few device batches as their shapes allow.

The reference's unit is the context (src/context/offline.rs:78-143): a host that serves requests builds one
OfflineAudioContext per request, each with its own graph.  The library's unit is the batch — N contexts of ONE graph shape
rendered together (include/waa_hip.h) — so a serving host has to sort its contexts by shape first.  `render_contexts` is that
step for the Python mirror (round-5 review, missing 4): contexts built one by one, exactly like reference contexts
(`OfflineAudioContext(channels, length, rate)` with n_instances = 1), are bucketed by `shape_key` — the graph (node kinds, options,
channel configuration, connections), the context's format, the SHAPES of per-context payloads (an AudioBufferSource's channel count,
length and rate, and on the device library the padded length of an IIRFilterNode's coefficients, which become per-instance sets of the
batch) and the identity of payloads a batch shares (a convolver's impulse response, an oversampled shaper's curve, and on other bindings
IIR coefficients, an oscillator's PeriodicWave and built-in type, a plain shaper's curve, a Biquad's type and a PannerNode's distance and cone options
(not its panning model, which shapes the plan), which the device library takes per instance) — every bucket is merged into one
batch (per-context AudioBuffers, AudioParam values and automation, start / stop / loop settings become per-instance settings of the batch), rendered, and the AudioBuffers are handed back in the callers' order.
Contexts with suspend callbacks render on their own (their callbacks may do anything)."""
from __future__ import annotations

import hashlib
from typing import List, Sequence

import numpy as np

from .api import ALL, AudioBufferSourceNode, AudioParam, BiquadFilterNode, ConvolverNode, IIRFilterNode, OfflineAudioContext, OscillatorNode, PannerNode, \
    RenderedBatch, WaveShaperNode, _ScheduledSource


def _digest(a) -> str:
    a = np.ascontiguousarray(a)
    return hashlib.sha1(a.tobytes()).hexdigest()[:16] + str(a.shape) + str(a.dtype)


def _iir_set(nd):
    """the coefficients context 0 of an IIRFilterNode renders with"""
    return nd._inst_coefs.get(0, (nd.feedforward, nd.feedback))


def _osc_wave(nd):
    """the PeriodicWave context 0 of an OscillatorNode renders with (None: a built-in waveform)"""
    return nd._inst_waves.get(0, nd.periodic_wave)


def _curve(nd):
    """the curve context 0 of a WaveShaperNode renders with (None: it passes its input through)"""
    return nd._inst_curves.get(0, nd.curve)


def _wave_id(w) -> tuple:
    return ("table", _digest(w.table)) if w.table is not None else (_digest(w.real), _digest(w.imag), w.disable_normalization)


def _node_key(nd) -> tuple:
    d = nd._desc()
    ints = tuple(int(x) for x in d.i)
    if isinstance(nd, BiquadFilterNode) and nd.context._b.prefix == "waa_":
        # the device library takes one filter type per context: contexts that differ only in their Biquad's type share a batch
        ints = ("biquad-type",) + ints[1:]
    if isinstance(nd, OscillatorNode) and nd.context._b.prefix == "waa_" and nd.type_of(0) != "custom":
        # ... and one built-in oscillator type per context; a context with a PeriodicWave stays apart from one without (below)
        ints = ("oscillator-type",) + ints[1:]
    # (a DynamicsCompressorNode's meter is i[0] and stays in the key: a metered context and an unmetered one are two plans — the
    # second has no trace buffer and no fourth launch — and do not merge)
    dbls = tuple(float(x) for x in d.d)
    if isinstance(nd, PannerNode) and nd.context._b.prefix == "waa_":
        # ... and one set of distance and cone options per context (i[1], d[0..5]); the panning model (i[0]) stays in the key
        ints = ints[:1] + ("panner-options",) + ints[2:]
        dbls = ("panner-options",) + dbls[6:]
    key = [type(nd).__name__, int(d.kind), int(d.channel_count), int(d.channel_count_mode), int(d.channel_interpretation),
           ints, dbls]
    if isinstance(nd, ConvolverNode):  # (shared by the batch: another response is another batch)
        key.append(None if nd.buffer is None else (_digest(nd.buffer.data), float(nd.buffer.sample_rate)))
        pcm = getattr(nd, "_pcm", None)
        key.append(None if pcm is None else (_digest(pcm[0]), pcm[1]))
    if isinstance(nd, WaveShaperNode):
        curve = _curve(nd)
        if curve is not None and nd.context._b.prefix == "waa_" and nd.oversample == "none":
            # the device library takes one curve per context: contexts that differ only in their curves share a batch (every curve
            # keeps its own length); an oversampled shaper stages its one curve per workgroup and keeps the digest
            key.append("curve")
        else:
            key.append(None if curve is None else _digest(curve))
    if isinstance(nd, IIRFilterNode):
        ff, fb = _iir_set(nd)  # (a single context's own set: its instance-0 set if it was given one, else the constructor's)
        if nd.context._b.prefix == "waa_":
            # the device library takes one set per context: contexts that differ only in their coefficients share a batch; the
            # padded length (iir_filter.rs:282-309) stays in the key, so a batch never pays for a longer filter than its own
            key.append(("iir-len", max(ff.size, fb.size)))
        else:
            key.append((_digest(ff), _digest(fb)))
    if isinstance(nd, OscillatorNode) and nd.type_of(0) == "custom":
        if nd.context._b.prefix == "waa_":
            # the device library takes one PeriodicWave per context: contexts that differ only in their waves share a batch
            key.append("periodic-wave")
        else:
            key.append(_wave_id(_osc_wave(nd)))
    if isinstance(nd, AudioBufferSourceNode):
        # per-context payloads: their SHAPE is part of the batch's shape (one device buffer [instance][channel][frame])
        if nd._batch is not None or nd._pcm is not None or nd._pcm_one or nd._device is not None:
            key.append(("own-upload", id(nd)))  # (pre-batched / PCM / device-resident payloads: not merged)
        buf = nd._buffers.get(ALL)
        key.append(None if buf is None else (buf.number_of_channels, buf.length, float(buf.sample_rate)))
    return tuple(key)


def shape_key(ctx: OfflineAudioContext) -> tuple:
    """what two contexts must agree on to be rendered as two instances of one batch"""
    if ctx.n_instances != 1 or ctx._suspends or ctx._ctl or ctx._handle is not None:
        return ("alone", id(ctx))
    return (ctx.number_of_channels, ctx.length, ctx.sample_rate, ctx.device, id(ctx._b), tuple(_node_key(nd) for nd in ctx._nodes),
            tuple(ctx._edges))


def _merge_param(dst: AudioParam, src: AudioParam, i: int):
    dst._const[i] = src._const[ALL]
    dst._blocks += [(q0, v, i) for (q0, v, inst) in src._blocks]
    dst._events += [(k, v, t, a, c, i) for (k, v, t, a, c, inst) in src._events]


def _own_instance_zero(p: AudioParam):
    """the carrier's own blocks and events, so far "for all", are instance 0's"""
    p._blocks = [(q0, v, 0 if inst == ALL else inst) for (q0, v, inst) in p._blocks]
    p._events = [(k, v, t, a, c, 0 if inst == ALL else inst) for (k, v, t, a, c, inst) in p._events]


def _merge(bucket: Sequence[OfflineAudioContext]) -> OfflineAudioContext:
    """bucket[0] becomes the batch (n_instances = len(bucket)); the others' per-context settings become per-instance settings"""
    car = bucket[0]
    n = len(bucket)
    if n == 1:
        return car
    car.n_instances = n
    # anything every context sets identically stays a setting "for all" (automation shared by the batch is evaluated once)
    def same(get):
        first = get(car)
        return all(get(o) == first for o in bucket[1:])
    for k, cn in enumerate(car._nodes):
        others = [o._nodes[k] for o in bucket[1:]]
        for pi, p in enumerate(cn.params):
            ops = [o.params[pi] for o in others]
            ev = lambda q: [(a, b, c, d, None if e is None else e.tobytes()) for (a, b, c, d, e, _) in q._events]  # noqa: E731
            bl = lambda q: [(a, b.tobytes()) for (a, b, _) in q._blocks]  # noqa: E731
            if all(ev(o) == ev(p) and bl(o) == bl(p) for o in ops):
                for i, o in enumerate(ops, start=1):
                    if o._const[ALL] != p._const[ALL]:
                        p._const[i] = o._const[ALL]
                continue
            _own_instance_zero(p)
            for i, o in enumerate(ops, start=1):
                _merge_param(p, o, i)
        if isinstance(cn, _ScheduledSource):
            if not all(o._starts == cn._starts and o._stops == cn._stops for o in others):
                cn._starts = {(0 if inst == ALL else inst): v for inst, v in cn._starts.items()}
                cn._stops = {(0 if inst == ALL else inst): v for inst, v in cn._stops.items()}
                for i, o in enumerate(others, start=1):
                    if ALL in o._starts:
                        cn._starts[i] = o._starts[ALL]
                    if ALL in o._stops:
                        cn._stops[i] = o._stops[ALL]
        if isinstance(cn, IIRFilterNode):
            # every context's effective set (_iir_set) becomes its instance's; equal sets everywhere: the node stays shared
            sets = [_iir_set(nd) for nd in [cn] + others]
            cn._inst_coefs = {}
            cn.feedforward, cn.feedback = sets[0]
            if not all(np.array_equal(ff, sets[0][0]) and np.array_equal(fb, sets[0][1]) for ff, fb in sets[1:]):
                for i, (ff, fb) in enumerate(sets[1:], start=1):
                    cn.set_coefficients(ff, fb, instance=i)
        if isinstance(cn, BiquadFilterNode):
            # every context's effective type becomes its instance's; equal types everywhere: the node stays shared
            types = [nd.type_of(0) for nd in [cn] + others]
            cn._inst_types = {}
            cn.type_ = types[0]
            if not all(t == types[0] for t in types[1:]):
                for i, t in enumerate(types):
                    cn.set_type(t, instance=i)
        if isinstance(cn, PannerNode) and cn.context._b.prefix == "waa_":
            # every context's effective option set becomes its instance's; equal sets everywhere: the node stays shared
            sets = [nd.options_of(0) for nd in [cn] + others]
            cn._inst_options = {}
            cn.set_options(**sets[0])
            if not all(o == sets[0] for o in sets[1:]):
                for i, o in enumerate(sets):
                    cn.set_options(instance=i, **o)
        if isinstance(cn, WaveShaperNode) and _curve(cn) is not None:
            # every context's effective curve (_curve) becomes its instance's; equal curves everywhere: the node stays shared
            curves = [_curve(nd) for nd in [cn] + others]
            cn._inst_curves = {}
            cn.curve = curves[0]
            if not all(np.array_equal(c, curves[0]) for c in curves[1:]):
                cn.curve = None
                for i, c in enumerate(curves):
                    cn.set_curve(c, instance=i)
        if isinstance(cn, OscillatorNode) and cn.type_of(0) != "custom":
            # every context's effective built-in type becomes its instance's; equal types everywhere: the node stays shared
            types = [nd.type_of(0) for nd in [cn] + others]
            cn._inst_types = {}
            cn.periodic_wave = None  # (a shared wave that context 0's own type outranked: nobody renders with it)
            cn.type_ = types[0]
            if not all(t == types[0] for t in types[1:]):
                for i, t in enumerate(types):
                    cn.set_type(t, instance=i)
        if isinstance(cn, OscillatorNode) and cn.type_of(0) == "custom":
            # every context's effective wave (_osc_wave) becomes its instance's; equal waves everywhere: the node stays shared
            waves = [_osc_wave(nd) for nd in [cn] + others]
            cn._inst_waves = {}
            cn.periodic_wave = waves[0]
            if not all(_wave_id(w) == _wave_id(waves[0]) for w in waves[1:]):
                cn.periodic_wave = None  # (no shared wave: its table would be built on the host for nobody)
                for i, w in enumerate(waves):
                    cn.set_periodic_wave(w, instance=i)
        if isinstance(cn, AudioBufferSourceNode):
            if not all(o._buffers.get(ALL) is cn._buffers.get(ALL) for o in others):
                if ALL in cn._buffers:
                    cn._buffers = {0: cn._buffers[ALL]}
                for i, o in enumerate(others, start=1):
                    if ALL in o._buffers:
                        cn._buffers[i] = o._buffers[ALL]
            if not all(o._loop == cn._loop for o in others):
                cn._loop = {(0 if inst == ALL else inst): v for inst, v in cn._loop.items()}
                for i, o in enumerate(others, start=1):
                    if ALL in o._loop:
                        cn._loop[i] = o._loop[ALL]
    for pi, p in enumerate(car._listener.params):  # the AudioListener's nine params (addressed through the panners)
        ops = [o._listener.params[pi] for o in bucket[1:]]
        if any(o._events or o._blocks or o._const[ALL] != p._const[ALL] for o in ops) or p._events or p._blocks:
            _own_instance_zero(p)
            for i, o in enumerate(ops, start=1):
                _merge_param(p, o, i)
    return car


def render_contexts(contexts: Sequence[OfflineAudioContext]) -> List[RenderedBatch]:
    """start_rendering_sync of every context, as few device batches as their shapes allow; results in the callers' order (each a
    RenderedBatch of one instance).  The contexts are consumed (like a reference context by its render): the first context of a
    bucket becomes the batch and is closed afterwards."""
    buckets = {}
    for idx, ctx in enumerate(contexts):
        buckets.setdefault(shape_key(ctx), []).append(idx)
    out: List[RenderedBatch] = [None] * len(contexts)  # type: ignore[list-item]
    for key, members in buckets.items():
        batch = _merge([contexts[i] for i in members])
        data = batch.start_rendering_sync().data
        for slot, i in enumerate(members):
            out[i] = RenderedBatch(data[slot:slot + 1].copy(), batch.sample_rate)
        batch.close()
    return out


def bucket_report(contexts: Sequence[OfflineAudioContext]) -> List[List[int]]:
    """which contexts would share a batch (indices, in first-seen order of their shapes): for logs and tests"""
    buckets = {}
    for idx, ctx in enumerate(contexts):
        buckets.setdefault(shape_key(ctx), []).append(idx)
    return list(buckets.values())
