"""Host-side mirror of the reference's control API for the offline render path.

The names follow the reference crate (web-audio-api 1.6.0):

* ``OfflineAudioContext(number_of_channels, length, sample_rate)``  src/context/offline.rs:78
* ``create_buffer_source / create_biquad_filter / create_gain / create_convolver /
  create_stereo_panner / create_panner / create_analyser / create_wave_shaper /
  create_constant_source``                                         src/context/base.rs:23-367
* ``AudioNode.connect``                                            src/node/audio_node.rs:247-289
* ``AudioScheduledSourceNode.start/start_at/stop/stop_at``         src/node/scheduled_source.rs:6-44
* ``AudioParam.value / set_value``                                 src/param.rs:268-662
* ``start_rendering_sync``                                         src/context/offline.rs:157-185

The one extension is ``n_instances``: a context object stands for a *batch* of N
identically shaped OfflineAudioContexts rendered together by one ``waa_batch``
(include/waa_hip.h).  Per-instance payloads are addressed with ``instance=k``.

This module only talks to a C-ABI library through ctypes.  Which library is decided by
the caller (``bind(lib, prefix)``): the product binds ``libwaa_hip.so`` with prefix
``waa_`` (see __init__.py); the tests may bind the CPU oracle with prefix ``orc_``.
Nothing in this package imports or loads the oracle.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence

import numpy as np

RENDER_QUANTUM_SIZE = 128
PLAN_ONLY = -2  # WAA_DEVICE_PLAN_ONLY: configure + plan without a device (never renders)
ALL = 0xFFFFFFFF
ENDED_NEVER, ENDED_AT_UNLOAD = -1, -2
F64_MAX = 1.7976931348623157e308

# node kinds / enums (include/waa_hip.h)
NODE_DESTINATION, NODE_BUFFER_SOURCE, NODE_BIQUAD, NODE_GAIN, NODE_CONVOLVER = 0, 1, 2, 3, 4
NODE_STEREO_PANNER, NODE_PANNER, NODE_ANALYSER, NODE_WAVESHAPER, NODE_CONSTANT_SOURCE = 5, 6, 7, 8, 9
NODE_IIR_FILTER = 10
NODE_DELAY = 11
NODE_OSCILLATOR = 12
NODE_DYNAMICS_COMPRESSOR = 13
NODE_CHANNEL_SPLITTER = 14
NODE_CHANNEL_MERGER = 15
MAX_CHANNELS = 32  # src/lib.rs:21
OSCILLATOR_TYPE = {"sine": 0, "square": 1, "sawtooth": 2, "triangle": 3, "custom": 4}
MAX_IIR_COEFFS = 20
PARAM_INPUT = 0x80000000  # WAA_PARAM_INPUT(param): edge into an AudioParam of the target node
(EVENT_SET_VALUE, EVENT_SET_VALUE_AT_TIME, EVENT_LINEAR_RAMP, EVENT_EXPONENTIAL_RAMP, EVENT_CANCEL_SCHEDULED_VALUES,
 EVENT_SET_TARGET, EVENT_CANCEL_AND_HOLD, EVENT_SET_VALUE_CURVE) = range(8)  # WAA_EVENT_* (src/param.rs:151-160)
COUNT_MODE = {"max": 0, "clamped-max": 1, "explicit": 2}
INTERPRETATION = {"speakers": 0, "discrete": 1}
BIQUAD_TYPE = {"lowpass": 0, "highpass": 1, "bandpass": 2, "notch": 3, "allpass": 4, "peaking": 5,
               "lowshelf": 6, "highshelf": 7}
PANNING_MODEL = {"equalpower": 0, "HRTF": 1}
DISTANCE_MODEL = {"linear": 0, "inverse": 1, "exponential": 2}
OVERSAMPLE = {"none": 0, "2x": 1, "4x": 2}


class WaaError(RuntimeError):
    """Raised where the reference panics (the message keeps the W3C error name)."""

    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = status


class NodeDesc(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("channel_count", C.c_uint32), ("channel_count_mode", C.c_uint32),
                ("channel_interpretation", C.c_uint32), ("i", C.c_int32 * 4), ("d", C.c_double * 8)]


class EdgeDesc(C.Structure):
    _fields_ = [("from_", C.c_uint32), ("from_output", C.c_uint32), ("to", C.c_uint32), ("to_input", C.c_uint32)]


class GraphDesc(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("nodes", C.POINTER(NodeDesc)), ("n_edges", C.c_uint32),
                ("edges", C.POINTER(EdgeDesc))]



_FP = C.POINTER(C.c_float)
_DP = C.POINTER(C.c_double)
_FPP = C.POINTER(_FP)
_VP = C.c_void_p

# waa_render_sharded (include/waa_hip.h): the callbacks run on the library's sub-batch threads (ctypes takes the GIL for them)
SHARD_FN = C.CFUNCTYPE(C.c_int32, _VP, C.c_uint32, C.c_uint32, C.c_int32, _VP)


class ShardedJob(C.Structure):
    _fields_ = [("graph", C.POINTER(GraphDesc)), ("n_instances", C.c_uint32), ("n_channels_out", C.c_uint32),
                ("length_frames", C.c_uint64), ("sample_rate", C.c_float), ("n_devices", C.c_uint32),
                ("devices", C.POINTER(C.c_int32)), ("sub_batches", C.c_uint32), ("source_node", C.c_uint32),
                ("host_in", _VP), ("in_channels", C.c_uint32), ("in_pcm16", C.c_int32), ("in_frames", C.c_uint64),
                ("in_sample_rate", C.c_float), ("out_pcm16", C.c_int32), ("host_out", _VP), ("setup", SHARD_FN),
                ("pull", SHARD_FN), ("user", _VP), ("reuse_batches", C.c_uint32)]

class ArenaStats(C.Structure):
    """waa_arena_stats (include/waa_hip.h)"""
    _fields_ = [(n, C.c_uint64) for n in ("reserved_bytes", "in_use_bytes", "peak_bytes", "largest_free_bytes", "served", "misses",
                                          "miss_bytes")]


class ArenaGrades(C.Structure):
    """waa_arena_grades (include/waa_hip.h)"""
    _fields_ = [("unit_bytes", C.c_uint64), ("n_units", C.c_uint32), ("n_candidates", C.c_uint32), ("best_ms", C.c_float),
                ("worst_kept_ms", C.c_float), ("worst_candidate_ms", C.c_float), ("grading_ms", C.c_float)]


def arena_grades(binding, device=-1) -> dict:
    """waa_device_arena_grades as a dict (+ "unit_ms": the kept units' grades in address order); all zero without a graded arena"""
    g = ArenaGrades()
    binding.check(binding.device_arena_grades(int(device), C.cast(C.pointer(g), _VP), None, 0))
    out = {n: (int if n in ("unit_bytes", "n_units", "n_candidates") else float)(getattr(g, n)) for n, _ in ArenaGrades._fields_}
    ms = (C.c_float * max(int(g.n_units), 1))()
    binding.check(binding.device_arena_grades(int(device), C.cast(C.pointer(g), _VP), ms, int(g.n_units)))
    out["unit_ms"] = [float(ms[k]) for k in range(int(g.n_units))]
    return out


def arena_stats(binding, device=-1) -> dict:
    """waa_device_arena_stats as a dict (all zero when no arena is reserved on the device)"""
    st = ArenaStats()
    binding.check(binding.device_arena_stats(int(device), C.cast(C.pointer(st), _VP)))
    return {n: int(getattr(st, n)) for n, _ in ArenaStats._fields_}


# name -> (restype, argtypes); every symbol include/waa_hip.h declares
ABI = {
    "batch_create": (C.c_int32, [C.POINTER(GraphDesc), C.c_uint32, C.c_uint32, C.c_uint64, C.c_float, C.c_int32,
                                 C.POINTER(_VP)]),
    "batch_destroy": (None, [_VP]),
    "last_error": (C.c_char_p, []),
    "device_count": (C.c_int32, []),
    "device_arena_reserve": (C.c_int32, [C.c_int32, C.c_uint64]),
    "device_arena_stats": (C.c_int32, [C.c_int32, _VP]),
    "batch_rearm": (C.c_int32, [_VP]),
    "render_range": (C.c_int32, [_VP, C.c_uint64, C.c_uint32]),
    "connect": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "disconnect": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "device_arena_reserve_graded": (C.c_int32, [C.c_int32, C.c_uint64, C.c_uint64]),
    "device_arena_grades": (C.c_int32, [C.c_int32, _VP, _FP, C.c_uint32]),
    "source_set_buffer": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, _FPP, C.c_uint32, C.c_uint64, C.c_float]),
    "source_set_buffer_batch": (C.c_int32, [_VP, C.c_uint32, _FP, C.c_uint32, C.c_uint64, C.c_float]),
    "source_set_buffer_pcm16": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, C.POINTER(C.c_int16), C.c_uint32, C.c_uint64, C.c_float]),
    "source_set_buffer_pcm16_batch": (C.c_int32, [_VP, C.c_uint32, C.POINTER(C.c_int16), C.c_uint32, C.c_uint64, C.c_float]),
    "convolver_set_buffer_pcm16": (C.c_int32, [_VP, C.c_uint32, C.POINTER(C.c_int16), C.c_uint32, C.c_uint64, C.c_float]),
    "source_adopt_device": (C.c_int32, [_VP, C.c_uint32, _VP, C.c_uint32, C.c_uint64, C.c_float]),
    "source_start": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double]),
    "source_stop": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, C.c_double]),
    "source_set_loop": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, C.c_int32, C.c_double, C.c_double]),
    "source_ended": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, C.POINTER(C.c_int64)]),
    "convolver_set_buffer": (C.c_int32, [_VP, C.c_uint32, _FPP, C.c_uint32, C.c_uint64, C.c_float]),
    "waveshaper_set_curve": (C.c_int32, [_VP, C.c_uint32, _FP, C.c_uint32]),
    "oscillator_set_periodic_wave": (C.c_int32, [_VP, C.c_uint32, _FP, _FP, C.c_uint32, C.c_int32]),
    "oscillator_set_wavetable": (C.c_int32, [_VP, C.c_uint32, _FP, C.c_uint32]),
    "iir_set_coefficients": (C.c_int32, [_VP, C.c_uint32, _DP, C.c_uint32, _DP, C.c_uint32]),
    "iir_frequency_response": (C.c_int32, [_DP, C.c_uint32, _DP, C.c_uint32, C.c_float, _FP, _FP, _FP, C.c_uint32]),
    "param_schedule_event": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_float, C.c_double, C.c_double,
                                         _FP, C.c_uint32]),
    "timeline_create": (_VP, [C.c_float, C.c_float, C.c_float, C.c_int32]),
    "timeline_destroy": (None, [_VP]),
    "timeline_event": (C.c_int32, [_VP, C.c_int32, C.c_float, C.c_double, C.c_double, _FP, C.c_uint32]),
    "timeline_compute": (C.c_uint32, [_VP, C.c_double, C.c_double, C.c_uint32, _FP]),
    "timeline_value": (C.c_float, [_VP]),
    "timeline_render_device": (C.c_int32, [_VP, C.c_uint32, C.c_float, _FP, C.POINTER(C.c_uint8)]),
    "set_param_const": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float]),
    "set_param_block": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, _FP]),
    "render": (C.c_int32, [_VP]),
    "sync": (C.c_int32, [_VP]),
    "download": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, _FP, C.c_uint64]),
    "download_all": (C.c_int32, [_VP, _FP]),
    "download_all_pcm16": (C.c_int32, [_VP, C.POINTER(C.c_int16)]),
    "render_sharded": (C.c_int32, [_VP, C.POINTER(C.c_double)]),
    "sharded_in_flight": (C.c_int32, [C.c_uint32]),
    "shard_range": (C.c_int32, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "output_device": (C.c_int32, [_VP, C.POINTER(_VP), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "analyser_get_float_frequency_data": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, _FP, C.c_uint32]),
    "analyser_get_byte_frequency_data": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8), C.c_uint32]),
    "analyser_get_float_time_domain_data": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, _FP, C.c_uint32]),
    "analyser_get_byte_time_domain_data": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8), C.c_uint32]),
    "analyser_get_float_frequency_data_batch": (C.c_int32, [_VP, C.c_uint32, _FP, C.c_uint32]),
    "analyser_get_byte_frequency_data_batch": (C.c_int32, [_VP, C.c_uint32, C.POINTER(C.c_uint8), C.c_uint32]),
    "analyser_get_float_time_domain_data_batch": (C.c_int32, [_VP, C.c_uint32, _FP, C.c_uint32]),
    "analyser_get_byte_time_domain_data_batch": (C.c_int32, [_VP, C.c_uint32, C.POINTER(C.c_uint8), C.c_uint32]),
    "hrtf_load_sphere": (C.c_int32, [C.c_char_p, C.c_uint64]),
    "hrtf_hrir_length": (C.c_uint32, [C.c_float]),
    "hrtf_sample": (None, [C.c_float, _FP, _FP, _FP]),
    "buffer_resample": (C.c_uint64, [_FP, C.c_uint64, C.c_float, C.c_float, _FP, C.c_uint64]),
    "biquad_frequency_response": (C.c_int32, [C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _FP,
                                              _FP, _FP, C.c_uint32]),
    "plan_describe": (C.c_int32, [_VP, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "profile_enable": (C.c_int32, [_VP, C.c_int32]),
    "profile_count": (C.c_int32, [_VP]),
    "profile_get": (C.c_int32, [_VP, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "profile_reset": (C.c_int32, [_VP]),
}


# what include/waa_hip_device.h declares: entry points of the device library alone (the oracle keeps one context's worth of state)
ABI_DEVICE = {
    "iir_set_coefficients_instance": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, _DP, C.c_uint32, _DP, C.c_uint32]),
    "oscillator_set_periodic_wave_instance": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, _FP, _FP, C.c_uint32, C.c_int32]),
    "oscillator_set_wavetable_instance": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, _FP, C.c_uint32]),
    "oscillator_get_wavetable": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, _FP, C.c_uint32]),
    "waveshaper_set_curve_instance": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, _FP, C.c_uint32]),
    "biquad_set_type_instance": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, C.c_int32]),
    "oscillator_set_type_instance": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, C.c_int32]),
    "panner_set_options_instance": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, _VP]),
    "compressor_get_reduction": (C.c_int32, [_VP, C.c_uint32, C.c_uint32, _FP]),
    "compressor_get_reduction_series": (C.c_int32, [_VP, C.c_uint32, _FP, C.c_uint32]),
    "output_levels": (C.c_int32, [_VP, _VP]),
    "output_level_series": (C.c_int32, [_VP, _FP, _DP]),
    "download_all_pcm16_gain": (C.c_int32, [_VP, C.POINTER(C.c_int16), _FP]),
    "output_loudness": (C.c_int32, [_VP, _DP, _VP]),
    "output_loudness_series": (C.c_int32, [_VP, _DP]),
    "loudness_hop": (C.c_uint32, [C.c_double]),
    "loudness_from_series": (C.c_int32, [_DP, C.c_uint32, C.c_uint32, C.c_uint32, _DP, _VP]),
}


class LevelStats(C.Structure):  # waa_level_stats (include/waa_hip_device.h): one per (instance, output channel)
    _fields_ = [("sum_sq", C.c_double), ("n_nonfinite", C.c_uint64), ("first_nonfinite", C.c_uint64), ("n_clipped", C.c_uint64),
                ("peak", C.c_float), ("reserved", C.c_uint32)]


# the same 40 bytes as a numpy record (OfflineAudioContext.output_levels)
LEVEL_STATS_DTYPE = np.dtype([("sum_sq", np.float64), ("n_nonfinite", np.uint64), ("first_nonfinite", np.uint64), ("n_clipped", np.uint64),
                              ("peak", np.float32), ("reserved", np.uint32)])


class LoudnessStats(C.Structure):  # waa_loudness_stats (include/waa_hip_device.h): one per instance
    _fields_ = [("integrated", C.c_double), ("momentary_max", C.c_double), ("short_term_max", C.c_double),
                ("relative_threshold", C.c_double), ("n_blocks", C.c_uint32), ("n_gated", C.c_uint32)]


# the same 40 bytes as a numpy record (OfflineAudioContext.output_loudness)
LOUDNESS_STATS_DTYPE = np.dtype([("integrated", np.float64), ("momentary_max", np.float64), ("short_term_max", np.float64),
                                 ("relative_threshold", np.float64), ("n_blocks", np.uint32), ("n_gated", np.uint32)])


def _weights_arg(weights, n_channels):
    """(array kept alive, pointer or None) for a `const double* weights` argument"""
    if weights is None:
        return None, None
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (n_channels,):
        raise ValueError(f"weights: expected {n_channels} values, one per channel (got shape {w.shape})")
    return w, w.ctypes.data_as(_DP)


def loudness_from_series(z, hop, weights=None, binding=None) -> np.ndarray:
    """waa_loudness_from_series: the loudness record (LOUDNESS_STATS_DTYPE, shape ()) of ONE context from its sub-block energies
    z[n_channels, n_sub] and the sub-block's length in frames — host arithmetic, no batch and no device."""
    if binding is None:
        from . import default_binding  # loads libwaa_hip.so; raises if it is not built
        binding = default_binding()
    b = binding
    if b.prefix != "waa_":
        raise WaaError(4, "loudness_from_series is a feature of the device library; this binding hands back f32 planes and nothing else")
    z = np.ascontiguousarray(z, dtype=np.float64)
    if z.ndim != 2:
        raise ValueError(f"z: expected [n_channels, n_sub] (got shape {z.shape})")
    w, wp = _weights_arg(weights, z.shape[0])
    out = np.zeros((), LOUDNESS_STATS_DTYPE)
    b.check(b.loudness_from_series(z.ctypes.data_as(_DP), z.shape[0], z.shape[1], int(hop), wp, out.ctypes.data_as(_VP)))
    return out


class PannerOptions(C.Structure):  # waa_panner_options (include/waa_hip_device.h)
    _fields_ = [("distance_model", C.c_int32), ("reserved", C.c_int32), ("ref_distance", C.c_double), ("max_distance", C.c_double),
                ("rolloff_factor", C.c_double), ("cone_inner_angle", C.c_double), ("cone_outer_angle", C.c_double),
                ("cone_outer_gain", C.c_double)]


class Binding:
    """ctypes view of one C-ABI library (prefix ``waa_`` for the product)."""

    def __init__(self, lib: C.CDLL, prefix: str):
        self.lib = lib
        self.prefix = prefix
        for name, (restype, argtypes) in ABI.items():
            fn = getattr(lib, prefix + name)  # AttributeError if the symbol is missing: fail loudly
            fn.restype = restype
            fn.argtypes = argtypes
            setattr(self, name, fn)
        # the device library's own entry points: bound where the library exports them (another binding, or a build of the device
        # library from before an entry point existed, does not), an AttributeError on first use otherwise
        for name, (restype, argtypes) in ABI_DEVICE.items():
            fn = getattr(lib, prefix + name, None) if prefix == "waa_" else None
            if fn is not None:
                fn.restype = restype
                fn.argtypes = argtypes
                setattr(self, name, fn)

    def __getattr__(self, name):
        if name in ABI_DEVICE:
            raise AttributeError(f"{self.prefix}{name} is an entry point of the device library that this binding's library does not export")
        raise AttributeError(name)

    def check(self, status: int):
        if status != 0:
            msg = self.last_error()
            raise WaaError(status, msg.decode() if msg else f"status {status}")


def bind(lib: C.CDLL, prefix: str = "waa_") -> Binding:
    return Binding(lib, prefix)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a: np.ndarray):
    return a.ctypes.data_as(_FP)


def _chan_ptrs(arr2d: np.ndarray):
    ptrs = (_FP * arr2d.shape[0])()
    for c in range(arr2d.shape[0]):
        ptrs[c] = arr2d[c].ctypes.data_as(_FP)
    return ptrs


class AudioBuffer:
    """src/buffer.rs:69 — channels x frames of f32 plus a sample rate."""

    def __init__(self, data, sample_rate: float):
        data = _f32(data)
        if data.ndim == 1:
            data = data[None, :]
        self.data = data
        self.sample_rate = float(np.float32(sample_rate))

    @property
    def number_of_channels(self) -> int:
        return self.data.shape[0]

    @property
    def length(self) -> int:
        return self.data.shape[1]

    @property
    def duration(self) -> float:
        return self.length / self.sample_rate

    def get_channel_data(self, c: int) -> np.ndarray:
        return self.data[c]


class AudioParam:
    """Value source for one AudioParam of one node (src/param.rs:268).

    Constants, explicit per-quantum value blocks and automation events all cross the C ABI; the timeline itself is
    evaluated by the library on the host (automation is control-side work)."""

    def __init__(self, node: "AudioNode", pid: int, default: float):
        self._node, self._pid = node, pid
        self._const = {ALL: float(default)}
        self._blocks = []
        self._events = []

    def _ctx(self):
        """the context whose control clock this param follows (an AudioListener's params: the listener's context)"""
        return self._node.context if self._node is not None else getattr(self, "_listener_ctx", None)

    def _owner_ids(self, ctx):
        """the node ids the param is addressed through (the listener's nine params: every PannerNode, like AudioListener::_apply)"""
        if self._node is not None:
            return [self._node.id]
        return [nd.id for nd in ctx._nodes if nd.kind == NODE_PANNER]

    @property
    def value(self) -> float:
        return self._const[ALL]

    @value.setter
    def value(self, v: float):
        self.set_value(v)

    def set_value(self, v: float, instance: int = ALL):
        ctx = self._ctx()
        if ctx is not None and ctx._now_q > 0:  # inside a suspend_sync callback: a SetValue event the render thread handles at that quantum
            pid, v = self._pid, float(v)
            for nid in self._owner_ids(ctx):
                ctx._log(lambda b, h, nid=nid: b.check(b.set_param_const(h, nid, pid, instance, v)))
            return self
        self._const[instance] = float(v)
        if instance == ALL:
            self._const = {ALL: float(v)}
        return self

    def set_block(self, quantum0: int, values, instance: int = ALL):
        """values: [n_quanta] (k-rate, len-1 slices) or [n_quanta, 128] (a-rate slices)."""
        v = _f32(values)
        if v.ndim == 1:
            v = v[:, None]
        assert v.shape[1] in (1, RENDER_QUANTUM_SIZE)
        self._blocks.append((int(quantum0), v, instance))
        return self

    # -- automation methods (src/param.rs:428-596).  The events cross the ABI (waa_param_schedule_event) and are
    #    evaluated by the library's restatement of AudioParamProcessor; nothing is computed in this mirror.
    #    `instance`: the context of the batch the call is made on (ALL = the same call on every context).
    def _event(self, kind: int, value: float, time: float, aux: float = 0.0, curve=None, instance: int = ALL):
        ev = (kind, float(value), float(time), float(aux), None if curve is None else _f32(curve), instance)
        ctx = self._ctx()
        if ctx is not None and ctx._now_q > 0:  # inside a suspend_sync callback
            pid = self._pid
            for nid in self._owner_ids(ctx):
                ctx._log(lambda b, h, nid=nid: b.check(b.param_schedule_event(h, nid, pid, ev[5], ev[0], ev[1], ev[2], ev[3],
                                                                              None if ev[4] is None else _fp(ev[4]), 0 if ev[4] is None else ev[4].size)))
            return self
        self._events.append(ev)
        return self

    def set_value_at_time(self, value: float, start_time: float, instance: int = ALL):
        return self._event(EVENT_SET_VALUE_AT_TIME, value, start_time, instance=instance)

    def linear_ramp_to_value_at_time(self, value: float, end_time: float, instance: int = ALL):
        return self._event(EVENT_LINEAR_RAMP, value, end_time, instance=instance)

    def exponential_ramp_to_value_at_time(self, value: float, end_time: float, instance: int = ALL):
        return self._event(EVENT_EXPONENTIAL_RAMP, value, end_time, instance=instance)

    def set_target_at_time(self, value: float, start_time: float, time_constant: float, instance: int = ALL):
        return self._event(EVENT_SET_TARGET, value, start_time, time_constant, instance=instance)

    def cancel_scheduled_values(self, cancel_time: float, instance: int = ALL):
        return self._event(EVENT_CANCEL_SCHEDULED_VALUES, 0.0, cancel_time, instance=instance)

    def cancel_and_hold_at_time(self, cancel_time: float, instance: int = ALL):
        return self._event(EVENT_CANCEL_AND_HOLD, 0.0, cancel_time, instance=instance)

    def set_value_curve_at_time(self, values, start_time: float, duration: float, instance: int = ALL):
        return self._event(EVENT_SET_VALUE_CURVE, 0.0, start_time, duration, values, instance=instance)

    def _apply(self, ctx: "OfflineAudioContext", node_id=None, pid=None):
        b, h = ctx._b, ctx._handle
        node_id = self._node.id if node_id is None else node_id
        pid = self._pid if pid is None else pid
        for inst, v in sorted(self._const.items(), key=lambda kv: kv[0] != ALL):
            b.check(b.set_param_const(h, node_id, pid, inst, v))
        for q0, v, inst in self._blocks:
            b.check(b.set_param_block(h, node_id, pid, inst, q0, v.shape[0], v.shape[1], _fp(v)))
        for kind, value, time, aux, curve, inst in self._events:  # in call order, like the reference's message queue
            b.check(b.param_schedule_event(h, node_id, pid, inst, kind, value, time, aux,
                                           None if curve is None else _fp(curve), 0 if curve is None else curve.size))


class AudioNode:
    kind = -1
    default_channel_config = (2, "max", "speakers")
    # AudioNode::number_of_inputs / number_of_outputs as far as connect() looks at them: one port each, except the
    # ChannelSplitterNode's outputs and the ChannelMergerNode's inputs
    number_of_inputs = 1
    number_of_outputs = 1

    def __init__(self, ctx: "OfflineAudioContext", channel_count=None, channel_count_mode=None,
                 channel_interpretation=None):
        self.context = ctx
        cc, mode, interp = self.default_channel_config
        self.channel_count = cc if channel_count is None else channel_count
        self.channel_count_mode = mode if channel_count_mode is None else channel_count_mode
        self.channel_interpretation = interp if channel_interpretation is None else channel_interpretation
        self._explicit_config = not (channel_count is None and channel_count_mode is None and
                                     channel_interpretation is None)
        self.params: List[AudioParam] = []
        self.id = ctx._register(self)

    # AudioNode channel config setters (audio_node.rs:296-340)
    def set_channel_count(self, v: int):
        self.channel_count = int(v)
        self._explicit_config = True

    def set_channel_count_mode(self, v: str):
        self.channel_count_mode = v
        self._explicit_config = True

    def set_channel_interpretation(self, v: str):
        self.channel_interpretation = v
        self._explicit_config = True

    # AudioNode::connect (audio_node.rs:247): returns the destination node for chaining
    def connect(self, dest, output: int = 0, input: int = 0):
        """AudioNode::connect; `dest` may be an AudioParam (audio-rate modulation, src/param.rs:300-320)."""
        if isinstance(dest, AudioParam):
            if dest._node.context is not self.context:
                raise WaaError(1, "InvalidAccessError - Attempting to connect nodes from different contexts")
            if not 0 <= output < self.number_of_outputs:  # param.rs connect: the same assertion on the output port
                raise WaaError(1, f"IndexSizeError - output port {output} is out of bounds")
            self.context._connect((self.id, output, dest._node.id, PARAM_INPUT | dest._pid))
            return dest
        if dest.context is not self.context:
            raise WaaError(1, "InvalidAccessError - Attempting to connect nodes from different contexts")
        if not 0 <= output < self.number_of_outputs:  # audio_node.rs:270-279
            raise WaaError(1, f"IndexSizeError - output port {output} is out of bounds")
        if not 0 <= input < dest.number_of_inputs:
            raise WaaError(1, f"IndexSizeError - input port {input} is out of bounds")
        self.context._connect((self.id, output, dest.id, input))
        return dest

    # AudioNode::disconnect and its four narrower forms (audio_node.rs:291-420); `dest` may be an AudioParam
    def disconnect(self, dest=None, output: Optional[int] = None, input: Optional[int] = None):
        if dest is not None:
            dctx = dest._node.context if isinstance(dest, AudioParam) else dest.context
            if dctx is not self.context:
                raise WaaError(1, "InvalidAccessError - Attempting to disconnect nodes from different contexts")
        if output is not None and not 0 <= output < self.number_of_outputs:
            raise WaaError(1, f"IndexSizeError - output port {output} is out of bounds")
        to = None if dest is None else (dest._node.id if isinstance(dest, AudioParam) else dest.id)
        ti = None if dest is None else (PARAM_INPUT | dest._pid if isinstance(dest, AudioParam) else input)
        self.context._disconnect(self.id, output, to, ti)

    def disconnect_dest(self, dest):
        self.disconnect(dest)

    def disconnect_output(self, output: int):
        self.disconnect(None, output)

    def disconnect_dest_from_output(self, dest, output: int):
        self.disconnect(dest, output)

    def disconnect_dest_from_output_to_input(self, dest, output: int, input: int):
        n_in = 1 if isinstance(dest, AudioParam) else dest.number_of_inputs
        if not 0 <= input < n_in:
            raise WaaError(1, f"IndexSizeError - input port {input} is out of bounds")
        self.disconnect(dest, output, input)

    def _desc(self) -> NodeDesc:
        d = NodeDesc()
        d.kind = self.kind
        if self._explicit_config:
            d.channel_count = self.channel_count
            d.channel_count_mode = COUNT_MODE[self.channel_count_mode]
            d.channel_interpretation = INTERPRETATION[self.channel_interpretation]
        self._fill_desc(d)
        return d

    def _fill_desc(self, d: NodeDesc):
        pass

    def _apply(self, ctx: "OfflineAudioContext"):
        for p in self.params:
            p._apply(ctx)


class AudioDestinationNode(AudioNode):
    kind = NODE_DESTINATION

    def __init__(self, ctx):
        # destination.rs:103-107: count = context channels, Explicit, Speakers
        self.default_channel_config = (ctx.number_of_channels, "explicit", "speakers")
        super().__init__(ctx)


class _ScheduledSource(AudioNode):
    def __init__(self, ctx, **kw):
        super().__init__(ctx, **kw)
        self._starts = {}
        self._stops = {}
        self._late = set()

    def start(self):
        return self.start_at(0.0)

    def start_at(self, when: float, instance: int = ALL):
        return self.start_at_with_offset_and_duration(when, 0.0, F64_MAX, instance)

    def start_at_with_offset(self, when: float, offset: float, instance: int = ALL):
        return self.start_at_with_offset_and_duration(when, offset, F64_MAX, instance)

    def start_at_with_offset_and_duration(self, when: float, offset: float, duration: float, instance: int = ALL):
        if instance in self._starts or ALL in self._starts:
            raise WaaError(3, "InvalidStateError - Cannot call `start` twice")
        self._starts[instance] = (float(when), float(offset), float(duration))
        ctx = self.context
        if ctx._now_q > 0:  # inside a suspend_sync callback: the start message is handled in front of that quantum
            nid, args = self.id, self._starts[instance]
            self._late.add(("start", instance))
            ctx._log(lambda b, h: b.check(b.source_start(h, nid, instance, *args)))
        return self

    def stop(self):
        return self.stop_at(0.0)

    def stop_at(self, when: float, instance: int = ALL):
        if instance not in self._starts and ALL not in self._starts:
            raise WaaError(3, "InvalidStateError - cannot stop before start")
        self._stops[instance] = float(when)
        ctx = self.context
        if ctx._now_q > 0:
            nid, w = self.id, float(when)
            self._late.add(("stop", instance))
            ctx._log(lambda b, h: b.check(b.source_stop(h, nid, instance, w)))
        return self

    def ended_quantum(self, instance: int = 0) -> int:
        """When the reference fires `onended` (scheduled_source.rs:44) for this source of `instance`: the index of
        the render quantum after which the event is dispatched, ENDED_AT_UNLOAD (after the last quantum, from
        before_drop) or ENDED_NEVER.  Call after the render."""
        ctx = self.context
        q = C.c_int64()
        ctx._b.check(ctx._b.source_ended(ctx._handle, self.id, instance, C.byref(q)))
        return q.value

    def _apply(self, ctx):
        super()._apply(ctx)
        b, h = ctx._b, ctx._handle
        for inst, (w, o, d) in self._starts.items():
            if ("start", inst) not in self._late:  # (calls made at a suspend point are replayed from the control log)
                b.check(b.source_start(h, self.id, inst, w, o, d))
        for inst, w in self._stops.items():
            if ("stop", inst) not in self._late:
                b.check(b.source_stop(h, self.id, inst, w))


class AudioBufferSourceNode(_ScheduledSource):
    kind = NODE_BUFFER_SOURCE

    def __init__(self, ctx, **kw):
        super().__init__(ctx, **kw)
        self.playback_rate = AudioParam(self, 0, 1.0)
        self.detune = AudioParam(self, 1, 0.0)
        self.params = [self.playback_rate, self.detune]
        self._buffers = {}
        self._batch = None
        self._pcm = None
        self._pcm_one = {}
        self._device = None
        self._loop = {}

    def set_buffer(self, buffer: AudioBuffer, instance: int = ALL):
        self._buffers[instance] = buffer
        return self

    def set_buffer_batch(self, data, sample_rate: float):
        """data: [n_instances, channels, frames], distinct per instance."""
        self._batch = (_f32(data), float(np.float32(sample_rate)))
        return self

    def set_buffer_pcm16_batch(self, pcm, sample_rate: float):
        """decode_audio_data_sync for decoded 16-bit PCM: pcm = [n_instances, frames, channels] int16 (interleaved); the
        sample conversion and the resampling to the context's rate run in the library (on the device)."""
        self._pcm = (np.ascontiguousarray(pcm, dtype=np.int16), float(np.float32(sample_rate)))
        return self

    def set_buffer_pcm16(self, pcm, sample_rate: float, instance: int = ALL):
        """pcm = [frames, channels] int16 for one instance (or all)."""
        self._pcm_one[instance] = (np.ascontiguousarray(pcm, dtype=np.int16), float(np.float32(sample_rate)))
        return self

    def adopt_device_buffer(self, device_ptr: int, n_channels: int, frames: int, sample_rate: float):
        """device_ptr: address of a resident [n_instances, channels, frames] f32 device array."""
        self._device = (int(device_ptr), int(n_channels), int(frames), float(np.float32(sample_rate)))
        return self

    def set_loop(self, value: bool, instance: int = ALL):
        self._loop.setdefault(instance, [False, 0.0, 0.0])[0] = bool(value)
        return self

    def set_loop_start(self, value: float, instance: int = ALL):
        self._loop.setdefault(instance, [False, 0.0, 0.0])[1] = float(value)
        return self

    def set_loop_end(self, value: float, instance: int = ALL):
        self._loop.setdefault(instance, [False, 0.0, 0.0])[2] = float(value)
        return self

    def _apply(self, ctx):
        b, h = ctx._b, ctx._handle
        if self._device is not None:
            p, nch, frames, sr = self._device
            b.check(b.source_adopt_device(h, self.id, p, nch, frames, sr))
        if self._batch is not None:
            data, sr = self._batch
            assert data.ndim == 3 and data.shape[0] == ctx.n_instances
            b.check(b.source_set_buffer_batch(h, self.id, _fp(data), data.shape[1], data.shape[2], sr))
        _I16 = C.POINTER(C.c_int16)
        if self._pcm is not None:
            pcm, sr = self._pcm
            assert pcm.ndim == 3 and pcm.shape[0] == ctx.n_instances
            b.check(b.source_set_buffer_pcm16_batch(h, self.id, pcm.ctypes.data_as(_I16), pcm.shape[2], pcm.shape[1], sr))
        for inst, (pcm, sr) in sorted(self._pcm_one.items(), key=lambda kv: kv[0] != ALL):
            b.check(b.source_set_buffer_pcm16(h, self.id, inst, pcm.ctypes.data_as(_I16), pcm.shape[1], pcm.shape[0], sr))
        for inst, buf in sorted(self._buffers.items(), key=lambda kv: kv[0] != ALL):
            b.check(b.source_set_buffer(h, self.id, inst, _chan_ptrs(buf.data), buf.number_of_channels, buf.length,
                                        buf.sample_rate))
        for inst, (lp, ls, le) in sorted(self._loop.items(), key=lambda kv: kv[0] != ALL):
            b.check(b.source_set_loop(h, self.id, inst, int(lp), ls, le))
        super()._apply(ctx)


class ConstantSourceNode(_ScheduledSource):
    kind = NODE_CONSTANT_SOURCE

    def __init__(self, ctx, offset: float = 1.0, **kw):
        super().__init__(ctx, **kw)
        self.offset = AudioParam(self, 0, offset)
        self.params = [self.offset]


class PeriodicWave:
    """src/periodic_wave.rs:35-190: PeriodicWaveOptions{real, imag, disable_normalization}; the 8192-point table is
    generated by the library when the wave is set on an oscillator."""

    def __init__(self, ctx=None, real=None, imag=None, disable_normalization: bool = False):
        if real is None and imag is None:  # defaults to a sine wave (periodic_wave.rs:140-143)
            real, imag = [0.0, 0.0], [0.0, 1.0]
        r = None if real is None else _f32(real).reshape(-1)
        i = None if imag is None else _f32(imag).reshape(-1)
        if r is not None and i is not None and r.size != i.size:
            raise WaaError(1, "IndexSizeError - `real` and `imag` length should be equal")
        n = (r if r is not None else i).size
        if n < 2:
            raise WaaError(1, "IndexSizeError - `real` and `imag` length should at least 2")
        self.real = r if r is not None else np.zeros(n, np.float32)
        self.imag = i if i is not None else np.zeros(n, np.float32)
        self.disable_normalization = bool(disable_normalization)
        self.table = None

    @classmethod
    def from_wavetable(cls, table):
        """A PeriodicWave that already IS its 8192-point table — what the reference's render side holds (periodic_wave.rs:72-74,
        oscillator.rs:487-493) and what the Rust shim forwards (waa_oscillator_set_wavetable)."""
        t = _f32(table).reshape(-1)
        if t.size != 8192:
            raise WaaError(1, f"IndexSizeError - a PeriodicWave table has 8192 points (got {t.size})")
        w = cls()
        w.table = t
        return w


class OscillatorNode(_ScheduledSource):
    """src/node/oscillator.rs:64-321 (OscillatorOptions{type = sine, frequency = 440, detune = 0, periodic_wave})"""

    kind = NODE_OSCILLATOR

    def __init__(self, ctx, type_="sine", frequency=440.0, detune=0.0, periodic_wave=None, **kw):
        super().__init__(ctx, **kw)
        if type_ == "custom" and periodic_wave is None:
            raise WaaError(3, "InvalidStateError: Custom type cannot be set manually")
        self.type_ = type_
        self.frequency = AudioParam(self, 0, frequency)
        self.detune = AudioParam(self, 1, detune)
        self.params = [self.frequency, self.detune]
        self.periodic_wave = None
        self._inst_waves = {}  # instance -> PeriodicWave: one wave per context (waa_oscillator_set_periodic_wave_instance)
        self._inst_types = {}  # instance -> built-in type name: one type per context (waa_oscillator_set_type_instance)
        if periodic_wave is not None:
            self.set_periodic_wave(periodic_wave)

    def set_type(self, type_: str, instance: int = ALL):
        """instance = ALL: the node's type, as before (ignored once the node is custom).  instance = i: context i's own built-in
        type (every context of the reference sets the type of its own node, oscillator.rs:305-330); the last call for an instance
        wins.  What a context renders with: type_of."""
        if type_ == "custom":  # oscillator.rs:305-309
            raise WaaError(3, "InvalidStateError: Custom type cannot be set manually")
        if instance == ALL:
            if self.type_ != "custom":  # ignored once a periodic wave is set (oscillator.rs:311-314)
                self.type_ = type_
            return self
        if type_ not in OSCILLATOR_TYPE:
            raise WaaError(1, "bad oscillator type")
        if self.context._handle is not None:
            raise WaaError(3, "InvalidStateError - the batch is frozen once rendering has started")
        if not 0 <= int(instance) < self.context.n_instances:
            raise WaaError(1, f"instance {instance} out of range")
        self._inst_types[int(instance)] = type_
        return self

    def set_type_batch(self, types):
        """types: a sequence of n_instances built-in type names, one per context"""
        n = self.context.n_instances
        if len(types) != n:
            raise WaaError(1, f"set_type_batch takes n_instances = {n} types, got {len(types)}")
        for i, t in enumerate(types):
            self.set_type(t, instance=i)
        return self

    def type_of(self, instance: int) -> str:
        """The type context `instance` renders with, resolved as the device library's plan resolves it: its own PeriodicWave
        (custom; a type given to it is ignored), its own type (also where a shared wave exists), the shared wave (custom), the
        node's type.  A node with per-instance waves, no shared one and nothing for this instance: WaaError(3), the plan's refusal."""
        if not 0 <= int(instance) < self.context.n_instances:
            raise WaaError(1, f"instance {instance} out of range")
        i = int(instance)
        if i in self._inst_waves:
            return "custom"
        if i in self._inst_types:
            return self._inst_types[i]
        if self.periodic_wave is not None:
            return "custom"
        if self._inst_waves:
            raise WaaError(3, f"InvalidStateError - OscillatorNode {self.id} has no PeriodicWave for instance {i}")
        return self.type_

    def set_periodic_wave(self, wave: PeriodicWave, instance: int = ALL):
        """instance = ALL: the wave of every context without one of its own.  instance = i: context i's own PeriodicWave (coefficients
        or PeriodicWave.from_wavetable); the node then works in per-instance mode, and the device library generates the tables of
        the coefficient sets when the batch is planned.  Lengths may differ between contexts."""
        if instance == ALL:
            self.type_ = "custom"
            self.periodic_wave = wave
            return self
        if self.context._handle is not None:
            raise WaaError(3, "InvalidStateError - the batch is frozen once rendering has started")
        if not 0 <= int(instance) < self.context.n_instances:
            raise WaaError(1, f"instance {instance} out of range")
        self.type_ = "custom"
        self._inst_waves[int(instance)] = wave
        return self

    def set_periodic_wave_batch(self, real, imag=None, disable_normalization: bool = False):
        """real [n_instances, n] and / or imag [n_instances, n]: one PeriodicWave per context."""
        r = None if real is None else _f32(real)
        i = None if imag is None else _f32(imag)
        n = self.context.n_instances
        if (r is None and i is None) or any(a is not None and (a.ndim != 2 or a.shape[0] != n) for a in (r, i)):
            raise WaaError(1, f"set_periodic_wave_batch takes [n_instances = {n}, n] arrays for real and / or imag, got "
                              f"{None if r is None else r.shape} and {None if i is None else i.shape}")
        for k in range(n):
            self.set_periodic_wave(PeriodicWave(real=None if r is None else r[k], imag=None if i is None else i[k],
                                                disable_normalization=disable_normalization), instance=k)
        return self

    @property
    def per_instance(self) -> bool:
        return bool(self._inst_waves)

    def _check_per_instance(self):
        if self.context._b.prefix != "waa_":
            raise WaaError(4, "one PeriodicWave per instance is a feature of the device library; this binding keeps one wave "
                              "per batch (render it one context at a time)")

    def _check_per_instance_types(self):
        """another binding keeps one type per batch: types that all resolve equal go through as the shared option"""
        if self.context._b.prefix != "waa_" and len({self.type_of(i) for i in range(self.context.n_instances)}) > 1:
            raise WaaError(4, "one oscillator type per instance is a feature of the device library; this binding keeps one type "
                              "per batch (render it one context at a time)")

    def wavetable(self, instance: int = 0) -> np.ndarray:
        """The 8192-point table context `instance` renders with.  A node in per-instance mode is planned first (which freezes the
        batch): the answer is then the instance's row of the device's tables; otherwise, and on a plan-only context, the table
        built on the host."""
        self._check_per_instance()
        if not 0 <= int(instance) < self.context.n_instances:
            raise WaaError(1, f"instance {instance} out of range")
        ctx = self.context
        if self.per_instance:
            ctx.plan_describe()
        else:
            ctx.prepare()
        out = np.empty(8192, np.float32)
        ctx._b.check(ctx._b.oscillator_get_wavetable(ctx._handle, self.id, int(instance), _fp(out), out.size))
        return out

    def _fill_desc(self, d):
        d.i[0] = OSCILLATOR_TYPE[self.type_]
        if self.per_instance:
            self._check_per_instance()  # (refusals before the batch exists)
        if self._inst_types:
            self._check_per_instance_types()
            if self.context._b.prefix != "waa_" and self.type_of(0) != "custom":
                d.i[0] = OSCILLATOR_TYPE[self.type_of(0)]  # (equal types everywhere: the shared option)

    @staticmethod
    def _set_wave(b, h, node, w, *inst):
        if w.table is not None:
            fn = b.oscillator_set_wavetable_instance if inst else b.oscillator_set_wavetable
            b.check(fn(h, node, *inst, _fp(w.table), w.table.size))
        else:
            fn = b.oscillator_set_periodic_wave_instance if inst else b.oscillator_set_periodic_wave
            b.check(fn(h, node, *inst, _fp(w.real), _fp(w.imag), w.real.size, int(w.disable_normalization)))

    def _apply(self, ctx):
        super()._apply(ctx)
        b, h = ctx._b, ctx._handle
        # another binding with own types: they are all equal (_fill_desc) and went through as the shared option; where that type is
        # built-in it outranks a shared wave in every context, so no wave is sent
        send_waves = not (self._inst_types and b.prefix != "waa_" and self.type_of(0) != "custom")
        if self._inst_types and b.prefix == "waa_":
            for i, t in sorted(self._inst_types.items()):
                b.check(b.oscillator_set_type_instance(h, self.id, i, OSCILLATOR_TYPE[t]))
        if send_waves and self.periodic_wave is not None:
            self._set_wave(b, h, self.id, self.periodic_wave)
        if send_waves and self.per_instance:
            self._check_per_instance()
            for i, w in sorted(self._inst_waves.items()):
                self._set_wave(b, h, self.id, w, i)


class BiquadFilterNode(AudioNode):
    kind = NODE_BIQUAD

    def __init__(self, ctx, type_="lowpass", frequency=350.0, detune=0.0, q=1.0, gain=0.0, **kw):
        super().__init__(ctx, **kw)
        self.type_ = type_
        self._inst_types = {}  # instance -> type name: one type per context (waa_biquad_set_type_instance)
        self.frequency = AudioParam(self, 0, frequency)
        self.detune = AudioParam(self, 1, detune)
        self.q = AudioParam(self, 2, q)
        self.gain = AudioParam(self, 3, gain)
        self.params = [self.frequency, self.detune, self.q, self.gain]

    def set_type(self, type_: str, instance: int = ALL):
        """instance = ALL: the type of every context without one of its own.  instance = i: context i's own type (every context of
        the reference sets the type of its own node, biquad_filter.rs:901-906).  May be called any number of times; the last call
        for an instance wins.  The two forms differ in their refusals: the per-instance form refuses an unknown name ("bad biquad
        type"), an instance out of range and a call after the batch exists (InvalidStateError) at once; the ALL form is as it was
        before instances had types — the name is looked up when the batch is created (an unknown one is a KeyError there), and a
        call after that is not refused and is not sent to the batch that exists."""
        if instance == ALL:
            self.type_ = type_
            return self
        if type_ not in BIQUAD_TYPE:
            raise WaaError(1, "bad biquad type")
        if self.context._handle is not None:
            raise WaaError(3, "InvalidStateError - the batch is frozen once rendering has started")
        if not 0 <= int(instance) < self.context.n_instances:
            raise WaaError(1, f"instance {instance} out of range")
        self._inst_types[int(instance)] = type_
        return self

    def set_type_batch(self, types):
        """types: a sequence of n_instances type names, one per context"""
        n = self.context.n_instances
        if len(types) != n:
            raise WaaError(1, f"set_type_batch takes n_instances = {n} types, got {len(types)}")
        for i, t in enumerate(types):
            self.set_type(t, instance=i)
        return self

    def type_of(self, instance: int) -> str:
        """the type context `instance` renders with: its own, or the shared one"""
        if not 0 <= int(instance) < self.context.n_instances:
            raise WaaError(1, f"instance {instance} out of range")
        return self._inst_types.get(int(instance), self.type_)

    @property
    def per_instance(self) -> bool:
        return bool(self._inst_types)

    def _types_differ(self) -> bool:
        return len({self.type_of(i) for i in range(self.context.n_instances)}) > 1 if self._inst_types else False

    def _check_per_instance(self):
        if self._types_differ() and self.context._b.prefix != "waa_":
            raise WaaError(4, "one filter type per instance is a feature of the device library; this binding keeps one type "
                              "per batch (render it one context at a time)")

    def _fill_desc(self, d):
        d.i[0] = BIQUAD_TYPE[self.type_]
        if self.per_instance:
            self._check_per_instance()  # (refusals before the batch exists)
            if self.context._b.prefix != "waa_":
                d.i[0] = BIQUAD_TYPE[self.type_of(0)]  # (equal types everywhere: the shared option)

    def _apply(self, ctx):
        super()._apply(ctx)
        if self.per_instance and ctx._b.prefix == "waa_":
            b, h = ctx._b, ctx._handle
            for i, t in sorted(self._inst_types.items()):
                b.check(b.biquad_set_type_instance(h, self.id, i, BIQUAD_TYPE[t]))

    def get_frequency_response(self, frequency_hz, instance: int = ALL) -> tuple:
        """instance = i: the response of context i's filter — its type and its constants (or the ALL ones where it has none)"""
        type_ = self.type_
        pv = [p._const[ALL] for p in self.params]
        if instance != ALL:
            type_ = self.type_of(instance)
            pv = [p._const.get(int(instance), p._const[ALL]) for p in self.params]
        hz = _f32(frequency_hz)
        mag = np.empty_like(hz)
        phase = np.empty_like(hz)
        b = self.context._b
        b.check(b.biquad_frequency_response(BIQUAD_TYPE[type_], self.context.sample_rate, pv[0], pv[1], pv[2], pv[3], _fp(hz), _fp(mag),
                                            _fp(phase), hz.size))
        return mag, phase


class GainNode(AudioNode):
    kind = NODE_GAIN

    def __init__(self, ctx, gain: float = 1.0, **kw):
        super().__init__(ctx, **kw)
        self.gain = AudioParam(self, 0, gain)
        self.params = [self.gain]


class ConvolverNode(AudioNode):
    kind = NODE_CONVOLVER
    default_channel_config = (2, "clamped-max", "speakers")

    def __init__(self, ctx, buffer: Optional[AudioBuffer] = None, disable_normalization: bool = False, **kw):
        super().__init__(ctx, **kw)
        self.normalize = not disable_normalization
        self.buffer = None
        self._inst_buffers = {}  # instance -> AudioBuffer: one impulse response per context (waa_node_desc.i[1] = 1)
        self._normalize_at_set = self.normalize
        if buffer is not None:
            self.set_buffer(buffer)

    def set_normalize(self, value: bool):
        self.normalize = bool(value)

    def set_buffer(self, buffer: AudioBuffer, instance: int = ALL):
        """instance = ALL: the impulse response of every context.  instance = i: context i's own response — every context of
        the reference owns its ConvolverNode and its buffer.  As soon as one instance has its own response the node works in
        per-instance mode; instances without one use the ALL buffer.  All responses of a node share channel count and length
        (pad shorter ones with zeros; the normalisation then sees the padded length)."""
        if buffer.sample_rate != self.context.sample_rate:
            raise WaaError(2, "NotSupportedError - sample rate of the convolution buffer must match the audio context")
        if buffer.number_of_channels not in (1, 2, 4):
            raise WaaError(2, "NotSupportedError - the convolution buffer must consist of 1, 2 or 4 channels")
        if instance == ALL:
            self.buffer = buffer
        else:
            if not 0 <= int(instance) < self.context.n_instances:
                raise WaaError(1, f"instance {instance} out of range")
            self._inst_buffers[int(instance)] = buffer
        self._normalize_at_set = self.normalize
        return self

    def set_buffer_batch(self, data, sample_rate: float):
        """data: [n_instances, channels, frames] — one impulse response per context."""
        data = _f32(data)
        if data.ndim != 3 or data.shape[0] != self.context.n_instances:
            raise WaaError(1, f"set_buffer_batch takes [n_instances = {self.context.n_instances}, channels, frames], got {data.shape}")
        for i in range(data.shape[0]):
            self.set_buffer(AudioBuffer(data[i], sample_rate), instance=i)
        return self

    @property
    def per_instance(self) -> bool:
        return bool(self._inst_buffers)

    def _instance_buffers(self):
        """The response of every context in per-instance mode; WaaError(4) for what the batch cannot express."""
        if self.context._b.prefix != "waa_":
            raise WaaError(4, "one impulse response per instance is a feature of the device library; this binding keeps one response "
                              "per batch (render it one context at a time)")
        bufs = [self._inst_buffers.get(i, self.buffer) for i in range(self.context.n_instances)]
        for i, bf in enumerate(bufs):
            if bf is None:
                raise WaaError(4, f"ConvolverNode in per-instance mode: instance {i} has no impulse response (set one for it, or one for ALL)")
        for i, bf in enumerate(bufs):
            if bf.number_of_channels != bufs[0].number_of_channels:
                raise WaaError(4, f"per-instance impulse responses must share the channel count: instance {i} has "
                                  f"{bf.number_of_channels}, instance 0 has {bufs[0].number_of_channels}")
            if bf.length != bufs[0].length:
                raise WaaError(4, f"per-instance impulse responses must share the length (pad with zeros): instance {i} has "
                                  f"{bf.length} frames, instance 0 has {bufs[0].length}")
        return bufs

    def set_buffer_pcm16(self, pcm, sample_rate: float):
        """decode_audio_data_sync + set_buffer: pcm = [frames, channels] int16 at `sample_rate`; decoded and resampled to
        the context's rate by the library (on the device)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        if pcm.shape[1] not in (1, 2, 4):
            raise WaaError(2, "NotSupportedError - the convolution buffer must consist of 1, 2 or 4 channels")
        self._pcm = (pcm, float(np.float32(sample_rate)))
        self._normalize_at_set = self.normalize
        return self

    def _fill_desc(self, d):
        d.i[0] = 0 if self._normalize_at_set else 1
        if self.per_instance:
            self._instance_buffers()  # (refusals before the batch exists)
            d.i[1] = 1

    def _apply(self, ctx):
        if self.per_instance:
            if getattr(self, "_pcm", None) is not None:
                raise WaaError(4, "16-bit impulse responses per instance are out of scope")
            bufs = self._instance_buffers()
            nch = bufs[0].number_of_channels
            table = (_FP * (len(bufs) * nch))()  # [instance][channel]
            for i, bf in enumerate(bufs):
                for c in range(nch):
                    table[i * nch + c] = bf.data[c].ctypes.data_as(_FP)
            ctx._b.check(ctx._b.convolver_set_buffer(ctx._handle, self.id, table, nch, bufs[0].length, bufs[0].sample_rate))
            return
        if getattr(self, "_pcm", None) is not None:
            pcm, sr = self._pcm
            ctx._b.check(ctx._b.convolver_set_buffer_pcm16(ctx._handle, self.id, pcm.ctypes.data_as(C.POINTER(C.c_int16)),
                                                           pcm.shape[1], pcm.shape[0], sr))
        if self.buffer is not None:
            b, h = ctx._b, ctx._handle
            buf = self.buffer
            b.check(b.convolver_set_buffer(h, self.id, _chan_ptrs(buf.data), buf.number_of_channels, buf.length,
                                           buf.sample_rate))


class StereoPannerNode(AudioNode):
    kind = NODE_STEREO_PANNER
    default_channel_config = (2, "clamped-max", "speakers")

    def __init__(self, ctx, pan: float = 0.0, **kw):
        super().__init__(ctx, **kw)
        self.pan = AudioParam(self, 0, pan)
        self.params = [self.pan]


class DynamicsCompressorNode(AudioNode):
    """src/node/dynamics_compressor.rs — the five k-rate AudioParams and the channel-config constraints; the node itself is
    rendered by the library (waa_compressor.hip), nothing is computed here.

    meter=True (the device library only) keeps `reduction()` after every render quantum of every context: `reduction_series()`
    is the whole trace, `reduction()` / `reduction_all()` its last row, as the reference's method returns it after the render."""
    kind = NODE_DYNAMICS_COMPRESSOR
    default_channel_config = (2, "clamped-max", "speakers")

    def __init__(self, ctx, attack: float = 0.003, knee: float = 30.0, ratio: float = 12.0, release: float = 0.25,
                 threshold: float = -24.0, meter: bool = False, **kw):
        self.meter = bool(meter)
        # DynamicsCompressorNode::new asserts both before anything else (dynamics_compressor.rs:184-185)
        self._assert_valid_channel_count(kw.get("channel_count") or 2)
        self._assert_valid_channel_count_mode(kw.get("channel_count_mode") or "clamped-max")
        super().__init__(ctx, **kw)
        self.threshold = AudioParam(self, 0, threshold)
        self.knee = AudioParam(self, 1, knee)
        self.ratio = AudioParam(self, 2, ratio)
        self.attack = AudioParam(self, 3, attack)
        self.release = AudioParam(self, 4, release)
        self.params = [self.threshold, self.knee, self.ratio, self.attack, self.release]

    @staticmethod
    def _assert_valid_channel_count(count: int):  # dynamics_compressor.rs:72-79
        if int(count) > 2:
            raise WaaError(2, "NotSupportedError - DynamicsCompressorNode channel count cannot be greater than two")

    @staticmethod
    def _assert_valid_channel_count_mode(mode: str):  # dynamics_compressor.rs:88-96
        if mode == "max":
            raise WaaError(2, "NotSupportedError - DynamicsCompressorNode channel count mode cannot be set to max")

    def set_channel_count(self, v: int):
        self._assert_valid_channel_count(v)
        super().set_channel_count(v)

    def set_channel_count_mode(self, v: str):
        self._assert_valid_channel_count_mode(v)
        super().set_channel_count_mode(v)

    def _fill_desc(self, d):
        if self.meter and self.context._b.prefix != "waa_":
            raise WaaError(4, "the reduction meter of a DynamicsCompressorNode (meter=True) is a feature of the device library; this "
                              "binding keeps no trace")
        d.i[0] = 1 if self.meter else 0

    # -- reduction (dynamics_compressor.rs:304-306) --------------------------------------------------------------------
    def _metered(self):
        if not self.meter:
            raise ValueError("this DynamicsCompressorNode keeps no reduction: create it with meter=True")

    def _last_row(self, instance):
        """the value after the last rendered quantum: [n_instances] (instance None) or one float.  Before the render, outside a
        suspend callback: the reference's initial 0 (:249), without a library call; inside a suspend_sync callback at quantum
        q > 0: the value after quantum q - 1, from a prefix render like an analyser pull"""
        self._metered()
        ctx = self.context
        if ctx._now_q > 0 and ctx._handle is None:
            q = ctx._now_q
            with ctx._prefix_render(q):  # (a batch of q quanta: its last row is the value after quantum q - 1)
                return self._read_last(instance, q)
        if ctx._handle is None or not ctx._rendered:
            return 0.0 if instance is not None else np.zeros(ctx.n_instances, np.float32)
        return self._read_last(instance, (ctx.length + RENDER_QUANTUM_SIZE - 1) // RENDER_QUANTUM_SIZE)

    def _read_last(self, instance, n_quanta):
        ctx = self.context
        if instance is not None:
            v = C.c_float()
            ctx._b.check(ctx._b.compressor_get_reduction(ctx._handle, self.id, int(instance), C.byref(v)))
            return float(v.value)
        # (every context's last value in ONE transfer: the trace's last column)
        rows = np.zeros((ctx.n_instances, n_quanta), np.float32)
        ctx._b.check(ctx._b.compressor_get_reduction_series(ctx._handle, self.id, _fp(rows), n_quanta))
        return np.ascontiguousarray(rows[:, -1])

    def reduction(self, instance: int = 0) -> float:
        """DynamicsCompressorNode::reduction of one context: the gain reduction in dB after the last rendered quantum"""
        return self._last_row(int(instance))

    def reduction_all(self) -> np.ndarray:
        """[n_instances]: `reduction()` of every context"""
        return self._last_row(None)

    def reduction_series(self, out=None) -> np.ndarray:
        """[n_instances][n_quanta]: row q is what `reduction()` returns after render quantum q (one gather launch per render, kept
        on the device until it is read).  Only after start_rendering_sync."""
        self._metered()
        ctx = self.context
        if ctx._handle is None or ctx._now_q > 0:
            raise WaaError(3, "InvalidStateError - the reduction trace is only available after start_rendering_sync")
        n_quanta = (ctx.length + RENDER_QUANTUM_SIZE - 1) // RENDER_QUANTUM_SIZE
        shape = (ctx.n_instances, n_quanta)
        if out is None:
            out = np.zeros(shape, np.float32)
        if not isinstance(out, np.ndarray) or out.shape != shape or out.dtype != np.float32 or not out.flags.c_contiguous:
            # (the library writes n_quanta values per context through the raw pointer: a wrong buffer is a silent out-of-bounds write)
            raise ValueError(f"out: expected a C-contiguous float32 array of shape {shape}")
        ctx._b.check(ctx._b.compressor_get_reduction_series(ctx._handle, self.id, _fp(out), n_quanta))
        return out


class AudioListener:
    """src/spatial.rs:127-144 — shared by every PannerNode of the context."""

    def __init__(self):
        # nine a-rate AudioParams (spatial.rs:18-24 defaults); they cross the ABI through every PannerNode (params 6..14)
        names = ["position_x", "position_y", "position_z", "forward_x", "forward_y", "forward_z", "up_x", "up_y", "up_z"]
        self.params = [AudioParam(None, 6 + i, v) for i, v in enumerate([0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0])]
        for name, prm in zip(names, self.params):
            setattr(self, name, prm)

    @property
    def values(self):
        return [p.value for p in self.params]

    def set_position(self, x, y, z):
        for p, v in zip(self.params[0:3], (x, y, z)):
            p.set_value(v)

    def set_orientation(self, fx, fy, fz, ux, uy, uz):
        for p, v in zip(self.params[3:9], (fx, fy, fz, ux, uy, uz)):
            p.set_value(v)


class PannerNode(AudioNode):
    kind = NODE_PANNER
    default_channel_config = (2, "clamped-max", "speakers")

    def __init__(self, ctx, panning_model="equalpower", distance_model="inverse", position=(0.0, 0.0, 0.0),
                 orientation=(1.0, 0.0, 0.0), ref_distance=1.0, max_distance=10000.0, rolloff_factor=1.0,
                 cone_inner_angle=360.0, cone_outer_angle=360.0, cone_outer_gain=0.0, **kw):
        super().__init__(ctx, **kw)
        self.panning_model, self.distance_model = panning_model, distance_model
        self.ref_distance, self.max_distance, self.rolloff_factor = ref_distance, max_distance, rolloff_factor
        self.cone_inner_angle, self.cone_outer_angle, self.cone_outer_gain = (cone_inner_angle, cone_outer_angle,
                                                                              cone_outer_gain)
        self.position_x = AudioParam(self, 0, position[0])
        self.position_y = AudioParam(self, 1, position[1])
        self.position_z = AudioParam(self, 2, position[2])
        self.orientation_x = AudioParam(self, 3, orientation[0])
        self.orientation_y = AudioParam(self, 4, orientation[1])
        self.orientation_z = AudioParam(self, 5, orientation[2])
        self.params = [self.position_x, self.position_y, self.position_z, self.orientation_x, self.orientation_y,
                       self.orientation_z]
        self._inst_options = {}  # instance -> {field: value}: one option set per context (waa_panner_set_options_instance)

    OPTION_FIELDS = ("distance_model", "ref_distance", "max_distance", "rolloff_factor", "cone_inner_angle", "cone_outer_angle",
                     "cone_outer_gain")

    @staticmethod
    def _check_option_values(fields):
        """the refusals of waa_panner_set_options_instance, which are the reference's (panner.rs:408-428, :545-641)"""
        if "distance_model" in fields and fields["distance_model"] not in DISTANCE_MODEL:
            raise WaaError(1, "bad distance model")
        if "ref_distance" in fields and not fields["ref_distance"] >= 0.0:
            raise WaaError(1, "RangeError - refDistance cannot be negative")
        if "max_distance" in fields and not fields["max_distance"] > 0.0:
            raise WaaError(1, "RangeError - maxDistance must be strictly positive")
        if "rolloff_factor" in fields and not fields["rolloff_factor"] >= 0.0:
            raise WaaError(1, "RangeError - rolloffFactor cannot be negative")
        if "cone_outer_gain" in fields and not 0.0 <= fields["cone_outer_gain"] <= 1.0:
            raise WaaError(3, "InvalidStateError - coneOuterGain must be in the range [0, 1]")

    def set_options(self, instance: int = ALL, **fields):
        """fields: any of the constructor's option names (OPTION_FIELDS); another name is a TypeError.  instance = ALL: the options of
        every context without a value of its own — the plain attributes, as assigning them does (checked when the batch is created).
        instance = i: context i's own values for the given fields (every context of the reference builds its own PannerNode from its
        own PannerOptions, panner.rs:146-166); bad values, an unknown distance model, an instance out of range and a call after the
        batch exists (InvalidStateError) are refused at once.  May be called any number of times; for one instance and one field the
        last call wins.  The panning model is not an option of this kind: it stays one per node."""
        for name in fields:
            if name not in self.OPTION_FIELDS:
                raise TypeError(f"set_options() got an unexpected option '{name}' (the options are {', '.join(self.OPTION_FIELDS)})")
        if instance == ALL:
            for name, v in fields.items():
                setattr(self, name, v)
            return self
        self._check_option_values(fields)
        if self.context._handle is not None:
            raise WaaError(3, "InvalidStateError - the batch is frozen once rendering has started")
        if not 0 <= int(instance) < self.context.n_instances:
            raise WaaError(1, f"instance {instance} out of range")
        self._inst_options.setdefault(int(instance), {}).update(fields)
        return self

    def set_options_batch(self, options):
        """options: a sequence of n_instances dicts of option fields, one per context"""
        n = self.context.n_instances
        if len(options) != n:
            raise WaaError(1, f"set_options_batch takes n_instances = {n} option sets, got {len(options)}")
        for i, o in enumerate(options):
            self.set_options(instance=i, **o)
        return self

    def options_of(self, instance: int) -> dict:
        """the complete option set context `instance` renders with: the shared attributes overlaid with its own fields (resolved
        now: the order of the set_options calls does not matter)"""
        if not 0 <= int(instance) < self.context.n_instances:
            raise WaaError(1, f"instance {instance} out of range")
        o = {name: getattr(self, name) for name in self.OPTION_FIELDS}
        o.update(self._inst_options.get(int(instance), {}))
        return o

    @property
    def per_instance(self) -> bool:
        return bool(self._inst_options)

    def _options_differ(self) -> bool:
        if not self._inst_options:
            return False
        return len({tuple(self.options_of(i).values()) for i in range(self.context.n_instances)}) > 1

    def set_position(self, x, y, z):
        self.position_x.set_value(x)
        self.position_y.set_value(y)
        self.position_z.set_value(z)

    def set_orientation(self, x, y, z):
        self.orientation_x.set_value(x)
        self.orientation_y.set_value(y)
        self.orientation_z.set_value(z)

    def _fill_desc(self, d):
        o = {name: getattr(self, name) for name in self.OPTION_FIELDS}
        if self.per_instance and self.context._b.prefix != "waa_":
            if self._options_differ():  # (refused before the batch exists)
                raise WaaError(4, "one PannerNode option set per instance is a feature of the device library; this binding keeps one "
                                  "set per batch (render it one context at a time)")
            o = self.options_of(0)  # (equal sets everywhere: the shared option)
        d.i[0] = PANNING_MODEL[self.panning_model]
        d.i[1] = DISTANCE_MODEL[o["distance_model"]]
        d.d[0], d.d[1], d.d[2] = o["ref_distance"], o["max_distance"], o["rolloff_factor"]
        d.d[3], d.d[4], d.d[5] = o["cone_inner_angle"], o["cone_outer_angle"], o["cone_outer_gain"]

    def _apply(self, ctx):
        super()._apply(ctx)
        if self.per_instance and ctx._b.prefix == "waa_":
            b, h = ctx._b, ctx._handle
            for i in sorted(self._inst_options):  # one complete set per instance that has fields of its own
                o = self.options_of(i)
                row = PannerOptions(DISTANCE_MODEL[o["distance_model"]], 0, o["ref_distance"], o["max_distance"], o["rolloff_factor"],
                                    o["cone_inner_angle"], o["cone_outer_angle"], o["cone_outer_gain"])
                b.check(b.panner_set_options_instance(h, self.id, i, C.byref(row)))
        for i, prm in enumerate(ctx.listener().params):  # the AudioListener's params, addressed through this panner
            prm._apply(ctx, node_id=self.id, pid=6 + i)


class AnalyserNode(AudioNode):
    kind = NODE_ANALYSER

    def __init__(self, ctx, fft_size=2048, smoothing_time_constant=0.8, min_decibels=-100.0, max_decibels=-30.0,
                 series_hop=0, series_first=0, **kw):
        super().__init__(ctx, **kw)
        self.fft_size, self.smoothing_time_constant = fft_size, smoothing_time_constant
        self.min_decibels, self.max_decibels = min_decibels, max_decibels
        # a whole series of pulls (spectrograms): one every `series_hop` render quanta from quantum `series_first` on; 0 = off
        self.series_hop, self.series_first = int(series_hop), int(series_first)

    @property
    def series_quanta(self) -> np.ndarray:
        """The render quanta q_k = series_first + k * series_hop <= n_quanta at which the series pulls (empty: not a series node)."""
        n_quanta = (self.context.length + RENDER_QUANTUM_SIZE - 1) // RENDER_QUANTUM_SIZE
        if self.series_hop <= 0 or self.series_first < 0:
            return np.zeros(0, np.int64)
        return np.arange(self.series_first, n_quanta + 1, self.series_hop, dtype=np.int64)

    @property
    def frequency_bin_count(self) -> int:
        return self.fft_size // 2

    def _fill_desc(self, d):
        d.i[0] = self.fft_size
        d.d[0], d.d[1], d.d[2] = self.smoothing_time_constant, self.min_decibels, self.max_decibels
        if self.series_hop != 0 and self.context._b.prefix != "waa_":
            raise WaaError(4, "a series of analyser pulls is a feature of the device library; this binding pulls once per render")
        # (the device library validates both fields; a prefix render serves ONE pull of a plain analyser at its own last quantum)
        if self.context._b.prefix == "waa_" and not self.context._in_prefix:
            d.i[1], d.i[2] = self.series_hop, self.series_first

    def _not_series(self):
        if self.series_hop != 0:
            raise ValueError("this AnalyserNode pulls a series (series_hop > 0): use the get_*_data_series methods")

    def _pull_series(self, fn_name: str, n: int, dtype, out=None):
        """[n_instances][P][n]: every pull of the series of every context (computed once per render and kind on the device).

        Pulls made inside a suspend_sync callback are not part of this: they still go through prefix renders and still start
        from a zero spectrum each."""
        ctx = self.context
        if self.series_hop <= 0:
            raise ValueError("this AnalyserNode pulls once per render (series_hop = 0): use the get_*_data / get_*_data_all methods")
        if ctx._handle is None or ctx._now_q > 0:
            raise WaaError(3, "InvalidStateError - analyser data is only available after start_rendering_sync")
        shape = (ctx.n_instances, len(self.series_quanta), n)
        if out is None:
            out = np.zeros(shape, dtype=dtype)
        if not isinstance(out, np.ndarray) or out.shape != shape or out.dtype != dtype or not out.flags.c_contiguous:
            # (the library writes n values per pull and context through the raw pointer: a wrong buffer is a silent out-of-bounds write)
            raise ValueError(f"out: expected a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
        ptr = out.ctypes.data_as(_FP if dtype == np.float32 else C.POINTER(C.c_uint8))
        ctx._b.check(getattr(ctx._b, fn_name)(ctx._handle, self.id, ptr, n))
        return out

    def get_float_frequency_data_series(self, n: Optional[int] = None, out=None) -> np.ndarray:
        """[n_instances][P][n] dB rows of the series, the smoothed spectrum carried from pull to pull as the reference carries it.
        Pulls made inside a suspend_sync callback still go through prefix renders and still start from a zero spectrum each."""
        return self._pull_series("analyser_get_float_frequency_data_batch", n or self.frequency_bin_count, np.float32, out)

    def get_byte_frequency_data_series(self, n: Optional[int] = None, out=None) -> np.ndarray:
        """[n_instances][P][n] byte rows of the series (same transform pass as the float rows).
        Pulls made inside a suspend_sync callback still go through prefix renders and still start from a zero spectrum each."""
        return self._pull_series("analyser_get_byte_frequency_data_batch", n or self.frequency_bin_count, np.uint8, out)

    def get_float_time_domain_data_series(self, n: Optional[int] = None, out=None) -> np.ndarray:
        """[n_instances][P][n]: the most recent n frames of the mono down-mix in front of every pull.
        Pulls made inside a suspend_sync callback still go through prefix renders."""
        return self._pull_series("analyser_get_float_time_domain_data_batch", n or self.fft_size, np.float32, out)

    def get_byte_time_domain_data_series(self, n: Optional[int] = None, out=None) -> np.ndarray:
        """[n_instances][P][n]: the byte form of the time-domain rows (128 behind fft_size values, as the reference writes).
        Pulls made inside a suspend_sync callback still go through prefix renders."""
        return self._pull_series("analyser_get_byte_time_domain_data_batch", n or self.fft_size, np.uint8, out)

    def _pull(self, fn_name: str, n: int, instance: int, dtype):
        self._not_series()
        ctx = self.context
        if ctx._now_q > 0 and ctx._handle is None:  # inside a suspend_sync callback: what has been rendered up to here
            with ctx._prefix_render(ctx._now_q):
                return self._pull(fn_name, n, instance, dtype)
        if ctx._handle is None:
            raise WaaError(3, "InvalidStateError - analyser data is only available after start_rendering_sync")
        out = np.zeros(n, dtype=dtype)
        ptr = out.ctypes.data_as(_FP if dtype == np.float32 else C.POINTER(C.c_uint8))
        ctx._b.check(getattr(ctx._b, fn_name)(ctx._handle, self.id, instance, ptr, n))
        return out

    def _pull_all(self, fn_name: str, n: int, dtype, out=None):
        """[n_instances][n]: every context's pull in one call (one launch, one transfer on the device)."""
        self._not_series()
        ctx = self.context
        if ctx._now_q > 0 and ctx._handle is None:
            with ctx._prefix_render(ctx._now_q):
                return self._pull_all(fn_name, n, dtype, out)
        if ctx._handle is None:
            raise WaaError(3, "InvalidStateError - analyser data is only available after start_rendering_sync")
        if out is None:
            out = np.zeros((ctx.n_instances, n), dtype=dtype)
        if not isinstance(out, np.ndarray) or out.shape != (ctx.n_instances, n) or out.dtype != dtype or not out.flags.c_contiguous:
            # (the library writes n values per context through the raw pointer: a wrong buffer is a silent out-of-bounds write)
            raise ValueError(f"out: expected a C-contiguous {np.dtype(dtype).name} array of shape {(ctx.n_instances, n)}")
        ptr = out.ctypes.data_as(_FP if dtype == np.float32 else C.POINTER(C.c_uint8))
        ctx._b.check(getattr(ctx._b, fn_name)(ctx._handle, self.id, ptr, n))
        return out

    def get_float_frequency_data_all(self, n: Optional[int] = None, out=None) -> np.ndarray:
        return self._pull_all("analyser_get_float_frequency_data_batch", n or self.frequency_bin_count, np.float32, out)

    def get_byte_frequency_data_all(self, n: Optional[int] = None, out=None) -> np.ndarray:
        return self._pull_all("analyser_get_byte_frequency_data_batch", n or self.frequency_bin_count, np.uint8, out)

    def get_float_time_domain_data_all(self, n: Optional[int] = None, out=None) -> np.ndarray:
        return self._pull_all("analyser_get_float_time_domain_data_batch", n or self.fft_size, np.float32, out)

    def get_byte_time_domain_data_all(self, n: Optional[int] = None, out=None) -> np.ndarray:
        return self._pull_all("analyser_get_byte_time_domain_data_batch", n or self.fft_size, np.uint8, out)

    def get_float_frequency_data(self, n: Optional[int] = None, instance: int = 0) -> np.ndarray:
        return self._pull("analyser_get_float_frequency_data", n or self.frequency_bin_count, instance, np.float32)

    def get_byte_frequency_data(self, n: Optional[int] = None, instance: int = 0) -> np.ndarray:
        return self._pull("analyser_get_byte_frequency_data", n or self.frequency_bin_count, instance, np.uint8)

    def get_float_time_domain_data(self, n: Optional[int] = None, instance: int = 0) -> np.ndarray:
        return self._pull("analyser_get_float_time_domain_data", n or self.fft_size, instance, np.float32)

    def get_byte_time_domain_data(self, n: Optional[int] = None, instance: int = 0) -> np.ndarray:
        return self._pull("analyser_get_byte_time_domain_data", n or self.fft_size, instance, np.uint8)


class WaveShaperNode(AudioNode):
    """src/node/waveshaper.rs:139-253.  A context of the batch may be given its own curve before the render (every context of
    the reference sets the curve of its own node)."""

    kind = NODE_WAVESHAPER

    def __init__(self, ctx, curve=None, oversample="none", **kw):
        super().__init__(ctx, **kw)
        self.oversample = oversample
        self.curve = None
        self._inst_curves = {}  # instance -> curve: one curve per context (waa_waveshaper_set_curve_instance)
        if curve is not None:
            self.set_curve(curve)

    def set_curve(self, curve, instance: int = ALL):
        """instance = ALL: the curve of every context without one of its own.  instance = i: context i's own curve; the node then
        works in per-instance mode.  Lengths may differ between contexts; a context that has neither passes its input through."""
        if instance == ALL:
            if self.curve is not None:
                raise WaaError(3, "InvalidStateError - cannot assign curve twice")
            self.curve = _f32(curve)
            return self
        if self.context._handle is not None:
            raise WaaError(3, "InvalidStateError - the batch is frozen once rendering has started")
        if not 0 <= int(instance) < self.context.n_instances:
            raise WaaError(1, f"instance {instance} out of range")
        if int(instance) in self._inst_curves:
            raise WaaError(3, "InvalidStateError - cannot assign curve twice")
        own = _f32(curve).reshape(-1)
        if own.size == 0:
            raise WaaError(1, "a curve of its own has at least one point")
        self._inst_curves[int(instance)] = own
        return self

    def set_curve_batch(self, curves):
        """curves: a sequence of n_instances arrays, one curve per context, of possibly different lengths"""
        n = self.context.n_instances
        if len(curves) != n:
            raise WaaError(1, f"set_curve_batch takes n_instances = {n} curves, got {len(curves)}")
        for i, c in enumerate(curves):
            self.set_curve(c, instance=i)
        return self

    @property
    def per_instance(self) -> bool:
        return bool(self._inst_curves)

    def _check_per_instance(self):
        if self.context._b.prefix != "waa_":
            raise WaaError(4, "one curve per instance is a feature of the device library; this binding keeps one curve "
                              "per batch (render it one context at a time)")

    def set_oversample(self, oversample: str):
        self.oversample = oversample

    def _fill_desc(self, d):
        d.i[0] = OVERSAMPLE[self.oversample]
        if self.per_instance:
            self._check_per_instance()  # (refusals before the batch exists)

    def _apply(self, ctx):
        b, h = ctx._b, ctx._handle
        if self.curve is not None:
            b.check(b.waveshaper_set_curve(h, self.id, _fp(self.curve), self.curve.size))
        if self.per_instance:
            self._check_per_instance()
            for i, c in sorted(self._inst_curves.items()):
                b.check(b.waveshaper_set_curve_instance(h, self.id, i, _fp(c), c.size))


def _dp(a: np.ndarray):
    return a.ctypes.data_as(_DP)


def _iir_coefficients(feedforward, feedback):
    """IIRFilterOptions validated like the reference's constructor (iir_filter.rs:17-46)"""
    ff = np.ascontiguousarray(feedforward, dtype=np.float64).reshape(-1)
    fb = np.ascontiguousarray(feedback, dtype=np.float64).reshape(-1)
    if not 1 <= ff.size <= MAX_IIR_COEFFS:
        raise WaaError(2, "NotSupportedError - IIR Filter feedforward coefficients should have length >= 0 and <= 20")
    if not np.any(ff != 0.0):
        raise WaaError(3, "InvalidStateError - IIR Filter feedforward coefficients cannot be all zeros")
    if not 1 <= fb.size <= MAX_IIR_COEFFS:
        raise WaaError(2, "NotSupportedError - IIR Filter feedback coefficients should have length >= 0 and <= 20")
    if fb[0] == 0.0:
        raise WaaError(3, "InvalidStateError - IIR Filter feedback first coefficient cannot be zero")
    return ff, fb


class IIRFilterNode(AudioNode):
    """src/node/iir_filter.rs:140-263.  Coefficients are fixed at construction (IIRFilterOptions); a context of the batch may be
    given its own set before the render (every context of the reference constructs its own node)."""

    kind = NODE_IIR_FILTER

    def __init__(self, ctx, feedforward, feedback, **kw):
        ff, fb = _iir_coefficients(feedforward, feedback)
        super().__init__(ctx, **kw)
        self.feedforward, self.feedback = ff, fb
        self._inst_coefs = {}  # instance -> (feedforward, feedback): one set per context (waa_iir_set_coefficients_instance)

    def set_coefficients(self, feedforward, feedback, instance: int = ALL):
        """instance = ALL: the set of every context without one of its own.  instance = i: context i's own IIRFilterOptions;
        the node then works in per-instance mode.  Lengths may differ between contexts."""
        ff, fb = _iir_coefficients(feedforward, feedback)
        if self.context._handle is not None:
            raise WaaError(3, "InvalidStateError - the batch is frozen once rendering has started")
        if instance == ALL:
            self.feedforward, self.feedback = ff, fb
        else:
            if not 0 <= int(instance) < self.context.n_instances:
                raise WaaError(1, f"instance {instance} out of range")
            self._inst_coefs[int(instance)] = (ff, fb)
        return self

    def set_coefficients_batch(self, feedforward, feedback):
        """feedforward [n_instances, nff], feedback [n_instances, nfb]: one set per context."""
        ff = np.asarray(feedforward, dtype=np.float64)
        fb = np.asarray(feedback, dtype=np.float64)
        n = self.context.n_instances
        if ff.ndim != 2 or fb.ndim != 2 or ff.shape[0] != n or fb.shape[0] != n:
            raise WaaError(1, f"set_coefficients_batch takes [n_instances = {n}, nff] and [n_instances = {n}, nfb], got {ff.shape} and {fb.shape}")
        for i in range(n):
            self.set_coefficients(ff[i], fb[i], instance=i)
        return self

    @property
    def per_instance(self) -> bool:
        return bool(self._inst_coefs)

    def _check_per_instance(self):
        if self.context._b.prefix != "waa_":
            raise WaaError(4, "one coefficient set per instance is a feature of the device library; this binding keeps one set "
                              "per batch (render it one context at a time)")

    def _fill_desc(self, d):
        if self.per_instance:
            self._check_per_instance()  # (refusals before the batch exists)

    def _apply(self, ctx):
        b, h = ctx._b, ctx._handle
        b.check(b.iir_set_coefficients(h, self.id, _dp(self.feedforward), self.feedforward.size, _dp(self.feedback),
                                       self.feedback.size))
        if self.per_instance:
            self._check_per_instance()
            for i, (ff, fb) in sorted(self._inst_coefs.items()):
                b.check(b.iir_set_coefficients_instance(h, self.id, i, _dp(ff), ff.size, _dp(fb), fb.size))

    def get_frequency_response(self, frequency_hz, instance: int = ALL) -> tuple:
        """instance = i: the response of context i's filter (its own set, or the ALL set where it has none)"""
        ff, fb = self.feedforward, self.feedback
        if instance != ALL:
            if not 0 <= int(instance) < self.context.n_instances:
                raise WaaError(1, f"instance {instance} out of range")
            ff, fb = self._inst_coefs.get(int(instance), (ff, fb))
        hz = _f32(frequency_hz)
        mag = np.empty_like(hz)
        phase = np.empty_like(hz)
        b = self.context._b
        b.check(b.iir_frequency_response(_dp(ff), ff.size, _dp(fb), fb.size, self.context.sample_rate, _fp(hz), _fp(mag), _fp(phase),
                                         hz.size))
        return mag, phase


class DelayNode(AudioNode):
    """src/node/delay.rs:127-376 (DelayOptions{max_delay_time = 1, delay_time = 0}).  Inside a graph cycle the
    node acts as the reference's cycle breaker (delay clamped to one render quantum)."""

    kind = NODE_DELAY

    def __init__(self, ctx, max_delay_time: float = 1.0, delay_time: float = 0.0, **kw):
        if not (0.0 < max_delay_time < 180.0):  # delay.rs:290-293
            raise WaaError(2, "NotSupportedError - maxDelayTime MUST be greater than zero and less than three minutes")
        super().__init__(ctx, **kw)
        self.max_delay_time = float(max_delay_time)
        self.delay_time = AudioParam(self, 0, delay_time)
        self.params = [self.delay_time]

    def _fill_desc(self, d):
        d.d[0] = self.max_delay_time


def _assert_valid_number_of_ports(n: int):
    # assert_valid_number_of_channels, channel_splitter.rs:23-30 / channel_merger.rs:21-28
    if not 0 < n <= MAX_CHANNELS:
        raise WaaError(1, f"IndexSizeError - Invalid number of channels: {n} is outside range [1, {MAX_CHANNELS}]")


class ChannelSplitterNode(AudioNode):
    """src/node/channel_splitter.rs:80-210 (ChannelSplitterOptions{number_of_outputs = 6}; count = number_of_outputs,
    explicit, discrete — all three fixed).  One input, `number_of_outputs` mono outputs: output k carries channel k of the
    input, silence where the input has no such channel.  Connect an output with `connect(dest, output=k)`."""

    kind = NODE_CHANNEL_SPLITTER
    DEFAULT_NUMBER_OF_OUTPUTS = 6

    def __init__(self, ctx, number_of_outputs: int = 6, channel_count=None, channel_count_mode=None, channel_interpretation=None):
        number_of_outputs = int(number_of_outputs)
        _assert_valid_number_of_ports(number_of_outputs)
        # (ChannelSplitterNode::new, :146-161: a count other than the default of 6 must equal number_of_outputs)
        if channel_count is not None and channel_count != self.DEFAULT_NUMBER_OF_OUTPUTS:
            self._assert_count(channel_count, number_of_outputs)
        if channel_count_mode is not None:
            self._assert_mode(channel_count_mode)
        if channel_interpretation is not None:
            self._assert_interpretation(channel_interpretation)
        self.number_of_outputs = number_of_outputs
        self.default_channel_config = (number_of_outputs, "explicit", "discrete")
        super().__init__(ctx)

    @staticmethod
    def _assert_count(count, number_of_outputs):
        if count != number_of_outputs:
            raise WaaError(3, "InvalidStateError - channel count of ChannelSplitterNode must be equal to number of outputs")

    @staticmethod
    def _assert_mode(mode):
        if mode != "explicit":
            raise WaaError(3, "InvalidStateError - channel count of ChannelSplitterNode must be set to Explicit")

    @staticmethod
    def _assert_interpretation(interpretation):
        if interpretation != "discrete":
            raise WaaError(3, "InvalidStateError - channel interpretation of ChannelSplitterNode must be set to Discrete")

    # channel_splitter.rs:120-134: the setters only assert (the values cannot change)
    def set_channel_count(self, v: int):
        self._assert_count(int(v), self.number_of_outputs)

    def set_channel_count_mode(self, v: str):
        self._assert_mode(v)

    def set_channel_interpretation(self, v: str):
        self._assert_interpretation(v)

    def _fill_desc(self, d):
        d.i[0] = self.number_of_outputs


class ChannelMergerNode(AudioNode):
    """src/node/channel_merger.rs:62-172 (ChannelMergerOptions{number_of_inputs = 6}; count 1 and explicit are fixed, the
    interpretation is free: speakers).  `number_of_inputs` inputs, each mixed to mono; one output with `number_of_inputs`
    channels, channel k = input k.  Connect to an input with `connect(merger, input=k)`."""

    kind = NODE_CHANNEL_MERGER
    default_channel_config = (1, "explicit", "speakers")

    def __init__(self, ctx, number_of_inputs: int = 6, channel_count=None, channel_count_mode=None, channel_interpretation=None):
        number_of_inputs = int(number_of_inputs)
        _assert_valid_number_of_ports(number_of_inputs)
        if channel_count is not None:
            self._assert_count(channel_count)
        if channel_count_mode is not None:
            self._assert_mode(channel_count_mode)
        self.number_of_inputs = number_of_inputs
        super().__init__(ctx, channel_interpretation=channel_interpretation)

    @staticmethod
    def _assert_count(count):
        if count != 1:
            raise WaaError(3, "InvalidStateError - channel count of ChannelMergerNode must be equal to 1")

    @staticmethod
    def _assert_mode(mode):
        if mode != "explicit":
            raise WaaError(3, "InvalidStateError - channel count of ChannelMergerNode must be set to Explicit")

    # channel_merger.rs:102-110
    def set_channel_count(self, v: int):
        self._assert_count(int(v))

    def set_channel_count_mode(self, v: str):
        self._assert_mode(v)

    def _fill_desc(self, d):
        d.i[0] = self.number_of_inputs


class RenderedBatch:
    """What start_rendering_sync returns: one AudioBuffer per instance (array [inst, ch, frames])."""

    def __init__(self, data: np.ndarray, sample_rate: float):
        self.data = data
        self.sample_rate = sample_rate

    def buffer(self, instance: int = 0) -> AudioBuffer:
        return AudioBuffer(self.data[instance], self.sample_rate)

    def get_channel_data(self, c: int, instance: int = 0) -> np.ndarray:
        return self.data[instance, c]

    @property
    def length(self):
        return self.data.shape[2]

    @property
    def number_of_channels(self):
        return self.data.shape[1]


class OfflineAudioContext:
    """A batch of ``n_instances`` identically shaped OfflineAudioContexts (offline.rs:68)."""

    def __init__(self, number_of_channels: int, length: int, sample_rate: float, n_instances: int = 1,
                 binding: Optional[Binding] = None, device: int = -1):
        if binding is None:
            from . import default_binding  # loads libwaa_hip.so; raises if it is not built
            binding = default_binding()
        self._b = binding
        self.number_of_channels = int(number_of_channels)
        self.length = int(length)
        self.sample_rate = float(np.float32(sample_rate))
        self.n_instances = int(n_instances)
        self.device = device
        self._nodes: List[AudioNode] = []
        self._edges = []
        self._handle = None
        self._rendered = False
        self._foreign = False
        # OfflineAudioContext::suspend_sync (offline.rs:359-397): callbacks by render quantum; while one runs, _now_q is its quantum
        # and every control call (connect / disconnect, AudioParam methods, start / stop) goes to _ctl[q] instead of the node's
        # static description — replayed between the ranges of waa_render_range, where the reference's render thread handles them
        self._suspends = {}
        self._ctl = {}
        self._now_q = 0
        self._in_prefix = False  # inside _prefix_render: series analysers are described as plain ones
        self._replayed = 0  # the control log has been replayed up to this quantum on the current batch
        self._live = []   # the connections that exist "now" (disconnect's InvalidAccessError, disconnect() of everything)
        self._state = "suspended"  # AudioContextState of a context that has not started rendering (offline.rs:451)
        self._listener = AudioListener()
        for prm in self._listener.params:
            prm._listener_ctx = self
        self._destination = AudioDestinationNode(self)

    def state(self) -> str:
        return self._state

    def _log(self, action):
        self._ctl.setdefault(self._now_q, []).append(action)

    def _connect(self, edge):
        if edge in self._live:
            return  # (connecting twice is a no-op: the reference keeps a set of connections)
        self._live.append(edge)
        if self._now_q > 0:
            self._log(lambda b, h: b.check(b.connect(h, *edge)))
        else:
            self._edges.append(edge)

    def _disconnect(self, frm, output, to, to_input):
        hit = [e for e in self._live if e[0] == frm and (output is None or e[1] == output) and (to is None or e[2] == to) and
               (to_input is None or e[3] == to_input)]
        if to is not None and not hit:
            raise WaaError(1, "InvalidAccessError - attempting to disconnect unconnected nodes")
        for e in hit:
            self._live.remove(e)
            if self._now_q > 0:
                self._log(lambda b, h, e=e: b.check(b.disconnect(h, *e)))
            else:
                self._edges.remove(e)

    def suspend_sync(self, suspend_time: float, callback):
        """OfflineAudioContext::suspend_sync (offline.rs:359-397): run `callback(context)` when the render reaches `suspend_time`
        (quantised UP to a render quantum, calculate_suspend_frame offline.rs:241-251); the render resumes when it returns."""
        if self._rendered:
            raise WaaError(3, "InvalidStateError - cannot suspend when rendering has already started")
        if not suspend_time >= 0.0:
            raise WaaError(3, "InvalidStateError: suspendTime cannot be negative")
        if not suspend_time < self.length / float(self.sample_rate):
            raise WaaError(3, "InvalidStateError: suspendTime cannot be greater than or equal to the total render duration")
        q = int(np.ceil(suspend_time * float(self.sample_rate) / RENDER_QUANTUM_SIZE))
        if q in self._suspends:
            raise WaaError(3, "InvalidStateError - cannot suspend multiple times at the same render quantum")
        self._suspends[q] = callback

    def _run_suspend_callbacks(self):
        """The callbacks in render order, each with the control clock at its quantum (thread.rs:281-287)."""
        for q in sorted(self._suspends):
            cb = self._suspends.pop(q)
            self._now_q = q if q > 0 else 0  # (a suspend at time 0 runs in front of the first quantum: plain graph edits)
            self._state = "suspended"
            try:
                cb(self)
            finally:
                self._state = "running"
                self._now_q = 0

    def _register(self, node: AudioNode) -> int:
        if self._handle is not None:
            raise WaaError(3, "InvalidStateError - graph is frozen once rendering has started")
        self._nodes.append(node)
        return len(self._nodes) - 1

    # BaseAudioContext
    def destination(self) -> AudioDestinationNode:
        return self._destination

    def listener(self) -> AudioListener:
        return self._listener

    def create_buffer(self, number_of_channels: int, length: int, sample_rate: float) -> AudioBuffer:
        return AudioBuffer(np.zeros((number_of_channels, length), np.float32), sample_rate)

    def create_buffer_source(self, **kw):
        return AudioBufferSourceNode(self, **kw)

    def create_constant_source(self, **kw):
        return ConstantSourceNode(self, **kw)

    def create_biquad_filter(self, **kw):
        return BiquadFilterNode(self, **kw)

    def create_gain(self, **kw):
        return GainNode(self, **kw)

    def create_convolver(self, **kw):
        return ConvolverNode(self, **kw)

    def create_stereo_panner(self, **kw):
        return StereoPannerNode(self, **kw)

    def create_panner(self, **kw):
        return PannerNode(self, **kw)

    def create_analyser(self, **kw):
        return AnalyserNode(self, **kw)

    def create_wave_shaper(self, **kw):
        return WaveShaperNode(self, **kw)

    def create_oscillator(self, **kw):
        return OscillatorNode(self, **kw)

    def create_periodic_wave(self, **kw):
        return PeriodicWave(self, **kw)

    def create_dynamics_compressor(self, **kw):
        """meter=True: keep reduction() after every render quantum (DynamicsCompressorNode.reduction_series)"""
        return DynamicsCompressorNode(self, **kw)

    def create_channel_splitter(self, number_of_outputs: int = 6, **kw):
        return ChannelSplitterNode(self, number_of_outputs, **kw)

    def create_channel_merger(self, number_of_inputs: int = 6, **kw):
        return ChannelMergerNode(self, number_of_inputs, **kw)

    def create_delay(self, max_delay_time: float = 1.0, **kw):
        return DelayNode(self, max_delay_time=max_delay_time, **kw)

    def create_iir_filter(self, feedforward, feedback, **kw):
        return IIRFilterNode(self, feedforward, feedback, **kw)

    # -- render -------------------------------------------------------------------------
    def graph_desc(self) -> "GraphDesc":
        """The waa_graph_desc of this context's graph (the arrays it points at stay alive with the returned object)."""
        n = len(self._nodes)
        nodes = (NodeDesc * n)(*[nd._desc() for nd in self._nodes])
        m = len(self._edges)
        edges = (EdgeDesc * max(m, 1))()
        for k, (f, fo, t, ti) in enumerate(self._edges):
            edges[k].from_, edges[k].from_output, edges[k].to, edges[k].to_input = f, fo, t, ti
        g = GraphDesc(n, nodes, m, edges)
        g._keep = (nodes, edges)
        if any(getattr(nd, "panning_model", None) == "HRTF" for nd in self._nodes):
            ensure_hrtf_database(self._b)
        return g

    def _prefix_render(self, q):
        """What a suspend callback sees when it READS rendered audio (an analyser pull at quantum q): the engine renders node-major,
        so the quanta in front of the suspend point are rendered by a batch of their own — the graph as it is so far, `q` quanta
        long, the control log of the earlier suspend points replayed (a render is causal: its first q quanta do not depend on what
        happens later).  The batch lives for the duration of the `with` block."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            now, replayed, rendered = self._now_q, self._replayed, self._rendered
            self._now_q = 0
            self._in_prefix = True
            try:
                self._build(length=q * RENDER_QUANTUM_SIZE, run_callbacks=False)
                self._replayed = 0
                self._render_ranges(q)
                yield
            finally:
                if self._handle is not None:
                    self._b.batch_destroy(self._handle)
                self._handle = None
                self._in_prefix = False
                self._now_q, self._replayed, self._rendered = now, replayed, rendered
        return scope()

    def _build(self, length=None, run_callbacks=True):
        if run_callbacks:
            self._run_suspend_callbacks()  # (every node a callback creates must be in the graph description)
        g = self.graph_desc()
        h = _VP()
        self._b.check(self._b.batch_create(C.byref(g), self.n_instances, self.number_of_channels, self.length if length is None else length,
                                           self.sample_rate, self.device, C.byref(h)))
        self._handle = h
        for nd in self._nodes:
            nd._apply(self)

    def _render_ranges(self, n_quanta, final=True):
        """waa_render_range between the suspend points, the control log of each point replayed in front of its quantum; the last
        range renders (final=False: everything but that last range — what a plan description needs).  Without suspend points:
        waa_render."""
        points = [q for q in sorted(self._ctl) if 0 < q < n_quanta]
        if self._replayed:
            points = []
        if not points:
            if final:
                self._b.check(self._b.render(self._handle) if not self._replayed else
                              self._b.render_range(self._handle, self._replayed, n_quanta - self._replayed))
            return
        prev = 0
        for q in points:
            self._b.check(self._b.render_range(self._handle, prev, q - prev))
            for action in self._ctl[q]:
                action(self._b, self._handle)
            prev = q
        self._replayed = prev
        if final:
            self._b.check(self._b.render_range(self._handle, prev, n_quanta - prev))

    def _adopt(self, handle):
        """Configure a batch the LIBRARY created for this graph (waa_render_sharded's setup callback): node payloads, params,
        schedules.  The batch stays the library's: _release() forgets it without destroying it."""
        self._handle = _VP(handle) if not isinstance(handle, _VP) else handle
        self._foreign = True
        try:
            for nd in self._nodes:
                nd._apply(self)
        except BaseException:
            self._handle = None  # a node refused its payload: the batch is still the library's to destroy, never ours
            raise

    def _release(self):
        self._handle = None
        self._foreign = False  # (the adopted batch is forgotten: whatever this context creates next is its own)

    def prepare(self):
        """Create the batch and upload every payload (outside any timed region)."""
        if self._handle is None:
            self._build()
        return self

    def render_async(self):
        """Launch the render on the batch's stream without waiting (bench inner loop)."""
        self.prepare()
        self._state = "running"
        if self._rendered or not self._ctl:
            self._b.check(self._b.render(self._handle))  # (a second render of the same batch: the bench loop)
        else:
            self._render_ranges((self.length + RENDER_QUANTUM_SIZE - 1) // RENDER_QUANTUM_SIZE)
        self._rendered = True

    def sync(self):
        self._b.check(self._b.sync(self._handle))

    def start_rendering_sync(self) -> RenderedBatch:
        if self._rendered:
            raise WaaError(3, "InvalidStateError - Cannot call `startRendering` twice")
        self.render_async()
        out = np.empty((self.n_instances, self.number_of_channels, self.length), np.float32)
        self._b.check(self._b.download_all(self._handle, _fp(out)))
        self._state = "closed"  # offline.rs:176
        return RenderedBatch(out, self.sample_rate)

    def render_instances(self, instances) -> np.ndarray:
        """start_rendering_sync for the whole batch, but only the AudioBuffers of `instances` are downloaded
        (waa_download per channel): full-size batches whose result would not fit a test's host memory budget."""
        if self._rendered:
            raise WaaError(3, "InvalidStateError - Cannot call `startRendering` twice")
        self.render_async()
        out = np.empty((len(instances), self.number_of_channels, self.length), np.float32)
        for k, inst in enumerate(instances):
            for c in range(self.number_of_channels):
                self._b.check(self._b.download(self._handle, int(inst), c, _fp(out[k, c]), self.length))
        return out

    # -- levels of the rendered output, computed on the device (include/waa_hip_device.h: waa_output_levels & co.) --------------
    def _rendered_on_device(self, what):
        if self._b.prefix != "waa_":
            raise WaaError(4, f"{what} is a feature of the device library; this binding hands back f32 planes and nothing else")
        if self._handle is None or not self._rendered or self._now_q > 0:
            raise WaaError(3, "InvalidStateError - nothing rendered yet")

    def output_levels(self) -> np.ndarray:
        """[n_instances, n_channels] records with the fields sum_sq (f64), n_nonfinite, first_nonfinite, n_clipped (u64) and peak
        (f32) of every context's every output channel, as waa_hip_device.h defines them — without downloading the audio.  After
        start_rendering_sync or render_async, until close()."""
        self._rendered_on_device("output_levels")
        out = np.zeros((self.n_instances, self.number_of_channels), LEVEL_STATS_DTYPE)
        out["first_nonfinite"] = np.iinfo(np.uint64).max  # (a context of no frames: the library writes nothing)
        self._b.check(self._b.output_levels(self._handle, out.ctypes.data_as(_VP)))
        return out[["sum_sq", "n_nonfinite", "first_nonfinite", "n_clipped", "peak"]]

    def output_level_series(self):
        """(peak float32, sum_sq float64), each [n_instances, n_channels, n_quanta]: the peak and the energy of every render quantum
        of every output channel"""
        self._rendered_on_device("output_level_series")
        shape = (self.n_instances, self.number_of_channels, (self.length + RENDER_QUANTUM_SIZE - 1) // RENDER_QUANTUM_SIZE)
        peak, sum_sq = np.zeros(shape, np.float32), np.zeros(shape, np.float64)
        self._b.check(self._b.output_level_series(self._handle, _fp(peak), sum_sq.ctypes.data_as(_DP)))
        return peak, sum_sq

    # -- integrated loudness of the rendered output (include/waa_hip_device.h: waa_output_loudness & co.) -----------------------
    def output_loudness(self, weights=None) -> np.ndarray:
        """[n_instances] records with the fields integrated, momentary_max, short_term_max, relative_threshold (LUFS, f64; -inf where
        there is nothing to measure), n_blocks and n_gated of every context (BS.1770-4 as waa_hip_device.h defines it) — without
        downloading the audio.  weights: one per output channel; None: the Web Audio layouts' (5.1 and quad surrounds 1.41, LFE 0)."""
        self._rendered_on_device("output_loudness")
        w, wp = _weights_arg(weights, self.number_of_channels)
        out = np.zeros(self.n_instances, LOUDNESS_STATS_DTYPE)
        self._b.check(self._b.output_loudness(self._handle, wp, out.ctypes.data_as(_VP)))
        return out

    def output_loudness_series(self) -> np.ndarray:
        """float64 [n_instances, n_channels, n_sub]: the K-weighted energy of every whole 100 ms sub-block of every output channel"""
        self._rendered_on_device("output_loudness_series")
        hop = int(self._b.loudness_hop(self.sample_rate))
        z = np.zeros((self.n_instances, self.number_of_channels, self.length // hop if hop else 0), np.float64)
        self._b.check(self._b.output_loudness_series(self._handle, z.ctypes.data_as(_DP)))
        return z

    def download_pcm16(self, gain=None, normalize_peak=None, normalize_loudness=None, max_peak=None) -> np.ndarray:
        """int16 [n_instances, length, n_channels]: every context's AudioBuffer as interleaved 16-bit PCM (sample * 32768, rounded to
        nearest even, saturated, NaN -> 0).  gain: [n_instances], each context multiplied by its own (one f32 multiply) in front of
        the pack.  normalize_peak=t: gain[i] = float32(t) / (the largest peak of context i's channels), computed on the host from
        output_levels(); 1 for a silent context.  Giving both is a ValueError.  normalize_loudness=T (LUFS): gain[i] =
        float32(10 ** ((T - I_i) / 20)) with I_i the integrated loudness of output_loudness(), 1 where that is -inf; with max_peak=p
        no larger than float32(p) / (the context's peak).  It excludes gain and normalize_peak; max_peak needs it."""
        if gain is not None and normalize_peak is not None:
            raise ValueError("download_pcm16: give gain or normalize_peak, not both")
        if normalize_loudness is not None and (gain is not None or normalize_peak is not None):
            raise ValueError("download_pcm16: give normalize_loudness or one of gain and normalize_peak, not both")
        if max_peak is not None and normalize_loudness is None:
            raise ValueError("download_pcm16: max_peak limits the gain of normalize_loudness and needs it")
        self._rendered_on_device("download_pcm16")
        if normalize_loudness is not None:
            integrated = self.output_loudness()["integrated"]
            gain = np.ones(self.n_instances, np.float32)
            measured = np.isfinite(integrated)
            with np.errstate(over="ignore"):
                gain[measured] = np.float32(10.0 ** ((float(normalize_loudness) - integrated[measured]) / 20.0))
            if max_peak is not None:
                peak = self.output_levels()["peak"].max(axis=1).astype(np.float32)
                limit = np.full(self.n_instances, np.inf, np.float32)
                np.divide(np.float32(max_peak), peak, out=limit, where=peak > 0)
                gain = np.minimum(gain, limit)
        if normalize_peak is not None:
            peak = self.output_levels()["peak"].max(axis=1).astype(np.float32)
            gain = np.ones(self.n_instances, np.float32)
            np.divide(np.float32(normalize_peak), peak, out=gain, where=peak > 0)
        out = np.empty((self.n_instances, self.length, self.number_of_channels), np.int16)
        dst = out.ctypes.data_as(C.POINTER(C.c_int16))
        if gain is None:
            self._b.check(self._b.download_all_pcm16(self._handle, dst))
            return out
        gain = _f32(gain)
        if gain.shape != (self.n_instances,):
            raise ValueError(f"gain: expected {self.n_instances} values, one per context (got shape {gain.shape})")
        self._b.check(self._b.download_all_pcm16_gain(self._handle, dst, _fp(gain)))
        return out

    def plan_describe(self) -> str:
        """The launch plan derived from the graph (works on a plan-only context: device=PLAN_ONLY)."""
        self.prepare()
        if self._ctl and not self._rendered:
            self._render_ranges((self.length + RENDER_QUANTUM_SIZE - 1) // RENDER_QUANTUM_SIZE, final=False)
        need = C.c_size_t()
        self._b.check(self._b.plan_describe(self._handle, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value + 1)
        self._b.check(self._b.plan_describe(self._handle, buf, need.value + 1, None))
        return buf.value.decode()

    def output_device(self):
        p, s_i, s_c = _VP(), C.c_uint64(), C.c_uint64()
        self._b.check(self._b.output_device(self._handle, C.byref(p), C.byref(s_i), C.byref(s_c)))
        return p.value, s_i.value, s_c.value

    def profile(self, enable=True):
        self.prepare()
        self._b.check(self._b.profile_enable(self._handle, int(enable)))

    def profile_entries(self):
        out = []
        for i in range(self._b.profile_count(self._handle)):
            name, launches, ms = C.c_char_p(), C.c_uint64(), C.c_double()
            self._b.check(self._b.profile_get(self._handle, i, C.byref(name), C.byref(launches), C.byref(ms)))
            out.append((name.value.decode(), launches.value, ms.value))
        return out

    def profile_reset(self):
        self._b.check(self._b.profile_reset(self._handle))

    def close(self):
        if self._handle is not None:
            if not getattr(self, "_foreign", False):  # an adopted batch belongs to the library (waa_render_sharded destroys it)
                self._b.batch_destroy(self._handle)
            self._handle = None
            self._foreign = False  # (a context that is prepared on its own afterwards owns THAT batch)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def resample(binding: Binding, data, source_sample_rate: float, target_sample_rate: float) -> np.ndarray:
    """AudioBuffer::resample (src/buffer.rs:311-363) for a [channels, frames] array."""
    data = _f32(data)
    if data.ndim == 1:
        data = data[None, :]
    n = binding.buffer_resample(_fp(data[0]), data.shape[1], source_sample_rate, target_sample_rate, None, 0)
    out = np.empty((data.shape[0], n), np.float32)
    for c in range(data.shape[0]):
        binding.buffer_resample(_fp(data[c]), data.shape[1], source_sample_rate, target_sample_rate, _fp(out[c]), n)
    return out


# ---- HRTF database (src/node/panner.rs:39-68) --------------------------------------------------------------
# The reference embeds resources/IRC_1003_C.bin in the crate (`include_bytes!`); a library behind the C ABI gets the
# same bytes through waa_hrtf_load_sphere, once per process.  `set_hrtf_database` names the file (or the bytes) this
# mirror hands over the first time a context with an HRTF PannerNode is built.
_HRTF_DATABASE = None
_HRTF_LOADED = set()


def set_hrtf_database(path_or_bytes):
    global _HRTF_DATABASE
    if isinstance(path_or_bytes, (bytes, bytearray)):
        _HRTF_DATABASE = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            _HRTF_DATABASE = f.read()
    _HRTF_LOADED.clear()


def ensure_hrtf_database(binding: Binding):
    if id(binding.lib) in _HRTF_LOADED:
        return
    if _HRTF_DATABASE is None:
        raise WaaError(3, "InvalidStateError - HRTF panning needs the HRIR sphere: call set_hrtf_database(path) first")
    binding.check(binding.hrtf_load_sphere(_HRTF_DATABASE, len(_HRTF_DATABASE)))
    _HRTF_LOADED.add(id(binding.lib))


def hrtf_sample(binding: Binding, sample_rate: float, direction) -> np.ndarray:
    """hrtf::HrirSphere::sample_bilinear (test hook): [2, taps] left / right HRIR for a direction (sphere coordinates)."""
    ensure_hrtf_database(binding)
    n = int(binding.hrtf_hrir_length(sample_rate))
    out = np.zeros((2, n), np.float32)
    d = _f32(direction)
    binding.hrtf_sample(sample_rate, _fp(d), _fp(out[0]), _fp(out[1]))
    return out
