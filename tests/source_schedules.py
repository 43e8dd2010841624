"""AudioBufferSourceNode schedules for tests/test_source_schedules.py: a generator of cases whose edge values are listed, not left
to chance, the calls that put a case onto a source node (the same calls for the oracle and the product), the record tables a
plan-only batch uploaded (waa_debug_source_records, measurement build) and their evaluation in numpy float64 the way the device
readers evaluate them."""
import ctypes as C

import numpy as np

import web_audio_api_rs_amd as waa
from graphs import assert_all_finite, assert_le, white_noise

RQ = 128
ALL = waa.api.ALL
Q_SILENT, Q_FAST, Q_SLOW, Q_FAST_LOOP = 0, 1, 2, 3

FRAMES = [1, 2, 3, 5, 127, 255, 257, 1000, 4097, 4999, 5001, 5002, 5003]
# "foreign": rate 1.0 on a buffer of another sample rate than the context's (the slow track by the sampling ratio alone); the plain
# 1.0 is listed twice so that the fast track (own rate, no detune, aligned start) is drawn often enough to be reached
RATES = ["foreign", 1.0, 1.0, 0.0, 1e-3, 0.37, 0.999, 1.5, 1.96, 1.98, 1.99, 2.0, 2.01, 3.25, 8.0, -0.37, -1.0, -1.99]
DETUNES = [0.0, 0.0, 0.0, 1200.0, -1200.0, 33.0]
BUFFER_RATES = [None, None, 22050.0, 38000.0, 44100.0, 96000.0]  # None: the context's own
CONTEXT_RATES = [48000.0, 48000.0, 44100.0]
LOOPS = ["none", "none", "whole", "on-frames", "between-frames", "3.5-frames", "empty", "offset-behind-end"]
WHENS = ["zero", "zero", "1.5-frames", "second-quantum", "later", "quantum-3"]
LENGTHS = [1, 127, 128, 129] + [RQ * 24 + 5] * 6
F64_MAX = 1.7976931348623157e308


def schedule_case(seed, length=None, frames=None, channels=None, sr=None):
    """One schedule as plain data.  `length`, `frames`, `channels`, `sr`: what a batch of several cases has to share (or a test
    pins); everything else is drawn.  Reverse + loop never reaches the buffer's last frame (the reference panics there,
    audio_buffer_source.rs:795-797): loop_end <= (frames - 1) / buffer_rate and an offset inside the loop — a rule on the inputs."""
    rng = np.random.default_rng(0x5C4ED + seed)
    pick = lambda seq: seq[int(rng.integers(len(seq)))]  # noqa: E731
    drawn = dict(frames=pick(FRAMES), channels=pick([1, 2]), sr=pick(CONTEXT_RATES), length=pick(LENGTHS))
    frames = drawn["frames"] if frames is None else frames
    channels = drawn["channels"] if channels is None else channels
    sr = drawn["sr"] if sr is None else sr
    length = drawn["length"] if length is None else length
    rate, detune, buffer_rate = pick(RATES), pick(DETUNES), pick(BUFFER_RATES)
    plain = pick(range(8)) == 0  # one case in eight can take the fast track: rate 1 on the context's own rate, no offset, whole loop or none
    if plain:
        rate, detune, buffer_rate = 1.0, 0.0, None
    if rate == "foreign":
        rate, buffer_rate = 1.0, pick([r for r in BUFFER_RATES if r not in (None, sr)])
    buffer_rate = sr if buffer_rate is None else buffer_rate
    dur = frames / buffer_rate
    kind = pick(LOOPS)
    if plain:
        kind = pick(["none", "whole"])
    a, b = frames // 4, max(frames // 4 + 1, 3 * frames // 4)  # interior loop points in buffer frames
    loop, loop_start, loop_end = kind != "none", 0.0, 0.0
    if kind in ("on-frames", "offset-behind-end"):
        loop_start, loop_end = a / buffer_rate, b / buffer_rate
    elif kind == "between-frames":
        loop_start, loop_end = (a + 0.37) / buffer_rate, min(b + 0.61, frames) / buffer_rate
    elif kind == "3.5-frames":
        loop_start, loop_end = a / buffer_rate, min(a + 3.5, frames) / buffer_rate
    elif kind == "empty":
        loop_start = loop_end = a / buffer_rate
    early = min(10.25, 0.25 * frames) / buffer_rate
    offset = pick([0.0, 0.0, early, 0.5 * dur, dur - 0.5 / buffer_rate] if rate < 0 else [0.0, 0.0, early, 0.5 * dur])
    if plain:
        offset = 0.0
    if kind == "offset-behind-end":
        offset = loop_end + 0.25 * (dur - loop_end)
    if loop and rate < 0:
        if frames < 3:
            loop, loop_start, loop_end = False, 0.0, 0.0
        else:
            loop_end = min(loop_end if loop_end > 0.0 else dur, (frames - 1) / buffer_rate)
            loop_start = max(0.0, min(loop_start, loop_end - 1.0 / buffer_rate))
            if not loop_start <= offset < loop_end:
                offset = loop_start + 0.5 * (loop_end - loop_start)
    when = {"zero": 0.0, "1.5-frames": 1.5 / sr, "second-quantum": (RQ + 37.25) / sr, "later": (RQ * 9 + 77.5) / sr,
            "quantum-3": RQ * 3 / sr}[pick(WHENS)]
    duration = pick([None, None, None, 200.25 / sr, 1000.5 / sr])
    stop = pick([None, None, None, when + 333.3 / sr, when + 1500.7 / sr])
    return dict(seed=seed, frames=frames, channels=channels, buffer_rate=buffer_rate, sr=sr, length=length, rate=rate, detune=detune,
                loop=loop, loop_kind=kind if loop else "none", loop_start=loop_start, loop_end=loop_end, when=when, offset=offset,
                duration=duration, stop=stop)


def make_case(**kw):
    """a named case: the defaults of a plain start() on a looping-off source, overridden by `kw`"""
    case = dict(seed=0, frames=1000, channels=2, buffer_rate=48000.0, sr=48000.0, length=RQ * 24 + 5, rate=1.0, detune=0.0, loop=False,
                loop_kind="named", loop_start=0.0, loop_end=0.0, when=0.0, offset=0.0, duration=None, stop=None)
    case.update(kw)
    return case


def expect_silence(case):
    """Is silence the right render?  From the inputs, by the reference's start rule (audio_buffer_source.rs:680-690): the first
    frame at or behind `when` lies behind the render's end; or the playhead STARTS at the buffer's end — the offset, moved on by
    the sub-sample part of `when` times the rate and clamped to the buffer (and to the loop's end), is the buffer's duration — and
    a forward source stays there, a reverse one without a loop has left the buffer with its next step.  (Buffers of one to three
    frames do this; rate 0 elsewhere holds a sample of white noise: not silent.  Every stop and duration drawn lets frames through.)"""
    sr, dur = case["sr"], case["frames"] / case["buffer_rate"]
    n0 = int(np.ceil(case["when"] * sr - 1e-6))
    if n0 >= case["length"]:
        return True
    current_time = float(n0 // RQ * RQ) / sr + float(n0 % RQ) * (1.0 / sr)
    cpr = case["rate"] * 2.0 ** (case["detune"] / 1200.0)
    start = min(max(case["offset"] + max(current_time - case["when"], 0.0) * cpr, 0.0), dur)
    if case["loop"]:
        lo, hi = min(max(case["loop_start"], 0.0), dur), (dur if case["loop_end"] <= 0.0 or case["loop_end"] > dur else case["loop_end"])
        if not lo < hi:
            lo, hi = 0.0, dur
        start = min(start, hi) if cpr >= 0.0 else max(start, lo)
    if cpr >= 0.0:
        return start >= dur
    return not case["loop"] and start >= dur and start + cpr / sr < 0.0


def case_buffer(case, instance=0):
    """[channels, frames] of white noise, one stream per (case seed, instance)"""
    return white_noise(1, case["channels"], case["frames"], seed0=0xA0D10 + 7919 * case["seed"], first=instance)[0]


def apply_case(src, case, instance=ALL, buffer=None):
    """the control calls of one case on `src` — for every context of the batch or for one"""
    if buffer is not None:
        src.set_buffer(waa.AudioBuffer(buffer, case["buffer_rate"]), instance=instance)
    src.playback_rate.set_value(case["rate"], instance=instance)
    src.detune.set_value(case["detune"], instance=instance)
    src.set_loop(case["loop"], instance=instance)
    src.set_loop_start(case["loop_start"], instance=instance)
    src.set_loop_end(case["loop_end"], instance=instance)
    src.start_at_with_offset_and_duration(case["when"], case["offset"], F64_MAX if case["duration"] is None else case["duration"], instance=instance)
    if case["stop"] is not None:
        src.stop_at(case["stop"], instance=instance)


def source_graph(binding, cases, buffers, tail=None, device=-1, n_out=None, setup=None):
    """A batch of len(cases) contexts: source -> tail(ctx, src) -> destination, case i and buffer i on context i (one case object
    repeated: a shared schedule, set with ALL).  buffers: a list of [channels, frames] arrays (through set_buffer per context), one
    array of [n, channels, frames] (set_buffer_batch) or one AudioBuffer shared by all.  setup(ctx, src): further calls on the source."""
    c0 = cases[0]
    ctx = waa.OfflineAudioContext(n_out or c0["channels"], c0["length"], c0["sr"], n_instances=len(cases), binding=binding, device=device)
    src = ctx.create_buffer_source()
    shared = all(c is c0 for c in cases)
    if isinstance(buffers, waa.AudioBuffer):
        src.set_buffer(buffers)
    elif isinstance(buffers, np.ndarray):
        src.set_buffer_batch(buffers, c0["buffer_rate"])
    elif buffers is not None:
        for i, buf in enumerate(buffers):
            src.set_buffer(waa.AudioBuffer(buf, cases[i]["buffer_rate"]), instance=i)
    if shared:
        apply_case(src, c0)
    else:
        for i, case in enumerate(cases):
            apply_case(src, case, instance=i)
    if setup is not None:
        setup(ctx, src)
    node = src if tail is None else tail(ctx, src)
    node.connect(ctx.destination())
    return ctx, src


def render(binding, *a, **kw):
    ctx, _ = source_graph(binding, *a, **kw)
    out = ctx.start_rendering_sync().data
    ctx.close()
    return out


def source_records(measure, ctx, src, instance=0):
    """(mode[n_quanta], prev, next, k [n_quanta * 128]) that the plan of a plan-only batch uploaded for `instance`"""
    fn = measure.lib.waa_debug_source_records
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    ctx.plan_describe()  # (plans)
    nq = (ctx.length + RQ - 1) // RQ
    mode = np.zeros(nq, np.uint32)
    prev, nxt, k = np.zeros(nq * RQ, np.int64), np.zeros(nq * RQ, np.int64), np.zeros(nq * RQ, np.float64)
    measure.check(fn(ctx._handle, src.id, instance, mode.ctypes.data_as(C.POINTER(C.c_uint32)), prev.ctypes.data_as(C.POINTER(C.c_int64)),
                     nxt.ctypes.data_as(C.POINTER(C.c_int64)), k.ctypes.data_as(C.POINTER(C.c_double))))
    return mode, prev, nxt, k


def case_records(measure, case, instance=0):
    ctx, src = source_graph(measure, [case], [case_buffer(case)], device=waa.PLAN_ONLY)
    rec = source_records(measure, ctx, src, instance)
    ctx.close()
    return rec


def record_kinds(mode, prev, nxt, k):
    """which of the six record kinds a table holds"""
    slow = np.repeat(mode == Q_SLOW, RQ) & (prev >= 0)
    kinds = set()
    if (mode == Q_FAST).any():
        kinds.add("fast")
    if (mode == Q_FAST_LOOP).any():
        kinds.add("fast-loop")
    if (slow & (nxt >= 0)).any():
        kinds.add("slow next>=0")
    if (slow & (nxt == -1)).any():
        kinds.add("slow next==-1")
    if (slow & (nxt == -2)).any():
        kinds.add("slow next==-2")
    if (mode == Q_SILENT).any() or (np.repeat(mode == Q_SLOW, RQ) & (prev < 0)).any():
        kinds.add("silent")
    return kinds


def evaluate_records(rec, buf, length):
    """[channels, length] f32: what a reader makes of the records — fast quanta read start + i (wrapped when looping, nothing
    behind the end otherwise), slow ones (1 - k) * prev + k * next with next = the sample, 0 or 2 * prev - buf[prev - 1];
    float64, rounded once"""
    mode, prev, nxt, k = rec
    frames = buf.shape[1]
    b64 = buf.astype(np.float64)
    fmode = np.repeat(mode, RQ)
    p = prev.copy()
    fast_loop = fmode == Q_FAST_LOOP
    p[fast_loop] %= frames
    p[(fmode == Q_FAST) & (p >= frames)] = -1
    p[fmode == Q_SILENT] = -1
    live = p >= 0
    assert (p[live] < frames).all() and (nxt[live] < frames).all() and (nxt >= -2).all(), "a record names a frame outside the buffer"
    assert (p[live & (nxt == -2)] >= 1).all(), "an extrapolated record without a frame in front of prev"
    pc = np.clip(p, 0, frames - 1)
    ps = b64[:, pc]
    ns = np.where(nxt >= 0, b64[:, np.clip(nxt, 0, frames - 1)], np.where(nxt == -1, 0.0, 2.0 * ps - b64[:, np.clip(pc - 1, 0, frames - 1)]))
    out = np.where(live, (1.0 - k) * ps + k * ns, 0.0)
    return out[:, :length].astype(np.float32)


def assert_within_one_spacing(got, want, what):
    """|got - want| <= one f32 spacing of the larger magnitude at every sample (both sides round one f64 expression once: only a
    fused against an unfused evaluation can move the rounding, by one step); returns whether the arrays are bit-identical"""
    assert_all_finite(got, what)
    assert_all_finite(want, what + " (reference)")
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.size == 0:
        return True
    big = np.maximum(np.abs(got), np.abs(want)).astype(np.float32)
    excess = np.abs(got.astype(np.float64) - want.astype(np.float64)) - np.spacing(big).astype(np.float64)
    assert_le(excess.max(), 0.0, what + f": worst sample at {np.unravel_index(int(np.argmax(excess)), got.shape)}")
    return bool(np.array_equal(got, want))


def ran(ctx, slot):
    """launches of the profile slot(s) whose name starts with `slot` (call after the render of a context with profile() on)"""
    return sum(launches for name, launches, _ in ctx.profile_entries() if name.startswith(slot))
