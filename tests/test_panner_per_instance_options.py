"""PannerNode with one set of distance and cone OPTIONS per context of a batch (waa_panner_set_options_instance,
include/waa_hip_device.h): distance model, ref / max distance, rolloff, the cone's two angles and its outer gain.

CPU part: the refusals of the C ABI and of api.py, the rule that keeps existing plans (every instance given the same set plans word for
word as the shared option, on the host-geometry path, under an audio-rate listener and for HRTF), the plan lines of batches whose sets
differ, mixed.py's buckets, the code objects of the two geometry kernels.

GPU part (-m gpu): the geometries, option sets, inputs, model, oracle and bounds are those of tests/test_panner_geometry.py (one context
per row of its ROWS, 25 contexts x 1541 frames).  (8) the SAME BITS as a single-option batch: context i of a batch in which context i
has OPTIONS[(i + s) % 13] against context i of the batch rendered with that set shared — the host rows come from one host function and
the per-frame rows from one device function (panner_geom_frame, waa_panner_geom.hpp), read by the same consumers, so nothing but
equality is right; 1664 table frames per row are 6.5 blocks of panner_geom_inst_kernel, so blocks straddle two contexts with two
distance models.  (9) against tests/panner_model.py and the oracle rendered with context i's set.  (10) 67 contexts and 1 context.
(11) HRTF.  (12) the panner in a dynamic-count plan, inside a feedback loop and in a Biquad -> Panner -> Gain chain.  (13) re-arm,
(14) render_sharded, (15) mixed.render_contexts."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import test_launch_list as tl
import test_panner_geometry as tg
import web_audio_api_rs_amd as waa
from graphs import assert_all_finite, assert_le, rms_err, white_noise
from test_panner_geometry import MAX_TOL, OPTIONS, ROWS, TOL, model, noise, oracle, row_params

RQ = 128
SR = tg.SR
FRAMES = tg.FRAMES
N = len(ROWS)
N_SETS = len(OPTIONS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-audio-api-rs_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
gpu = pytest.mark.gpu
NOTE = "one option set per instance:"
REFUSAL = ("one PannerNode option set per instance is a feature of the device library; this binding keeps one set per batch (render it "
           "one context at a time)")
MODELS = ("linear", "inverse", "exponential")
assert N == 25 and N_SETS == 13 and FRAMES == 1541 and [waa.api.DISTANCE_MODEL[m] for m in MODELS] == [0, 1, 2]


def sets_of(n, shift=0):
    """context i renders with OPTIONS[(i + shift) % 13]"""
    return [(i + shift) % N_SETS for i in range(n)]


def note_of(node, sets):
    """the plan's line for a node whose contexts render with OPTIONS[sets[i]]"""
    names = [OPTIONS[s]["distance_model"] for s in sets]
    per_model = " ".join(f"{m} x{names.count(m)}" for m in MODELS if m in names)
    return f"panner node {node}: {NOTE} {len(set(sets))} distinct set(s) ({per_model})"


def give_options(pn, sets, one_by_one=False):
    """every context its own set where the sets differ (or where asked to); else the shared option"""
    if len(set(sets)) > 1 or one_by_one:
        pn.set_options_batch([OPTIONS[s] for s in sets])
    else:
        pn.set_options(**OPTIONS[sets[0]])


def set_row_params(pn, listener, idx, path):
    """instance k: the fifteen params of ROWS[idx[k] % 25], as tests/test_panner_geometry.py::render sets them"""
    for k, i in enumerate(idx):
        for prm, v in zip(pn.params + listener.params, row_params(ROWS[i % N], path)):
            prm.set_value(v if np.isscalar(v) else v[0], instance=k)
            if not np.isscalar(v):
                prm.set_block(v[1], v[2], instance=k)


def table(be, sets, nch, path, idx=None, device=-1, one_by_one=False, first_option=None):
    """source -> PannerNode -> destination, the graph of tests/test_panner_geometry.py::render.  idx: the contexts this batch holds
    (default 0 .. len(sets) - 1); context i: row i % 25 with its noise, option set OPTIONS[sets[i]]"""
    idx = list(range(len(sets))) if idx is None else list(idx)
    ctx = waa.OfflineAudioContext(2, FRAMES, SR, n_instances=len(idx), binding=be, device=device)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(np.ascontiguousarray(noise(nch)[[i % N for i in idx]]), SR)
    pn = ctx.create_panner(panning_model="equalpower", **(first_option or {}))
    give_options(pn, [sets[i] for i in idx], one_by_one)
    set_row_params(pn, ctx.listener(), idx, path)
    src.connect(pn).connect(ctx.destination())
    src.start()
    return ctx, pn


def render(ctx):
    out = ctx.start_rendering_sync().data
    ctx.close()
    return out


def plan_lines(ctx):
    """the plan's text without the timing figures of its first line"""
    lines = ctx.plan_describe().splitlines()
    return [lines[0].split(" | timing:")[0]] + lines[1:]


def slots(ctx):
    """the names of the plan's profile slots: the kernels its launches run (the plan's text names launches, not kernels)"""
    ctx.prepare()
    return {name for name, _, _ in ctx.profile_entries()}


def assert_words(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32, (what, got.shape, ref.shape)
    diff = got.view(np.uint32) != ref.view(np.uint32)
    if diff.any():
        k = tuple(int(v) for v in np.unravel_index(int(np.argmax(diff)), diff.shape))
        raise AssertionError(f"{what}: {int(diff.sum())} of {got.size} words differ from the single-option batch; the first at {k}: "
                             f"{got[k]!r} against {ref[k]!r}")


def assert_heard(a, what):
    assert_all_finite(a, what)
    assert float(np.abs(a).max()) > 1e-3, f"{what}: silent"


# ----------------------------------------------------------------------------------------------------------- CPU: the C ABI
def opts_struct(o, reserved=0, model=None):
    return waa.api.PannerOptions(waa.api.DISTANCE_MODEL[o["distance_model"]] if model is None else model, reserved, o["ref_distance"],
                                 o["max_distance"], o["rolloff_factor"], o["cone_inner_angle"], o["cone_outer_angle"], o["cone_outer_gain"])


def _raw_batch(hip, n_inst, kind=None, frames=RQ * 8):
    """BufferSource -> Panner (or `kind`) -> destination through the C ABI, plan-only; the panner's desc is all zero: the linear model (i[1] = 0) with the default values"""
    nodes = (waa.api.NodeDesc * 3)()
    nodes[0].kind, nodes[1].kind, nodes[2].kind = waa.api.NODE_DESTINATION, waa.api.NODE_BUFFER_SOURCE, kind or waa.api.NODE_PANNER
    edges = (waa.api.EdgeDesc * 2)()
    edges[0].from_, edges[0].to = 1, 2
    edges[1].from_, edges[1].to = 2, 0
    g = waa.api.GraphDesc(3, nodes, 2, edges)
    h = C.c_void_p()
    hip.check(hip.batch_create(C.byref(g), n_inst, 2, frames, SR, waa.PLAN_ONLY, C.byref(h)))
    hip.check(hip.source_set_buffer_batch(h, 1, waa.api._fp(white_noise(n_inst, 2, frames)), 2, frames, SR))
    return h


def _describe(hip, h):
    need = C.c_size_t()
    st = hip.plan_describe(h, None, 0, C.byref(need))
    if st:
        return st, hip.last_error().decode()
    buf = C.create_string_buffer(need.value + 1)
    hip.check(hip.plan_describe(h, buf, need.value + 1, None))
    return 0, buf.value.decode()


def test_entry_point_is_declared_and_exported(hip):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "waa_hip_device.h")).read(), flags=re.S)
    assert re.search(r"\bwaa_panner_set_options_instance\s*\(", text) and re.search(r"\}\s*waa_panner_options\s*;", text)
    assert "panner_set_options_instance" in waa.api.ABI_DEVICE
    assert hasattr(C.CDLL(waa.LIB_PATH), "waa_panner_set_options_instance")
    assert C.sizeof(waa.api.PannerOptions) == 56
    shared = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "waa_hip.h")).read(), flags=re.S)
    assert "waa_panner_set_options_instance" not in shared  # (the boundary the oracle exports too stays as it is)


def test_abi_refusals(hip):
    ALL = waa.api.ALL
    good = OPTIONS[1]
    h = _raw_batch(hip, 3)
    try:
        f = lambda node, inst, o: hip.panner_set_options_instance(h, node, inst, C.byref(o) if o is not None else None)  # noqa: E731
        assert f(2, 3, opts_struct(good)) == 1 and b"instance 3 out of range (PannerNode 2, 3 instances)" in hip.last_error()
        assert f(1, 0, opts_struct(good)) == 1 and b"not of the expected kind" in hip.last_error()  # a source
        assert f(7, 0, opts_struct(good)) == 1                                                      # no such node
        assert f(2, 0, None) == 1 and b"null options" in hip.last_error()
        assert f(2, 0, opts_struct(good, reserved=1)) == 1 and b"reserved" in hip.last_error()
        for inst in (1, ALL):
            for bad in (-1, 3, 100):
                assert f(2, inst, opts_struct(good, model=bad)) == 1 and hip.last_error() == b"bad distance model", bad
            for field, value, status, msg in (("ref_distance", -0.5, 1, b"RangeError - refDistance cannot be negative"),
                                              ("ref_distance", float("nan"), 1, b"RangeError - refDistance cannot be negative"),
                                              ("max_distance", 0.0, 1, b"RangeError - maxDistance must be strictly positive"),
                                              ("max_distance", -3.0, 1, b"RangeError - maxDistance must be strictly positive"),
                                              ("rolloff_factor", -1e-9, 1, b"RangeError - rolloffFactor cannot be negative"),
                                              ("cone_outer_gain", 1.5, 3, b"InvalidStateError - coneOuterGain must be in the range [0, 1]"),
                                              ("cone_outer_gain", -0.1, 3, b"InvalidStateError - coneOuterGain must be in the range [0, 1]")):
                assert f(2, inst, opts_struct(dict(good, **{field: value}))) == status and hip.last_error() == msg, (inst, field, value)
        # there is no all-zero-means-defaults shorthand here: zeros are checked as given
        zeros = waa.api.PannerOptions(1, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
        assert f(2, 0, zeros) == 1 and hip.last_error() == b"RangeError - maxDistance must be strictly positive"
        # (a refused call leaves the node as it was: one set everywhere, no note)
        st, msg = _describe(hip, h)
        assert st == 0 and NOTE not in msg, msg
        assert f(2, 1, opts_struct(good)) == 3 and b"frozen" in hip.last_error()  # InvalidStateError once the batch is planned
    finally:
        hip.batch_destroy(h)
    h = _raw_batch(hip, 2, kind=waa.api.NODE_GAIN)
    try:
        assert hip.panner_set_options_instance(h, 2, 0, C.byref(opts_struct(good))) == 1 and b"not of the expected kind" in hip.last_error()
    finally:
        hip.batch_destroy(h)


def _raw_note(hip, calls, n_inst=4):
    h = _raw_batch(hip, n_inst)
    try:
        for inst, s in calls:
            hip.check(hip.panner_set_options_instance(h, 2, inst, C.byref(opts_struct(OPTIONS[s]))))
        st, msg = _describe(hip, h)
        assert st == 0, msg
        notes = [l for l in msg.splitlines() if NOTE in l]
        assert len(notes) <= 1, msg
        return notes[0] if notes else None
    finally:
        hip.batch_destroy(h)


def test_all_and_single_instances_in_either_order(hip):
    ALL = waa.api.ALL
    # OPTIONS[0..4] linear, [5..8] inverse, [9..12] exponential; the batch is created with an all-zero desc: i[1] = 0 is linear
    # ALL, then single instances: the singles keep theirs, the others follow ALL
    want = "panner node 2: one option set per instance: 3 distinct set(s) (linear x1 inverse x1 exponential x2)"
    assert _raw_note(hip, [(ALL, 9), (1, 0), (3, 5)]) == want
    # single instances, then ALL: ALL replaces the shared set and leaves the sets given to single instances in force
    assert _raw_note(hip, [(1, 0), (3, 5), (ALL, 9)]) == want
    # an instance without a set of its own uses the shared one of waa_batch_create
    assert _raw_note(hip, [(0, 10)]) == "panner node 2: one option set per instance: 2 distinct set(s) (linear x3 exponential x1)"
    # two sets of one distance model are two sets
    assert _raw_note(hip, [(0, 1), (1, 2), (2, 1), (3, 1)]) == "panner node 2: one option set per instance: 2 distinct set(s) (linear x4)"
    # a second call for one instance wins
    assert _raw_note(hip, [(ALL, 5), (0, 0), (0, 9), (2, 1), (2, 9)]) == "panner node 2: one option set per instance: 2 distinct set(s) (inverse x2 exponential x2)"
    # ... also back to the shared set: no instance differs, no note
    assert _raw_note(hip, [(ALL, 5), (0, 0), (0, 5)]) is None
    assert _raw_note(hip, [(ALL, 3), (ALL, 4)]) is None
    assert _raw_note(hip, [(i, 7) for i in range(4)]) is None


# ------------------------------------------------------------------------------------------------------------- CPU: api.py
def test_api_calls_and_refusals(hip, orc):
    ctx, pn = table(hip, [5, 5, 5], 2, "host", device=waa.PLAN_ONLY)
    assert not pn.per_instance and pn.options_of(2) == OPTIONS[5]
    for i in (3, -2):
        with pytest.raises(waa.WaaError, match="out of range") as e:
            pn.set_options(instance=i, rolloff_factor=2.0)
        assert e.value.status == 1
        with pytest.raises(waa.WaaError, match="out of range"):
            pn.options_of(i)
    for fields, status, msg in ((dict(distance_model="cubic"), 1, "bad distance model"),
                                (dict(ref_distance=-1.0), 1, "RangeError - refDistance cannot be negative"),
                                (dict(max_distance=0.0), 1, "RangeError - maxDistance must be strictly positive"),
                                (dict(rolloff_factor=-0.5), 1, "RangeError - rolloffFactor cannot be negative"),
                                (dict(rolloff_factor=1.0, cone_outer_gain=1.01), 3, "InvalidStateError - coneOuterGain must be in the range [0, 1]")):
        with pytest.raises(waa.WaaError) as e:
            pn.set_options(instance=1, **fields)
        assert e.value.status == status and msg in str(e.value) and not pn.per_instance, fields
    for inst in (1, waa.api.ALL):
        with pytest.raises(TypeError, match="panning_model"):
            pn.set_options(instance=inst, panning_model="HRTF")  # (not an option of this kind: it stays one per node)
    with pytest.raises(waa.WaaError) as e:
        pn.set_options_batch([OPTIONS[0]] * 2)  # (two sets for three contexts)
    assert e.value.status == 1 and not pn.per_instance
    # options_of resolves the overlay when asked: the order of the calls does not matter
    pn.set_options(instance=1, rolloff_factor=0.25, distance_model="linear")
    pn.set_options(instance=1, rolloff_factor=0.75)  # (the last call for a field wins)
    pn.set_options(max_distance=40.0, rolloff_factor=3.0)  # ALL, after the instance's: plain attributes
    assert pn.max_distance == 40.0 and pn.rolloff_factor == 3.0 and pn.per_instance
    assert pn.options_of(1) == dict(OPTIONS[5], distance_model="linear", rolloff_factor=0.75, max_distance=40.0)
    assert pn.options_of(0) == pn.options_of(2) == dict(OPTIONS[5], max_distance=40.0, rolloff_factor=3.0)
    other, pn2 = table(hip, [5, 5, 5], 2, "host", device=waa.PLAN_ONLY)
    pn2.set_options(max_distance=40.0, rolloff_factor=3.0)
    pn2.set_options(instance=1, rolloff_factor=0.75, distance_model="linear")
    assert [pn2.options_of(i) for i in range(3)] == [pn.options_of(i) for i in range(3)]
    other.close()
    assert [l for l in plan_lines(ctx) if NOTE in l] == ["panner node 2: one option set per instance: 2 distinct set(s) (linear x1 inverse x2)"]
    with pytest.raises(waa.WaaError, match="frozen") as e:  # after the plan
        pn.set_options(instance=2, rolloff_factor=1.0)
    assert e.value.status == 3
    ctx.close()
    # the oracle keeps one set per batch: differing sets are refused, never rendered with one instance's set
    ctx, pn = table(orc, [5, 5, 5], 2, "host")
    pn.set_options(instance=1, rolloff_factor=0.25)
    with pytest.raises(waa.WaaError) as e:
        ctx.start_rendering_sync()
    assert e.value.status == 4 and str(e.value).endswith(REFUSAL), str(e.value)
    # ... and equal ones collapse to the shared set and render the same bits
    got = render(table(orc, [3, 3, 3], 2, "host", one_by_one=True, first_option=OPTIONS[5])[0])
    ref = render(table(orc, [3, 3, 3], 2, "host")[0])
    assert np.array_equal(got, ref) and float(np.abs(ref).max()) > 1e-3
    assert not np.array_equal(ref, render(table(orc, [5, 5, 5], 2, "host")[0]))


# --------------------------------------------------------------------------------------------- CPU: the rule that keeps existing plans
HRTF_SR = 44100.0  # (the rate of the sphere as tests/test_hrtf.py loads it)
HRTF_FRAMES = 18 * RQ + 5  # (16 quanta and more: a panner at rest renders in the transform form on the device)
HRTF_SETS = [5, 1, 6, 1, 5]  # the default-like inverse law without a cone; linear with a cone that attenuates; inverse with a negative-angle cone


def hrtf_position(i):
    return (1.0 + 0.3 * i, 0.4 - 0.2 * i, -1.0 + 0.5 * i)


def hrtf(be, sets, form, idx=None, device=-1, one_by_one=False):
    """source (mono) -> HRTF PannerNode -> destination at 44.1 kHz.  form "shared": one direction for the batch (all fifteen params
    shared); "static": a position per context; "moving": a position per context and quantum (k-rate).  The orientation points away
    from the listener off the axis, so a cone attenuates."""
    idx = list(range(len(sets))) if idx is None else list(idx)
    nq = (HRTF_FRAMES + RQ - 1) // RQ
    ctx = waa.OfflineAudioContext(2, HRTF_FRAMES, HRTF_SR, n_instances=len(idx), binding=be, device=device)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(np.ascontiguousarray(white_noise(len(sets), 1, HRTF_FRAMES, seed0=0x48F)[idx]), HRTF_SR)
    pn = ctx.create_panner(panning_model="HRTF", position=hrtf_position(0), orientation=(0.3, 0.2, 1.0))
    give_options(pn, [sets[i] for i in idx], one_by_one)
    if form != "shared":
        for k, i in enumerate(idx):
            for prm, v in zip(pn.params[:3], hrtf_position(i)):
                prm.set_value(v, instance=k)
            if form == "moving":
                pn.position_x.set_block(0, (hrtf_position(i)[0] + 0.4 * np.arange(nq)).astype(np.float32), instance=k)
    src.connect(pn).connect(ctx.destination())
    src.start()
    return ctx, pn


def shared_listener_ramp(be, sets, device=-1, one_by_one=False):
    """the table's graph with all fifteen params shared by the batch and ONE audio-rate block on the listener's positionX"""
    ctx = waa.OfflineAudioContext(2, FRAMES, SR, n_instances=len(sets), binding=be, device=device)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(np.ascontiguousarray(noise(2)[:len(sets)]), SR)
    pn = ctx.create_panner(panning_model="equalpower", position=(1.3, 0.8, -2.1), orientation=(0.3, -0.2, 1.0))
    give_options(pn, sets, one_by_one)
    ctx.listener().position_x.set_block(3, np.linspace(-4.0, 4.0, 6 * RQ).astype(np.float32).reshape(6, RQ))
    src.connect(pn).connect(ctx.destination())
    src.start()
    return ctx, pn


@pytest.mark.parametrize("opt", range(N_SETS), ids=tg.OPTION_IDS)
def test_equal_sets_plan_as_the_shared_option(hip, opt):
    """every instance set one by one to the same set (not the set the node was created with): the plan's text is the shared option's,
    word for word — the host geometry, the audio-rate listener with a row per context and with one row for the batch, and HRTF"""
    n = 5
    other = OPTIONS[(opt + 6) % N_SETS]
    builds = {
        "host": (lambda one: table(hip, [opt] * n, 2, "host", device=waa.PLAN_ONLY, one_by_one=one, first_option=other if one else None), None),
        "device": (lambda one: table(hip, [opt] * n, 2, "device", device=waa.PLAN_ONLY, one_by_one=one, first_option=other if one else None),
                   f"per-frame geometry on the device ({n} table row(s))"),
        "device, one row": (lambda one: shared_listener_ramp(hip, [opt] * n, device=waa.PLAN_ONLY, one_by_one=one),
                            "per-frame geometry on the device (1 table row(s))"),
        "hrtf": (lambda one: hrtf(hip, [opt] * n, "shared", device=waa.PLAN_ONLY, one_by_one=one), "geometry table 1 row(s) x 1"),
        "hrtf, moving": (lambda one: hrtf(hip, [opt] * n, "moving", device=waa.PLAN_ONLY, one_by_one=one), f"geometry table {n} row(s) x"),
    }
    for name, (build, marker) in builds.items():
        texts = []
        for one_by_one in (False, True):
            ctx, pn = build(one_by_one)
            assert pn.per_instance == one_by_one
            texts.append(plan_lines(ctx))
            assert "panner_geom_inst_kernel" not in slots(ctx) and ("panner_geom_kernel" in slots(ctx)) == name.startswith("device"), name
            ctx.close()
        assert texts[0] == texts[1], name
        assert marker is None or any(marker in l for l in texts[0]), (name, texts[0])
        assert ("audio-rate AudioListener automation" in "\n".join(texts[0])) == name.startswith("device"), (name, texts[0])
        assert not any(NOTE in l or "because of the options" in l for l in texts[0]), (name, texts[0])


# ------------------------------------------------------------------------------------------------------ CPU: plans of differing sets
def late_source(be, sets, idx=None, device=-1):
    """the panner in a dynamic-count plan: a mono source from t = 0 and a stereo one that joins late, per context at a sub-quantum
    time of its own (tests/test_biquad_per_instance_type.py)"""
    idx = list(range(len(sets))) if idx is None else list(idx)
    frames = RQ * 20 + 50
    mono, stereo = white_noise(len(sets), 1, frames, seed0=11) * 0.5, white_noise(len(sets), 2, RQ * 8, seed0=12) * 0.5
    ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=len(idx), binding=be, device=device)
    a, b = ctx.create_buffer_source(), ctx.create_buffer_source()
    a.set_buffer_batch(np.ascontiguousarray(mono[idx]), SR)
    b.set_buffer_batch(np.ascontiguousarray(stereo[idx]), SR)
    pn = ctx.create_panner(panning_model="equalpower", orientation=(0.3, -0.2, 1.0))
    give_options(pn, [sets[i] for i in idx])
    for k, i in enumerate(idx):
        for prm, v in zip(pn.params[:3], (1.5 + 0.6 * i, 0.2 * i, -1.0 - 0.8 * i)):
            prm.set_value(v, instance=k)
        b.start_at(RQ * 5.5 / SR + i * 300.0 / SR, instance=k)
    a.connect(pn)
    b.connect(pn)
    pn.connect(ctx.destination())
    a.start()
    return ctx, pn


def in_a_loop(be, sets, idx=None, device=-1):
    """the panner inside a feedback loop (tests/test_launch_list.py::g_listener_automated_in_a_loop without the listener's ramp):
    source -> Delay -> Panner -> Gain -> back into the Delay"""
    idx = list(range(len(sets))) if idx is None else list(idx)
    frames = RQ * 24 + 7
    ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=len(idx), binding=be, device=device)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(np.ascontiguousarray(white_noise(len(sets), 2, frames, seed0=38)[idx]), SR)
    delay, pn, fb = ctx.create_delay(0.1), ctx.create_panner(panning_model="equalpower", orientation=(0.3, -0.2, 1.0)), ctx.create_gain(gain=0.5)
    give_options(pn, [sets[i] for i in idx])
    for k, i in enumerate(idx):
        delay.delay_time.set_value(float(np.float32((300 + 17.5 * i) / SR)), instance=k)
        for prm, v in zip(pn.params[:3], (1.0 + 0.7 * i, 0.1 * i, -1.0 - 0.6 * i)):
            prm.set_value(v, instance=k)
    src.connect(delay)
    delay.connect(pn).connect(fb).connect(delay)
    pn.connect(ctx.destination())
    src.start()
    return ctx, pn


def filter_chain(be, sets, idx=None, device=-1):
    """source -> Biquad -> Panner -> Gain -> destination: the panner as one op of a chain"""
    idx = list(range(len(sets))) if idx is None else list(idx)
    frames = RQ * 12 + 9
    ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=len(idx), binding=be, device=device)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(np.ascontiguousarray(white_noise(len(sets), 2, frames, seed0=52)[idx]), SR)
    pn = ctx.create_panner(panning_model="equalpower", orientation=(0.3, -0.2, 1.0))
    give_options(pn, [sets[i] for i in idx])
    nq = (frames + RQ - 1) // RQ
    for k, i in enumerate(idx):
        pn.position_x.set_value(1.0 + 0.5 * i, instance=k)
        pn.position_z.set_block(0, (-1.0 - 0.3 * i - 0.2 * np.arange(nq)).astype(np.float32), instance=k)  # k-rate
    src.connect(ctx.create_biquad_filter(type_="lowpass", frequency=2000.0)).connect(pn).connect(ctx.create_gain(gain=0.5)).connect(ctx.destination())
    src.start()
    return ctx, pn


PLACES = {"late_source": (late_source, "dynamic-count group"), "in_a_loop": (in_a_loop, "loop"), "filter_chain": (filter_chain, "chain")}
PLACE_SETS = [0, 6, 10, 3, 7, 12, 6]  # 7 contexts, 6 distinct sets, all three distance models, cones that attenuate


def test_differing_sets_plan_lines(hip):
    sets = sets_of(N)
    assert note_of(2, sets) == "panner node 2: one option set per instance: 13 distinct set(s) (linear x10 inverse x8 exponential x7)"
    # host geometry: the gain tables were per instance already; no geometry kernel
    ctx, _ = table(hip, sets, 2, "host", device=waa.PLAN_ONLY)
    lines, kernels = plan_lines(ctx), slots(ctx)
    ctx.close()
    assert [l for l in lines if NOTE in l] == [note_of(2, sets)], lines
    assert not any("audio-rate AudioListener automation" in l for l in lines) and not any(k.startswith("panner_geom") for k in kernels), lines
    # an audio-rate listener, the params per instance: the tables were per instance already
    ctx, _ = table(hip, sets, 2, "device", device=waa.PLAN_ONLY)
    lines, kernels = plan_lines(ctx), slots(ctx)
    ctx.close()
    assert "panner_geom_inst_kernel" in kernels and "panner_geom_kernel" not in kernels, kernels  # the same launch, the other kernel
    assert [l for l in lines if NOTE in l] == [note_of(2, sets)], lines
    assert "panner node 2: audio-rate AudioListener automation -> per-frame geometry on the device (25 table row(s))" in lines, lines
    # all fifteen params shared by the batch: the single-option batch has one row, the mixed one a row per context
    ctx, _ = shared_listener_ramp(hip, sets, device=waa.PLAN_ONLY)
    lines = plan_lines(ctx)
    ctx.close()
    assert [l for l in lines if NOTE in l] == [note_of(2, sets)], lines
    assert ("panner node 2: audio-rate AudioListener automation -> per-frame geometry on the device (25 table row(s)); per instance "
            "because of the options") in lines, lines
    # HRTF, one direction for the batch: a geometry row per context
    ctx, _ = hrtf(hip, sets, "shared", device=waa.PLAN_ONLY)
    lines = plan_lines(ctx)
    ctx.close()
    assert [l for l in lines if NOTE in l] == [note_of(2, sets)], lines
    assert any(l.startswith("panner node 2: HRTF") and "geometry table 25 row(s) x 1," in l for l in lines), lines


@pytest.mark.parametrize("place", list(PLACES))
def test_differing_sets_plan_where_a_panner_already_renders(hip, place):
    build, marker = PLACES[place]
    ctx, pn = build(hip, PLACE_SETS, device=waa.PLAN_ONLY)
    lines = plan_lines(ctx)
    ctx.close()
    assert [l for l in lines if NOTE in l] == [note_of(pn.id, PLACE_SETS)], lines  # (one line, however often the geometry is evaluated)
    assert any(marker in l for l in lines), lines
    ctx, _ = build(hip, [6] * len(PLACE_SETS), device=waa.PLAN_ONLY)
    same = plan_lines(ctx)
    ctx.close()
    assert [l for l in lines if NOTE not in l] == same  # nothing but the note differs from the single-option plan


@pytest.mark.measure
def test_launch_lists_with_a_panner_are_what_they_were(hip, monkeypatch):
    """the graphs of tests/test_launch_list.py that contain a PannerNode, with the feature unused: their golden sections (the launch
    list is a switch of the measurement build)"""
    named, dyn = tl._sections(tl._golden("named")), tl._sections(tl._golden("dyn_items"))
    for name in ("listener_automated_in_a_loop", "qloop_hrtf"):
        build, switches = tl.NAMED[name]
        assert tl.describe(hip, build, switches, monkeypatch.setenv, monkeypatch.delenv) == named[name], name
    assert "panner_geom" in named["listener_automated_in_a_loop"]
    for name in ("equal_power_panner", "hrtf_behind_its_group"):
        build, switches = tl.DYN_ITEMS[name]
        assert tl.describe(hip, build, dict(switches, WAA_PLAN_DYN_ITEMS="1"), monkeypatch.setenv, monkeypatch.delenv) == dyn[name], name


# --------------------------------------------------------------------------------------------------------------- CPU: mixed.py
def _single(binding, opt, i, device=-1, panning_model="equalpower", sr=SR):
    """one context of the reference: BufferSource -> PannerNode(its own options and position) -> destination"""
    ctx = waa.OfflineAudioContext(2, FRAMES, sr, binding=binding, device=device)
    src = ctx.create_buffer_source()
    src.set_buffer(waa.AudioBuffer(white_noise(1, 2, FRAMES, first=i)[0], sr))
    pn = ctx.create_panner(panning_model=panning_model, position=(1.0 + 0.4 * i, 0.3, -1.0 - 0.2 * i), orientation=(0.3, -0.2, 1.0), **OPTIONS[opt])
    src.connect(pn).connect(ctx.destination())
    src.start()
    return ctx


def test_mixed_buckets(hip, orc):
    from web_audio_api_rs_amd.mixed import bucket_report

    def requests(binding, **kw):
        return [_single(binding, opt, i, device=waa.PLAN_ONLY if binding is hip else -1, **kw) for i, opt in enumerate(range(N_SETS))]

    for kw in ({}, dict(panning_model="HRTF", sr=HRTF_SR)):  # contexts that differ only in their options share a bucket
        ctxs = requests(hip, **kw)
        assert bucket_report(ctxs) == [list(range(N_SETS))], kw
        for c in ctxs:
            c.close()
    ctxs = [_single(hip, i % 3, i, device=waa.PLAN_ONLY, panning_model="HRTF" if i % 2 else "equalpower") for i in range(6)]
    assert bucket_report(ctxs) == [[0, 2, 4], [1, 3, 5]]  # different panning models stay apart
    for c in ctxs:
        c.close()
    ctxs = requests(orc) + [_single(orc, 4, 13)]  # one set per batch: every set its own bucket
    assert bucket_report(ctxs) == [[i] for i in range(4)] + [[4, 13]] + [[i] for i in range(5, 13)]
    for c in ctxs:
        c.close()


def test_mixed_merge_carries_the_options(hip):
    from web_audio_api_rs_amd.mixed import _merge
    car = _merge([_single(hip, opt, i, device=waa.PLAN_ONLY) for i, opt in enumerate([3, 9, 3])])
    pn = car._nodes[2]
    assert car.n_instances == 3 and pn.per_instance and [pn.options_of(i) for i in range(3)] == [OPTIONS[3], OPTIONS[9], OPTIONS[3]]
    assert note_of(2, [3, 9, 3]) in car.plan_describe()
    car.close()
    # equal sets everywhere: the node stays shared
    car = _merge([_single(hip, 7, i, device=waa.PLAN_ONLY) for i in range(3)])
    assert not car._nodes[2].per_instance and car._nodes[2].options_of(1) == OPTIONS[7] and NOTE not in car.plan_describe()
    car.close()


# ------------------------------------------------------------------------------------------------ CPU: the kernels' code objects
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_kernel_registers_and_no_scratch(tmp_path):
    """waa_panner.hip compiled to ISA with the library's flags, read like tests/test_waveshaper_per_instance.py reads its kernel:
    exactly the two kernels; the new one spills nothing, uses no scratch memory and no LDS and at most 64 vector registers (so that
    registers never limit the eight wavefronts per SIMD a streaming kernel wants); the shared one still has no scratch and no spill"""
    out = str(tmp_path / "waa_panner.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fgpu-flush-denormals-to-zero",
                           "--cuda-device-only", "-S", os.path.join(CSRC, "waa_panner.hip"), "-o", out], stderr=subprocess.DEVNULL)
    res = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)(.*?)\.wavefront_size", open(out).read(), re.S):  # (one kernel's metadata, keys in order)
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(2)).group(1))  # noqa: E731
        res[re.search(r"\.name:\s+(\S+)", m.group(2)).group(1)] = {
            "vgpr": get("vgpr_count"), "spill": get("vgpr_spill_count"), "sgpr_spill": get("sgpr_spill_count"),
            "scratch": get("private_segment_fixed_size"), "lds": int(m.group(1))}
    print(res)
    assert sorted(res) == ["_ZN3waa18panner_geom_kernelENS_14PannerGeomDescE", "_ZN3waa23panner_geom_inst_kernelENS_14PannerGeomDescE"], res
    inst, shared = res["_ZN3waa23panner_geom_inst_kernelENS_14PannerGeomDescE"], res["_ZN3waa18panner_geom_kernelENS_14PannerGeomDescE"]
    assert inst["spill"] == 0 and inst["sgpr_spill"] == 0 and inst["scratch"] == 0 and inst["lds"] == 0 and inst["vgpr"] <= 64, inst
    assert shared["scratch"] == 0 and shared["spill"] == 0, shared


# ======================================================================================================================== GPU
# --------------------------------------------------------------------------------- 8. the same bits as a single-option batch
_SHARED = {}


def shared_render(hip, opt, nch, path):
    """tests/test_panner_geometry.py::render with OPTIONS[opt] shared by the batch, once per (set, channels, path)"""
    key = (opt, nch, path)
    if key not in _SHARED:
        out, plan = tg.render(hip, opt, nch, path)
        assert NOTE not in plan and ("audio-rate AudioListener automation" in plan) == (path == "device"), plan
        assert_heard(out, f"shared render {key}")
        out.setflags(write=False)
        _SHARED[key] = out
    return _SHARED[key]


def mixed_render(hip, sets, nch, path):
    ctx, _ = table(hip, sets, nch, path)
    plan = ctx.plan_describe()
    assert note_of(2, sets) in plan, plan
    geom = {k for k in slots(ctx) if k.startswith("panner_geom")}
    if path == "device":  # launched as the per-instance kernel
        assert geom == {"panner_geom_inst_kernel"} and "(25 table row(s))" in plan, (geom, plan)
    else:                 # no geometry kernel at all
        assert not geom and "audio-rate AudioListener automation" not in plan, (geom, plan)
    got = render(ctx)
    assert_heard(got, f"mixed sets, {nch} channel(s), {path}")
    return got


@gpu
@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("shift", range(N_SETS))
def test_same_bits_as_a_single_option_batch(hip, shift, nch, path):
    """over the 13 shifts every (row, set) pair; neighbouring contexts always differ in their set and, where a block of the kernel
    straddles two contexts (every second boundary: 1664 frames per row), mostly in their distance model"""
    sets = sets_of(N, shift)
    got = mixed_render(hip, sets, nch, path)
    for opt in range(N_SETS):
        mine = [i for i in range(N) if sets[i] == opt]
        assert mine
        assert_words(got[mine], shared_render(hip, opt, nch, path)[mine], f"shift {shift}, {nch} channel(s), {path}, set {tg.OPTION_IDS[opt]}")
    others = [i for i in range(N) if sets[i] != sets[0]]  # (the sets are heard: the other contexts against a batch of context 0's set)
    assert (got[others].view(np.uint32) != shared_render(hip, sets[0], nch, path)[others].view(np.uint32)).any()


# --------------------------------------------------------------------------------------------- 9. against the model and the oracle
def per_context(full_of, sets):
    """[context i] of full_of(sets[i]): a reference rendered once per option set, its row picked per context"""
    return np.stack([full_of(s)[i] for i, s in enumerate(sets)])


@gpu
@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("shift", [0, 7])
def test_against_model_and_oracle(hip, orc, shift, nch, path):
    """bounds: those of tests/test_panner_geometry.py, per (context, channel) RMS <= 1e-6 and max |diff| <= 5e-6; its test_input_cap
    shows on the CPU that every (set, row) pair keeps 2 * |model32 - model64| under the bound"""
    sets = sets_of(N, shift)
    got = mixed_render(hip, sets, nch, path)
    want = per_context(lambda s: model(s, nch, path, np.float32), sets)
    ref = per_context(lambda s: oracle(orc, s, nch, path), sets)
    case = f"shift {shift}-{nch}ch-{path}"
    results = [tg.check(f"{case}: device vs model", got, want), tg.check(f"{case}: device vs oracle", got, ref)]
    for i in range(N):
        assert float(np.abs(got[i]).max()) > 1e-6 or float(np.abs(want[i]).max()) <= 1e-6, f"context {i} is silent"
    for r, m in results:  # (after both legs' figures have been printed)
        assert_le(r, 1.0, "RMS, fraction of 1e-6")
        assert_le(m, 1.0, "max |diff|, fraction of 5e-6")


# ------------------------------------------------------------------------------------------------------------ 10. batch sizes
@gpu
@pytest.mark.parametrize("nch", [1, 2])
def test_67_contexts(hip, nch):
    """more than a wavefront of contexts: rows repeated, sets i % 13, under the audio-rate listener; the single-option renders are
    those of the 25-context batches (context i: row i % 25 with its noise)"""
    sets = sets_of(67)
    ctx, _ = table(hip, sets, nch, "device")
    plan = ctx.plan_describe()
    assert note_of(2, sets) in plan and "panner_geom_inst_kernel" in slots(ctx) and "(67 table row(s))" in plan, plan
    got = render(ctx)
    assert_heard(got, "67 contexts")
    for i in range(67):
        assert_words(got[i], shared_render(hip, sets[i], nch, "device")[i % N], f"context {i} of 67")


@gpu
@pytest.mark.parametrize("path", ["host", "device"])
def test_one_context_with_a_set_of_its_own(hip, path):
    ctx, pn = table(hip, [2], 2, path, one_by_one=True, first_option=OPTIONS[9])
    assert pn.per_instance
    lines = plan_lines(ctx)
    assert "panner_geom_inst_kernel" not in slots(ctx) and ("panner_geom_kernel" in slots(ctx)) == (path == "device")
    got = render(ctx)
    ctx, _ = table(hip, [2], 2, path)
    assert lines == plan_lines(ctx) and NOTE not in "\n".join(lines)
    ref = render(ctx)
    assert_heard(ref, "one context")
    assert_words(got, ref, f"one context, {path}")
    assert_words(got[0], shared_render(hip, 2, 2, path)[0], f"one context against the table's batch, {path}")


# -------------------------------------------------------------------------------------------------------------------- 11. HRTF
@gpu
@pytest.mark.parametrize("form", ["static", "moving"])
def test_hrtf_same_bits_as_single_option_batches(hip, form):
    ctx, _ = hrtf(hip, HRTF_SETS, form)
    plan = ctx.plan_describe()
    assert note_of(2, HRTF_SETS) in plan, plan
    assert ("geometry table 5 row(s) x 19," if form == "moving" else "one direction per context") in plan, plan
    got = render(ctx)
    assert_heard(got, f"HRTF, {form}")
    refs = {}
    for opt in sorted(set(HRTF_SETS)):
        ctx, _ = hrtf(hip, [opt] * len(HRTF_SETS), form)
        assert NOTE not in ctx.plan_describe()
        refs[opt] = render(ctx)
        mine = [i for i, s in enumerate(HRTF_SETS) if s == opt]
        assert_words(got[mine], refs[opt][mine], f"HRTF, {form}, set {tg.OPTION_IDS[opt]}")
    assert (refs[5][1].view(np.uint32) != refs[1][1].view(np.uint32)).any()  # (the cone and the linear law are heard)


@gpu
def test_hrtf_shared_direction_against_the_oracle(hip, orc):
    """one direction for the batch, a geometry row (on the device: a table of partition spectra) per context because of
    the options; bound: tests/test_hrtf.py's RMS <= 1e-6 per channel against the oracle, here rendered with context i's set"""
    ctx, _ = hrtf(hip, HRTF_SETS, "shared")
    plan = ctx.plan_describe()
    assert note_of(2, HRTF_SETS) in plan and "one direction per context" in plan, plan  # (a single-option batch: "for the whole batch")
    got = render(ctx)
    assert_heard(got, "HRTF, shared direction")
    refs = {opt: render(hrtf(orc, [opt] * len(HRTF_SETS), "shared")[0]) for opt in sorted(set(HRTF_SETS))}
    ref = np.stack([refs[s][i] for i, s in enumerate(HRTF_SETS)])
    assert_heard(ref, "oracle")
    r = rms_err(got, ref)
    print(f"HRTF, shared direction: worst RMS {float(r.max()):.3e} (bound 1e-6), peak {float(np.abs(ref).max()):.3f}")
    assert float(np.abs(refs[1][1] - refs[5][1]).max()) > 1e-2  # (the sets are heard: context 1 under its own set and under context 0's)
    assert_le(r.max(), 1e-6, "RMS per context and channel")


# ------------------------------------------------------------------------------------------ 12. where a panner already renders
@gpu
@pytest.mark.parametrize("place", list(PLACES))
def test_same_bits_where_a_panner_already_renders(hip, place):
    build, marker = PLACES[place]
    ctx, pn = build(hip, PLACE_SETS)
    plan = ctx.plan_describe()
    assert note_of(pn.id, PLACE_SETS) in plan and marker in plan, plan
    got = render(ctx)
    assert_heard(got, place)
    for opt in sorted(set(PLACE_SETS)):
        ctx, _ = build(hip, [opt] * len(PLACE_SETS))
        assert NOTE not in ctx.plan_describe()
        ref = render(ctx)
        mine = [i for i, s in enumerate(PLACE_SETS) if s == opt]
        assert_words(got[mine], ref[mine], f"{place}, set {tg.OPTION_IDS[opt]}")
        others = [i for i, s in enumerate(PLACE_SETS) if s != opt]
        assert (got[others].view(np.uint32) != ref[others].view(np.uint32)).any()  # (the sets really differ)


# ------------------------------------------------------------------------------------------------------------------ 13. re-arm
@gpu
@pytest.mark.parametrize("path", ["host", "device"])
def test_rearm_keeps_the_sets(hip, path):
    from rearm import assert_differs, assert_same_bits, other_dense, refill_from, render_again
    sets = sets_of(N, 3)

    def build(audio):
        ctx = waa.OfflineAudioContext(2, FRAMES, SR, n_instances=N, binding=hip)
        src = ctx.create_buffer_source()
        src.set_buffer_batch(audio, SR)
        pn = ctx.create_panner(panning_model="equalpower")
        give_options(pn, sets)
        set_row_params(pn, ctx.listener(), list(range(N)), path)
        src.connect(pn).connect(ctx.destination())
        src.start()
        return ctx

    a, b2 = np.ascontiguousarray(noise(2)), other_dense(N, 2, FRAMES)
    ctx = build(a)
    assert note_of(2, sets) in ctx.plan_describe()
    first = ctx.start_rendering_sync().data
    donor = build(b2)  # (never applied: only its audio is taken)
    assert refill_from(ctx, donor) == 1
    again = render_again(ctx)
    ctx.close()
    donor.close()
    fresh = render(build(b2))
    assert_all_finite(again, "re-armed render")
    assert_differs(again, first)
    assert_same_bits(again, fresh)


# ------------------------------------------------------------------------------------------------------------------ 14. sharded
@gpu
def test_render_sharded_slices_the_sets_by_first(hip):
    from web_audio_api_rs_amd.sharding import render_sharded
    sets = sets_of(N, 5)
    audio = np.ascontiguousarray(noise(2))
    want = mixed_render(hip, sets, 2, "device")

    def build(n_instances, device, first=0):
        idx = list(range(first, first + n_instances))
        ctx = waa.OfflineAudioContext(2, FRAMES, SR, n_instances=n_instances, binding=hip, device=device)
        src = ctx.create_buffer_source()
        pn = ctx.create_panner(panning_model="equalpower")
        pn.set_options_batch([OPTIONS[sets[i]] for i in idx])
        set_row_params(pn, ctx.listener(), idx, "device")
        src.connect(pn).connect(ctx.destination())
        src.start()
        return ctx, src

    out = np.zeros_like(want)
    info = render_sharded(build, audio, out, devices=[0], sub_batches=2, sample_rate=SR, pass_first=True)
    assert len(info["shards"]) == 2, info
    assert np.array_equal(out, want)


# ------------------------------------------------------------------------------------------------------ 15. mixed.render_contexts
@gpu
def test_render_contexts_merges_the_sets(hip):
    from web_audio_api_rs_amd.mixed import bucket_report, render_contexts
    alone = [render(_single(hip, opt, i)) for i, opt in enumerate(range(N_SETS))]
    ctxs = [_single(hip, opt, i) for i, opt in enumerate(range(N_SETS))]
    assert bucket_report(ctxs) == [list(range(N_SETS))]
    merged = render_contexts(ctxs)
    for i in range(N_SETS):
        assert merged[i].data.shape == alone[i].shape == (1, 2, FRAMES)
        assert np.array_equal(merged[i].data, alone[i]), tg.OPTION_IDS[i]
        assert_heard(alone[i], f"context {i}")
    assert not np.array_equal(alone[0][:, :, :RQ], alone[5][:, :, :RQ])
