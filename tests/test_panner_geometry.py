"""Every branch of the equal-power PannerNode's geometry — the three distance models with their clamps, the cone's regions
and its shortcut, the early returns and both sign branches of the azimuth, the fold to [-90, 90], the mono and the stereo
gain law — through panner_geom_kernel (waa_panner.hip: the path taken when an AudioListener param is audio-rate), through
its host twin (waa_plan_ops.cpp: a single-valued listener) and through the oracle, against tests/panner_model.py, a numpy
model written from the reference's src/spatial.rs and src/node/panner.rs alone.

One context per row of a table of geometries (ROWS), the panner's and the listener's params set per context, so one small
render covers the whole table; the node's own options (OPTIONS: distance model with ref / max / rolloff, cone) are
parametrised.  Each table runs through two paths:
* "host": every listener param is single-valued (constants, and a k-rate block); panner params are k-rate blocks and one
  128-value block, of which the first value per quantum counts (panner.rs:833-846);
* "device": the listener's positionX (positionZ for the listener that faces +x) delivers 128 values in quanta 3 ... 8 only —
  per-frame geometry there, the once-per-quantum rule in quanta 0 ... 2 and 9 ... of the same kernel.  For the generic rows
  that block moves the listener past the source, so azimuth, distance and cone angle change every frame; the degenerate
  rows get a block that holds the listener still, so that every frame takes the early return the row is about.
All fifteen params take value blocks, so the three legs are handed the same f32 per-frame values.

Bounds (those of test_audio_rate_listener_automation): per (context, channel) RMS <= 1e-6 and max |diff| <= 5e-6, for
device against model(float32), device against oracle and oracle against model(float32).  Input cap, checked on the CPU:
acosf near +-1 turns one ulp of its argument into 3e-4 rad, so generic rows keep away from those points and the degenerate
rows sit exactly on them (axis-aligned, so that the f32 and the f64 model take the same early return); for every row and
frame 2 * |model(float32) - model(float64)| <= 5e-6 — the rule of test_compressor.py, max(2 * E_ref, floor), with inputs for
which the floor applies.

Not covered, because the reference itself yields non-finite gains: `linear` with ref_distance == max_distance (0 / 0) and
`exponential` with ref_distance == 0.  The HRTF panning model has tests of its own (test_hrtf.py).

WAA_WRITE_PROFILES=1 makes the GPU session write the measured fractions of the bounds into the "panner" section of
profiles/param_kernels_parity.json."""
import itertools
import json
import os

import numpy as np
import pytest

import panner_model as pm
import web_audio_api_rs_amd as waa
from graphs import assert_all_finite, assert_le, rms_err, white_noise

RQ = 128
TOL = 1e-6
MAX_TOL = 5e-6
SR = 48000.0
FRAMES = 12 * RQ + 5
NQ = (FRAMES + RQ - 1) // RQ
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A_RATE_QUANTA = (3, 9)  # the listener's 128-value block of the device path covers quanta 3 ... 8
_FIGURES = {}

CONES = [(360.0, 360.0, 0.3), (60.0, 200.0, 0.3), (-60.0, -200.0, 0.3), (200.0, 60.0, 0.3)]  # none; two cones; negative angles; inner > outer
DISTANCES = [  # (model, ref, max, rolloff); the rows' distances run from 0 over 0.5, 1.2, 3 to 13
    ("linear", 1.0, 10.0, 1.0), ("linear", 2.0, 6.0, 0.5), ("linear", 1.0, 5.0, 1.7), ("linear", 8.0, 2.0, 1.0), ("linear", 1.5, 9.0, 0.0),
    ("inverse", 1.0, 10000.0, 1.0), ("inverse", 2.5, 10000.0, 0.5), ("inverse", 1.0, 10000.0, 1.7), ("inverse", 0.7, 10000.0, 0.0),
    ("exponential", 1.0, 10000.0, 1.0), ("exponential", 2.5, 10000.0, 0.5), ("exponential", 1.0, 10000.0, 1.7),
    ("exponential", 0.7, 10000.0, 0.0)]
OPTIONS = [dict(distance_model=d[0], ref_distance=d[1], max_distance=d[2], rolloff_factor=d[3], cone_inner_angle=c[0],
                cone_outer_angle=c[1], cone_outer_gain=c[2]) for d, c in zip(DISTANCES, itertools.cycle(CONES))]
OPTION_IDS = [f"{o['distance_model']}-ref{o['ref_distance']:g}-max{o['max_distance']:g}-roll{o['rolloff_factor']:g}-"
              f"cone{o['cone_inner_angle']:g}_{o['cone_outer_angle']:g}" for o in OPTIONS]


def _rows():
    """the table of geometries: name, source position / orientation, listener position / forward / up; `still`: the row is
    about an exact configuration, so nothing moves in it; `along`: the listener param the device path moves (positionX, or
    positionZ)"""
    rows = []

    def add(name, sp, so=(1.0, 0.0, 0.0), lp=(0.0, 0.0, 0.0), lf=(0.0, 0.0, -1.0), lu=(0.0, 1.0, 0.0), still=False, along=6):
        rows.append(dict(name=name, v=[float(t) for t in (*sp, *so, *lp, *lf, *lu)], still=still, along=along))

    scales = [0.2, 0.45, 0.8, 1.2, 1.9, 2.7, 4.2, 5.0]  # |(1.3, 0.8, 2.1)| = 2.6: distances 0.5 ... 13
    for k, (sx, sy, sz) in enumerate(itertools.product((1.0, -1.0), repeat=3)):
        s = scales[k]
        add(f"octant {sx:+.0f}{sy:+.0f}{sz:+.0f}", (1.3 * sx * s, 0.8 * sy * s, 2.1 * sz * s), so=(0.3 * sz, -0.2 * sx, 1.0 * sy),
            lp=(0.1, -0.2, 0.3) if k % 2 else (0.0, 0.0, 0.0))
    add("straight ahead", (0.0, 0.0, -3.0), still=True)
    add("directly behind", (0.0, 0.0, 4.0), still=True)
    add("exactly left", (-2.0, 0.0, 0.0), still=True)
    add("exactly right", (2.0, 0.0, 0.0), still=True)
    add("straight above", (0.0, 3.0, 0.0), still=True)  # the projected source is exactly zero
    add("straight below", (0.0, -0.5, 0.0), still=True)
    add("at the listener", (0.5, 0.25, -1.0), lp=(0.5, 0.25, -1.0), still=True)
    add("forward parallel to up", (1.0, 0.5, -2.0), so=(-0.4, 0.1, 1.0), lu=(0.0, 0.0, -2.0))
    add("non-unit forward, non-orthogonal up", (1.5, -0.7, -2.2), so=(0.2, 1.0, 0.4), lf=(0.5, 0.2, -2.0), lu=(0.3, 1.5, -0.4))
    # (a listener that moves ALONG its forward axis has the source exactly at its side as it passes — acos(+-1): these move along z)
    add("listener turned, behind right", (-2.0, 0.5, 1.5), so=(0.0, 0.0, 0.0), lf=(1.0, 0.0, 0.0), along=8)  # 450 - az
    add("listener turned, ahead right", (2.0, 0.3, 1.0), so=(-1.0, 0.2, 0.1), lf=(1.0, 0.0, 0.0), along=8)
    add("listener turned, behind left", (-1.5, -0.4, -2.0), so=(1.0, 1.0, 1.0), lf=(1.0, 0.0, 0.0), along=8)
    # the cone, from a source straight ahead; the angle is measured against (source - listener), spatial.rs:289-297
    add("no orientation", (0.0, 0.0, -3.0), so=(0.0, 0.0, 0.0), still=True)
    add("orientation on the axis", (0.0, 0.0, -3.0), so=(0.0, 0.0, -2.0), still=True)
    for deg in (20.0, 60.0, 150.0):  # inside the inner cone (30), between the cones, beyond the outer one (100)
        add(f"orientation at {deg:g} degrees", (0.0, 0.0, -3.0), still=True,
            so=(1.5 * np.sin(np.radians(deg)), 0.0, -1.5 * np.cos(np.radians(deg))))
    return rows


ROWS = _rows()


def row_params(row, path):
    """the fifteen params of one row as panner_model.per_frame takes them"""
    p = list(row["v"])
    if row["still"]:
        if path == "device":
            p[6] = (p[6], A_RATE_QUANTA[0], np.full((A_RATE_QUANTA[1] - A_RATE_QUANTA[0], RQ), p[6], np.float32))
        return p
    q = np.arange(NQ, dtype=np.float64)
    p[0] = (p[0], 0, (p[0] + 0.05 * q).astype(np.float32))                                       # panner positionX: k-rate
    p[4] = (p[4], 1, (p[4] + 0.1 * q[1:NQ - 1]).astype(np.float32))                              # panner orientationY: k-rate, quanta 1 ... NQ - 2
    p[2] = (p[2], 0, (p[2] + np.linspace(0.0, 0.3, NQ * RQ)).astype(np.float32).reshape(NQ, RQ))  # panner positionZ: 128 values
    if path == "host":
        p[7] = (p[7], 2, (p[7] + 0.02 * q[2:]).astype(np.float32))                               # listener positionY: k-rate
    else:
        n = (A_RATE_QUANTA[1] - A_RATE_QUANTA[0]) * RQ
        k = row["along"]
        p[k] = (p[k], A_RATE_QUANTA[0], (p[k] + np.linspace(-4.0, 4.0, n)).astype(np.float32).reshape(-1, RQ))  # past the source
    return p


_NOISE = {}


def noise(nch):
    if nch not in _NOISE:
        _NOISE[nch] = white_noise(len(ROWS), nch, FRAMES, seed0=0x9A77E4)
        _NOISE[nch].setflags(write=False)
    return _NOISE[nch]


_MODEL = {}


def model(opt, nch, path, dtype):
    """[rows, 2, FRAMES] of the model in `dtype`, once per (option set, channels, path, dtype)"""
    key = (opt, nch, path, dtype)
    if key not in _MODEL:
        out = np.empty((len(ROWS), 2, FRAMES), dtype)
        for i, row in enumerate(ROWS):
            cols = [pm.per_frame(v, NQ) for v in row_params(row, path)]
            a_rate = np.any([wide for _, wide in cols[6:]], axis=0)
            out[i] = pm.render(noise(nch)[i], np.stack([v for v, _ in cols]), a_rate, dtype, **OPTIONS[opt])
        assert_all_finite(out, f"model {key}")
        out.setflags(write=False)
        _MODEL[key] = out
    return _MODEL[key]


def render(be, opt, nch, path):
    """source -> PannerNode -> destination, one context per row; (output, plan description or None)"""
    x = noise(nch)
    ctx = waa.OfflineAudioContext(2, FRAMES, SR, n_instances=len(ROWS), binding=be)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(x, SR)
    pn = ctx.create_panner(panning_model="equalpower", **OPTIONS[opt])
    handles = pn.params + ctx.listener().params
    for i, row in enumerate(ROWS):
        for prm, v in zip(handles, row_params(row, path)):
            prm.set_value(v if np.isscalar(v) else v[0], instance=i)
            if not np.isscalar(v):
                prm.set_block(v[1], v[2], instance=i)
    src.connect(pn).connect(ctx.destination())
    src.start()
    plan = ctx.plan_describe() if be.prefix == "waa_" else None
    out = ctx.start_rendering_sync().data
    ctx.close()
    return out, plan


_ORACLE = {}


def oracle(orc, opt, nch, path):
    key = (opt, nch, path)
    if key not in _ORACLE:
        out = render(orc, opt, nch, path)[0]
        out.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def check(name, got, want, figures=None):
    """(worst RMS / TOL, worst max |diff| / MAX_TOL), the worst row named"""
    assert got.shape == want.shape == (len(ROWS), 2, FRAMES), (got.shape, want.shape)
    assert_all_finite(got, name)
    d = np.abs(got.astype(np.float64) - want).max(axis=(1, 2))
    r, m = float(rms_err(got, want).max()) / TOL, float(d.max()) / MAX_TOL
    print(f"{name}: RMS {r:.3e} of its bound, max |diff| {m:.3e} of its bound (row '{ROWS[int(d.argmax())]['name']}')")
    if figures is not None:
        figures[name.split(": ")[1]] = dict(rms=r, max_abs=m)
    return r, m


def e_ref(opt, nch, path):
    """2 * max |model(float32) - model(float64)| per row, as fractions of MAX_TOL"""
    d = np.abs(model(opt, nch, path, np.float32).astype(np.float64) - model(opt, nch, path, np.float64)).max(axis=(1, 2))
    return 2.0 * d / MAX_TOL


ALL = [(o, nch, path) for o in range(len(OPTIONS)) for nch in (1, 2) for path in ("host", "device")]
ALL_IDS = [f"{OPTION_IDS[o]}-{nch}ch-{path}" for o, nch, path in ALL]


@pytest.fixture(scope="module", autouse=True)
def _write_parity_profile():
    yield
    if os.environ.get("WAA_WRITE_PROFILES") and _FIGURES:
        path = os.path.join(ROOT, "profiles", "param_kernels_parity.json")
        doc = {}
        if os.path.exists(path):
            with open(path) as f:
                doc = json.load(f)
        worst = {k: max(v[leg][k] for v in _FIGURES.values() for leg in v) for k in ("rms", "max_abs")}
        doc["panner"] = {
            "rule": "per (context, channel): RMS <= 1e-6 and max |diff| <= 5e-6; the figures are fractions of those bounds.  e_ref: "
                    "2 * max |model(float32) - model(float64)| over the rows and frames of the case, as a fraction of 5e-6 (asserted <= 1)",
            "worst_fraction_of_bound": worst, "cases": _FIGURES,
            "e_ref": {i: float(e_ref(*k).max()) for i, k in zip(ALL_IDS, ALL)}}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


# ---- CPU --------------------------------------------------------------------------------------------------------------------
def test_table_reaches_the_branches_it_names():
    """on the model's own intermediate values: every early return, both sign branches, the fold from both sides, both halves
    of the stereo law, the three cone regions, and distances below ref, between ref and max, and beyond max"""
    c = np.float32
    v = np.array([r["v"] for r in ROWS], np.float32).T
    sp, so, lp, lf, lu = (list(v[3 * k:3 * k + 3]) for k in range(5))
    az = pm.azimuth(sp, lp, lf, lu, c)
    by_name = {r["name"]: i for i, r in enumerate(ROWS)}
    for name in ("straight above", "straight below", "at the listener", "forward parallel to up", "straight ahead"):
        assert az[by_name[name]] == 0.0, name
    assert az[by_name["exactly left"]] == -90.0 and az[by_name["exactly right"]] == 90.0
    assert abs(abs(az[by_name["directly behind"]]) - 180.0) < 1e-3
    assert az[by_name["listener turned, behind right"]] > 90.0  # reached through 450 - az
    folded = pm.wrapped(az, c)
    assert (az < -90.0).sum() >= 2 and (az > 90.0).sum() >= 2 and (folded <= 0.0).sum() >= 4 and (folded > 0.0).sum() >= 4
    assert np.abs(folded).max() <= 90.0
    a = pm.angle(sp, so, lp, c)
    assert a[by_name["no orientation"]] == 0.0 and a[by_name["orientation on the axis"]] == 0.0
    assert (a < 30.0).sum() >= 3 and ((a >= 30.0) & (a < 100.0)).sum() >= 3 and (a >= 100.0).sum() >= 3
    dist = np.sqrt(np.sum((v[0:3] - v[6:9]) ** 2, axis=0))
    assert (dist == 0.0).sum() == 1 and ((dist > 0.0) & (dist < 0.7)).sum() >= 2 and ((dist > 2.5) & (dist < 5.0)).sum() >= 2
    assert (dist > 10.0).sum() >= 2
    for o in OPTIONS:  # the parameter sets for which the reference itself yields non-finite gains stay out
        assert o["ref_distance"] != o["max_distance"] and o["ref_distance"] > 0.0


@pytest.mark.parametrize("opt,nch,path", ALL, ids=ALL_IDS)
def test_input_cap(opt, nch, path):
    """no row or frame whose f32 arithmetic strays from the mathematics by more than half the max-|diff| bound"""
    e = e_ref(opt, nch, path)
    k = int(e.argmax())
    print(f"2 * E_ref = {e[k]:.3e} of the max-|diff| bound, in row '{ROWS[k]['name']}'")
    for i, row in enumerate(ROWS):
        assert_le(e[i], 1.0, f"row '{row['name']}': 2 * |model(f32) - model(f64)| as a fraction of 5e-6")


@pytest.mark.parametrize("opt,nch,path", ALL, ids=ALL_IDS)
def test_oracle_against_model(orc, opt, nch, path):
    want = model(opt, nch, path, np.float32)
    r, m = check("oracle vs model", oracle(orc, opt, nch, path), want)
    assert float(np.abs(want).max()) > 1e-3
    assert_le(r, 1.0, "RMS, fraction of 1e-6")
    assert_le(m, 1.0, "max |diff|, fraction of 5e-6")


# ---- GPU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("opt,nch,path", ALL, ids=ALL_IDS)
def test_device_against_model_and_oracle(hip, orc, opt, nch, path):
    got, plan = render(hip, opt, nch, path)
    assert ("audio-rate AudioListener automation" in plan) == (path == "device"), plan
    case = ALL_IDS[ALL.index((opt, nch, path))]
    figures = _FIGURES.setdefault(case, {})
    results = [check(f"{case}: device vs model", got, model(opt, nch, path, np.float32), figures),
               check(f"{case}: device vs oracle", got, oracle(orc, opt, nch, path), figures)]
    for r, m in results:  # (after both legs' figures have been printed)
        assert_le(r, 1.0, "RMS, fraction of 1e-6")
        assert_le(m, 1.0, "max |diff|, fraction of 5e-6")
