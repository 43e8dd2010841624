"""numpy model of the reference's equal-power PannerNode for tests/test_panner_geometry.py, written from src/spatial.rs:205-299
(azimuth_and_elevation, distance, angle) and src/node/panner.rs:716-779, 830-897, 927-1057 (the per-frame iterator of
spatial params, the single-valued-listener shortcut, cone_gain, dist_gain, the mono and the stereo gain law) — a third leg
next to the device's panner_geom_kernel, its host twin and the oracle's C restatement.

One `dtype` argument.  np.float32 mirrors the reference operation by operation: the vecmath algebra on f32 (square_len
= x*x + y*y + z*z, normalized = scale by 1 / sqrt(square_len), dot, cross), acos / cos / sin on f32, the distance gain in
f64 from the f32 distance and the node's f64 options, rounded to f32, the cone angles halved in f32.  np.float64 is the same
formulas in f64 throughout (nothing rounded to f32, the output included): what the mathematics gives for the same inputs.
The elevation is not modelled: the equal-power law does not read it.

Inputs are the values `AudioParamValues::get` hands the renderer, one per frame: 15 rows (the panner's position and
orientation, the listener's position, forward and up), and per quantum whether any of the nine listener slices has 128
values; where none has, the geometry of the quantum's first frame holds for all of it (panner.rs:833-846)."""
import numpy as np

RQ = 128
F32_MIN_POSITIVE = float(np.finfo(np.float32).tiny)
DISTANCE_MODELS = ("linear", "inverse", "exponential")


PARAMS = ("position_x", "position_y", "position_z", "orientation_x", "orientation_y", "orientation_z",  # the PannerNode's
          "position_x", "position_y", "position_z", "forward_x", "forward_y", "forward_z", "up_x", "up_y", "up_z")  # the listener's


def per_frame(param, n_quanta):
    """(one f32 value per frame [n_quanta * 128], [n_quanta] bool: a 128-value slice) of a param given as a constant or as
    (constant, quantum0, block) with a block of shape (nq,) or (nq, 128)"""
    v, wide = np.empty((n_quanta, RQ), np.float32), np.zeros(n_quanta, bool)
    if np.isscalar(param):
        v[:] = param
    else:
        const, q0, block = param
        block = np.asarray(block, np.float32)
        n = min(block.shape[0], n_quanta - q0)
        v[:] = const
        v[q0:q0 + n] = block[:n] if block.ndim == 2 else block[:n, None]
        wide[q0:q0 + n] = block.ndim == 2
    return v.reshape(-1), wide


def _sqlen(a):
    return a[0] * a[0] + a[1] * a[1] + a[2] * a[2]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _scale(a, s):
    return [a[0] * s, a[1] * s, a[2] * s]


def _normalized(a, one):
    return _scale(a, one / np.sqrt(_sqlen(a)))


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def azimuth(sp, lp, lf, lu, dtype):
    """spatial.rs:205-270 for arrays of vectors ([3][n] each): the azimuth in degrees, 0 on each of the three early returns"""
    c = dtype
    pi = c(np.pi)
    with np.errstate(all="ignore"):
        rel = _sub(sp, lp)
        at_listener = _sqlen(rel) <= c(F32_MIN_POSITIVE)
        sl = _normalized(rel, c(1))
        right = _cross(lf, lu)
        no_right = _sqlen(right) == 0
        rn, fn = _normalized(right, c(1)), _normalized(lf, c(1))
        up = _cross(rn, fn)
        ps = _sub(sl, _scale(up, _dot(sl, up)))
        no_projection = _sqlen(ps) == 0
        psn = _normalized(ps, c(1))
        az = c(180) * np.arccos(_dot(psn, rn)) / pi
        az = np.where(_dot(psn, fn) < 0, c(360) - az, az)
        az = np.where((az >= 0) & (az <= c(270)), c(90) - az, c(450) - az)
    return np.where(at_listener | no_right | no_projection, c(0), az).astype(dtype)


def angle(sp, so, lp, dtype):
    """spatial.rs:278-299: degrees between the source's orientation and (source - listener); 0 without an orientation and with
    the source at the listener"""
    c = dtype
    with np.errstate(all="ignore"):
        no_orientation = _sqlen(so) == 0
        son = _normalized(so, c(1))
        rel = _sub(sp, lp)
        at_listener = _sqlen(rel) <= c(F32_MIN_POSITIVE)
        a = np.abs(c(180) * np.arccos(_dot(_normalized(rel, c(1)), son)) / c(np.pi))
    return np.where(no_orientation | at_listener, c(0), a).astype(dtype)


def cone_gain(sp, so, lp, inner, outer, outer_gain, dtype):
    """panner.rs:927-953"""
    c = dtype
    abs_inner, abs_outer = c(abs(inner)) / c(2), c(abs(outer)) / c(2)
    if abs_inner >= 180 and abs_outer >= 180:
        return np.ones(np.shape(sp[0]), dtype)  # no cone specified
    g = c(outer_gain)
    a = angle(sp, so, lp, dtype)
    with np.errstate(all="ignore"):
        x = (a - abs_inner) / (abs_outer - abs_inner)
        between = (c(1) - x) + g * x
    return np.where(a < abs_inner, c(1), np.where(a >= abs_outer, g, between)).astype(dtype)


def dist_gain(sp, lp, model, ref, max_distance, rolloff, dtype):
    """panner.rs:955-985: f64 arithmetic on the distance computed in `dtype`; rounded to f32 by the f32 model only"""
    assert model in DISTANCE_MODELS, model
    distance = np.sqrt(_sqlen(_sub(sp, lp))).astype(np.float64)
    ref, max_distance, rolloff = float(ref), float(max_distance), float(rolloff)
    with np.errstate(all="ignore"):
        if model == "linear":
            r = min(max(rolloff, 0.0), 1.0)
            d2ref, d2max = min(ref, max_distance), max(ref, max_distance)
            g = 1.0 - r * (np.clip(distance, d2ref, d2max) - d2ref) / (d2max - d2ref)
        elif model == "inverse":
            r = max(rolloff, 0.0)
            g = np.where(distance > 0.0, ref / (ref + r * (np.maximum(ref, distance) - ref)), 1.0)
        else:
            r = max(rolloff, 0.0)
            g = np.power(np.maximum(distance, ref) / ref, -r)
    return g.astype(dtype)


def wrapped(az, dtype):
    """panner.rs:996-1004: clamp to [-180, 180], then fold to [-90, 90]"""
    c = dtype
    az = np.clip(az, c(-180), c(180))
    return np.where(az < c(-90), c(-180) - az, np.where(az > c(90), c(180) - az, az)).astype(dtype)


def render(x, params, listener_a_rate, dtype, distance_model="inverse", ref_distance=1.0, max_distance=10000.0, rolloff_factor=1.0,
           cone_inner_angle=360.0, cone_outer_angle=360.0, cone_outer_gain=0.0):
    """x [1 or 2, frames] f32 through one equal-power PannerNode -> [2, frames] in `dtype`.  params [15, n_quanta * 128] f32:
    one value per frame of position xyz, orientation xyz, listener position xyz, forward xyz, up xyz; listener_a_rate
    [n_quanta] bool: a listener slice of 128 values in that quantum"""
    c = dtype
    x = np.asarray(x, np.float32)
    nch, frames = x.shape
    params = np.asarray(params, np.float32)
    frame = np.arange(frames)
    first = frame // RQ * RQ
    use = np.where(np.asarray(listener_a_rate, bool)[frame // RQ], frame, first)  # single-valued listener: the quantum's first frame
    v = params[:, use].astype(dtype)
    sp, so, lp, lf, lu = (list(v[3 * k:3 * k + 3]) for k in range(5))
    dg = dist_gain(sp, lp, distance_model, ref_distance, max_distance, rolloff_factor, dtype)
    cg = cone_gain(sp, so, lp, cone_inner_angle, cone_outer_angle, cone_outer_gain, dtype)
    az = wrapped(azimuth(sp, lp, lf, lu, dtype), dtype)
    half_pi_of = lambda t: t * c(np.pi) / c(2)  # noqa: E731  (x * PI / 2.)
    xin = x.astype(dtype)
    out = np.empty((2, frames), dtype)
    if nch == 1:  # apply_mono_to_stereo_gain, panner.rs:988-1014 (the mono input up-mixed to both channels first)
        t = (az + c(90)) / c(180)
        gl, gr = np.cos(half_pi_of(t)), np.sin(half_pi_of(t))
        out[0] = xin[0] * (gl * dg * cg)
        out[1] = xin[0] * (gr * dg * cg)
    else:  # apply_stereo_to_stereo_gain, panner.rs:1016-1057
        assert nch == 2, nch
        left = az <= 0
        t = np.where(left, (az + c(90)) / c(90), az / c(90))
        gl, gr = np.cos(half_pi_of(t)), np.sin(half_pi_of(t))
        il, ir = xin
        out[0] = np.where(left, (il + ir * gl) * dg * cg, il * gl * dg * cg)
        out[1] = np.where(left, ir * gr * dg * cg, (ir + il * gr) * dg * cg)
    return out
