"""Integrated loudness (BS.1770) of the rendered output computed on the device (waa_output_loudness, waa_output_loudness_series,
waa_loudness_hop, waa_loudness_from_series of include/waa_hip_device.h), the Python mirror OfflineAudioContext.output_loudness /
output_loudness_series / loudness_from_series and download_pcm16(normalize_loudness=, max_peak=).

The reference is tests/loudness_model.py in np.longdouble, applied to what waa_download_all returned from the SAME batch.  The
device's sub-block energies are not bit-equal to a serial recurrence (the state hand-over between sub-blocks rounds differently):
they are held within the model's first-order bound (loudness_model.bound, derived there), which every test also shows to be at most
1e-7 of z wherever z is at least 1e-6 of its row's largest.  Loudness fields are compared under that bound carried through
10 log10; gate decisions are exact because every case asserts on the model that no block lies within 1e-5 LU of a threshold.

WAA_LOUDNESS_PARITY_OUT=<file>: the GPU tests append their observed |device - model| / bound ratios there (profiles/
loudness_parity.json is such a run)."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import web_audio_api_rs_amd as waa
import batch_graphs as G
import loudness_model as M
import pcm_model
import rearm
import test_launch_list as L

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-audio-api-rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = ("integrated", "momentary_max", "short_term_max", "relative_threshold")
# what enters as +0.0 (non-finite, both zeros' sign, a denormal)
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40], np.float32)
NEW = ("output_loudness", "output_loudness_series", "loudness_hop", "loudness_from_series")


def assert_bound_is_tight(z, bz, what):
    """the issue's condition on the derived bound: at most 1e-7 of z on every sub-block with z >= 1e-6 of its row's largest"""
    z = np.asarray(z, np.float64)
    if z.size == 0:
        return
    big = (z >= 1e-6 * z.max(axis=-1, keepdims=True)) & (z > 0)
    if big.any():
        worst = float((bz[big] / z[big]).max())
        assert worst <= 1e-7, f"{what}: the derived bound is {worst:.3g} of z"
    assert not bz[~(z != 0).any(axis=-1)].any(), f"{what}: a row of zeros has a bound of zero"


def assert_within_bound(got, z, bz, what):
    """|got - z| <= bz (z: longdouble); rows of zeros are exact zeros.  Returns the largest |got - z| / bz."""
    assert got.shape == z.shape and got.dtype == np.float64, (what, got.shape, z.shape)
    err = np.abs(got.astype(np.longdouble) - z).astype(np.float64)
    bad = err > bz
    if bad.any():
        k = tuple(int(v) for v in np.unravel_index(int(np.argmax(bad)), bad.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} sub-blocks outside the bound; the first at {k}: got {got[k]!r}, "
                             f"model {float(z[k])!r}, |difference| {err[k]:.3g}, bound {bz[k]:.3g}")
    zero_rows = ~(np.asarray(z, np.float64) != 0).any(axis=-1)
    assert not got[zero_rows].view(np.uint64).any(), f"{what}: a row of zeros gives +0.0"
    return float((err[bz > 0] / bz[bz > 0]).max()) if (bz > 0).any() else 0.0


def assert_stats(got, z, bz, h, what, weights=None):
    """one context's record against the model's gating of the longdouble z[n_ch, n_sub]"""
    want = M.gating(np.asarray(z, np.float64), h, weights)
    margin = M.gate_margin(want)
    assert margin > 1e-5, f"{what}: a block lies {margin:.3g} LU from a threshold: choose another seed"
    tol = M.lufs_bound(z, bz, h, weights)
    assert tol < 1e-6, (what, tol)
    assert (int(got["n_blocks"]), int(got["n_gated"])) == (want["n_blocks"], want["n_gated"]), (what, got, want)
    for f in FIELDS:
        a, b = float(got[f]), want[f]
        assert (a == b) if math.isinf(b) or math.isinf(a) else abs(a - b) <= tol, f"{what}: {f}: got {a!r}, model {b!r}, tolerance {tol:.3g}"
    return want


_RATIOS = {}


def record(what, ratio):
    _RATIOS[what] = ratio
    out = os.environ.get("WAA_LOUDNESS_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"device_to_bound": _RATIOS, "largest": max(_RATIOS.values())}, f, indent=1, sort_keys=True)


# ---- the model ------------------------------------------------------------------------------------------------------------------
def test_the_coefficients_are_the_tables_of_bs1770_at_48_khz():
    shelf, hp = M.coefficients(48000.0)
    want = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585)
    assert max(abs(a - b) for a, b in zip(shelf, want)) <= 1e-12
    assert hp[:3] == (1.0, -2.0, 1.0) and abs(hp[3] + 1.99004745483398) <= 1e-12 and abs(hp[4] - 0.99007225036621) <= 1e-12
    assert [M.hop(sr) for sr in (8000.0, 11025.0, 44100.0, 48000.0)] == [800, 1103, 4410, 4800]


def _scalar_series(x, sr):
    """the definitions restated frame by frame in plain Python floats"""
    (b0, b1, b2, a1, a2), (d0, d1, d2, c1, c2) = M.coefficients(sr)
    h = M.hop(sr)
    p1 = p2 = q1 = q2 = 0.0
    z = []
    for j in range(len(x) // h):
        acc = 0.0
        for f in range(j * h, (j + 1) * h):
            a = int(np.float32(x[f]).view(np.uint32)) & 0x7FFFFFFF
            s = float(x[f]) if 1 <= (a >> 23) <= 254 else 0.0
            v = b0 * s + p1
            p1 = (b1 * s - a1 * v) + p2
            p2 = b2 * s - a2 * v
            w = d0 * v + q1
            q1 = (d1 * v - c1 * w) + q2
            q2 = d2 * v - c2 * w
            acc = acc + w * w
        z.append(acc)
    return z


def test_the_model_equals_a_scalar_restatement():
    sr, h = 8000.0, 800
    frames = 2 * h + 7
    x = np.random.default_rng(8).uniform(-1.2, 1.2, frames).astype(np.float32)
    x[[0, h - 1, h, 2 * h - 1, 2 * h]] = SPECIALS
    x[2 * h + 1:] = 1e30  # (behind the last whole sub-block: not read)
    got = M.series(x, sr)
    assert got.shape == (2,) and [float(v).hex() for v in got] == [v.hex() for v in _scalar_series(x, sr)]
    both = M.series(np.stack([x, x[::-1]]).reshape(1, 2, frames), sr)
    assert both.shape == (1, 2, 2) and both[0, 0].tobytes() == got.tobytes()
    assert M.series(x[:h - 1], sr).shape == (0,)


def noise(n, ch, frames, seed, sr):
    """white noise in +-1.2, every context at a level of its own, the special values planted at the first and the last frame and on
    both sides of every sub-block edge, in another rotation for every row"""
    rng = np.random.default_rng([n, ch, frames, seed])
    x = (rng.uniform(-1.2, 1.2, (n, ch, frames)) * rng.uniform(0.05, 1.0, (n, 1, 1))).astype(np.float32)
    h = M.hop(sr)
    at = sorted({f for e in range(0, frames + h, h) for f in (e - 1, e) if 0 <= f < frames} | {0, frames - 1})
    for i in range(n):
        for c in range(ch):
            for k, f in enumerate(at):
                x[i, c, f] = SPECIALS[(k + i * ch + c) % SPECIALS.size]
    return x


CPU_CASES = [(48000.0, 7 * 4800 + 13), (44100.0, 4 * 4410 + 1), (11025.0, 31 * 1103), (8000.0, 12 * 800 + 5)]


@pytest.mark.parametrize("sr,frames", CPU_CASES)
def test_f64_is_within_the_bound_of_longdouble(sr, frames):
    x = noise(2, 2, frames, 1, sr)
    x[1, 0, frames // 2:] *= np.float32(0.01)   # a quiet section behind a loud one
    x[1, 1, frames // 3:] = 0.0                 # silence behind a loud section: the filters ring out
    z, bz = M.bound(x, sr)
    assert_bound_is_tight(z, bz, f"{sr}")
    ratio = assert_within_bound(M.series(x, sr), z, bz, f"{sr}")
    assert ratio > 0
    zeros = np.zeros((1, frames), np.float32)
    zz, zb = M.bound(zeros, sr)
    assert not np.asarray(zz, np.float64).any() and not zb.any()


def _sine(sr, seconds, hz, amp, ch=1):
    t = np.arange(int(sr * seconds)) / sr
    return np.repeat((amp * np.sin(2 * np.pi * hz * t)).astype(np.float32)[None, :], ch, axis=0)


def _model_loudness(x, sr, weights=None):
    z, bz = M.bound(x, sr)
    r = M.gating(np.asarray(z, np.float64), M.hop(sr), weights)
    assert M.gate_margin(r) > 1e-5
    return r, M.lufs_bound(z, bz, M.hop(sr), weights)


def _gated(z, h):
    r = M.gating(z, h)
    assert M.gate_margin(r) > 1e-5
    return r


def test_known_answers():
    r = _gated(M.series(_sine(48000.0, 3, 997.0, 1.0), 48000.0), 4800)
    assert abs(r["integrated"] + 3.01) <= 0.01 and r["n_blocks"] == 27 == r["n_gated"]
    # the rest at 8 kHz, one run of the model: a 1 kHz sine at -23 dBFS (3 s, then silence), 3 s at 0.5 and 3 s 20 dB down
    sr, h = 8000.0, 800
    silence = np.zeros((1, 3 * 8000), np.float32)
    a = 10 ** (-23 / 20)
    z = M.series(np.concatenate([np.concatenate([_sine(sr, 3, 1000.0, a), silence], axis=1),
                                 np.concatenate([_sine(sr, 3, 1000.0, 0.5), _sine(sr, 3, 1000.0, 0.05)], axis=1)]), sr)
    stereo = _gated(z[[0, 0], :30], h)   # (both channels the same row)
    assert abs(stereo["integrated"] + 23.0) <= 0.1 and stereo["n_gated"] == 27
    # 2 s of digital silence behind an abrupt end: the three blocks that straddle the end hold 3/4, 1/2, 1/4 of a block's energy
    # (-1.2, -3, -6 LU: above the relative gate) and stay in the mean — 10 log10(28.5 / 30) = -0.22 LU, BS.1770's own behaviour
    padded = _gated(z[[0, 0], :50], h)
    assert padded["n_blocks"] == 47 and padded["n_gated"] == 30
    assert abs(padded["integrated"] - stereo["integrated"] - 10 * math.log10(28.5 / 30)) <= 0.01
    # a section 20 LU down is gated out by the relative gate; the three blocks that straddle the step stay in
    step, alone = _gated(z[1:], h), _gated(z[1:, :30], h)
    assert step["n_blocks"] == 57 and step["n_gated"] == 30 and alone["n_gated"] == 27
    assert abs(step["integrated"] - alone["integrated"] - 10 * math.log10((27 + 0.7525 + 0.505 + 0.2575) / 30)) <= 0.01


def test_appended_silence_changes_nothing_beyond_the_bound():
    """2 s of digital silence appended to a clip whose own last 400 ms are silent already (behind an abrupt end the straddling
    blocks change the mean: test_known_answers): more blocks, the same gated set, the same loudness within the bound"""
    sr, h = 8000.0, 800
    x = noise(1, 1, 20 * h, 3, sr)[0]
    x[:, 16 * h:] = 0.0
    with_silence, tol = _model_loudness(x, sr)
    z, _ = M.bound(x, sr)
    z = np.asarray(z, np.float64)
    assert z[0, 17] < 1e-9 * z[0, 15]
    # digital silence appended to a clip that ended anyway: longer, and the same loudness within the bound
    longer = np.concatenate([x, np.zeros((1, 20 * h), np.float32)], axis=1)
    r, tol2 = _model_loudness(longer, sr)
    assert r["n_blocks"] == with_silence["n_blocks"] + 20 and r["n_gated"] == with_silence["n_gated"]
    assert abs(r["integrated"] - with_silence["integrated"]) <= tol + tol2


# ---- waa_loudness_from_series against the model's gating -------------------------------------------------------------------------
def _synthetic(n_ch, n_sub, seed, h=800):
    rng = np.random.default_rng([n_ch, n_sub, seed])
    return rng.uniform(0.2, 1.0, (n_ch, n_sub)) * h * 10.0 ** rng.integers(-3, 0, (1, n_sub))


def _assert_record(got, want, what, tol=1e-11):
    assert (int(got["n_blocks"]), int(got["n_gated"])) == (want["n_blocks"], want["n_gated"]), (what, got, want)
    for f in FIELDS:
        a, b = float(got[f]), want[f]
        assert (a == b) if math.isinf(b) or math.isinf(a) else abs(a - b) <= tol, f"{what}: {f}: got {a!r}, model {b!r}"


@pytest.mark.parametrize("n_sub", [0, 3, 4, 5, 29, 30, 31])
@pytest.mark.parametrize("n_ch", [1, 2, 4, 6])
def test_from_series_equals_the_models_gating(hip, n_sub, n_ch):
    z = _synthetic(n_ch, n_sub, 0)
    want = M.gating(z, 800)
    assert M.gate_margin(want) > 1e-5
    got = waa.loudness_from_series(z, 800, binding=hip)
    _assert_record(got, want, f"{n_ch} x {n_sub}")
    assert int(got["n_blocks"]) == max(n_sub - 3, 0) and (float(got["short_term_max"]) > -math.inf) == (n_sub >= 30)
    if n_sub >= 4:
        assert 0 < int(got["n_gated"]) and float(got["integrated"]) > -70.0
    if n_sub >= 5 and n_ch == 2:
        w = [0.25, 3.0]
        _assert_record(waa.loudness_from_series(z, 800, weights=w, binding=hip), M.gating(z, 800, w), "caller weights")
        assert float(waa.loudness_from_series(z, 800, weights=w, binding=hip)["integrated"]) != float(got["integrated"])


def test_from_series_layouts_and_silence(hip):
    z = _synthetic(6, 12, 1)
    got = waa.loudness_from_series(z, 800, binding=hip)
    _assert_record(got, M.gating(z, 800, [1, 1, 1, 0, 1.41, 1.41]), "5.1")
    lfe = z.copy()
    lfe[3] *= 100.0   # the LFE has weight 0
    assert waa.loudness_from_series(lfe, 800, binding=hip).tobytes() == got.tobytes()
    q = _synthetic(4, 12, 2)
    _assert_record(waa.loudness_from_series(q, 800, binding=hip), M.gating(q, 800, [1, 1, 1.41, 1.41]), "quad")
    assert M.default_weights(6) == [1, 1, 1, 0, 1.41, 1.41] and M.default_weights(4) == [1, 1, 1.41, 1.41] and M.default_weights(3) == [1, 1, 1]
    # a section 30 LU down falls to the relative gate
    step = np.concatenate([_synthetic(2, 12, 6), _synthetic(2, 12, 7) * 1e-3], axis=1)
    got = waa.loudness_from_series(step, 800, binding=hip)
    _assert_record(got, M.gating(step, 800), "a quiet half")
    assert M.gate_margin(M.gating(step, 800)) > 1e-5 and 9 <= int(got["n_gated"]) <= 12 and int(got["n_blocks"]) == 21
    # one channel of zeros
    one = _synthetic(2, 12, 3)
    one[1] = 0.0
    _assert_record(waa.loudness_from_series(one, 800, binding=hip), M.gating(one[:1], 800), "a channel of zeros")
    # all blocks below -70 LUFS, and nothing at all
    low = _synthetic(2, 35, 4) * 1e-8
    got = waa.loudness_from_series(low, 800, binding=hip)
    want = M.gating(low, 800)
    assert -120 < want["momentary_max"] < -70 and M.gate_margin(want) > 1e-5
    _assert_record(got, want, "below the absolute gate")
    assert float(got["integrated"]) == -math.inf == float(got["relative_threshold"]) and int(got["n_gated"]) == 0 and int(got["n_blocks"]) == 32
    assert -120 < float(got["short_term_max"]) < -70
    got = waa.loudness_from_series(np.zeros((2, 35)), 800, binding=hip)
    assert all(float(got[f]) == -math.inf for f in FIELDS) and int(got["n_blocks"]) == 32 and int(got["n_gated"]) == 0


def test_from_series_refusals(hip):
    z = _synthetic(2, 8, 5)
    out = waa.api.LoudnessStats()
    zp = z.ctypes.data_as(waa.api._DP)
    assert hip.loudness_from_series(None, 2, 8, 800, None, C.byref(out)) == 1 and "null series / destination" in hip.last_error().decode()
    assert hip.loudness_from_series(zp, 2, 8, 800, None, None) == 1 and "null series / destination" in hip.last_error().decode()
    assert hip.loudness_from_series(zp, 2, 8, 0, None, C.byref(out)) == 1 and "no frames" in hip.last_error().decode()
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(waa.WaaError, match="weight of channel 1") as e:
            waa.loudness_from_series(z, 800, weights=[1.0, bad], binding=hip)
        assert e.value.status == 1
    with pytest.raises(ValueError):
        waa.loudness_from_series(z, 800, weights=[1.0], binding=hip)
    assert hip.loudness_from_series(None, 0, 0, 800, None, C.byref(out)) == 0 and out.integrated == -math.inf and out.n_blocks == 0


# ---- the C ABI and its mirror, without a device -------------------------------------------------------------------------------------
def test_the_header_declares_the_library_exports_and_api_binds(hip):
    header = open(os.path.join(ROOT, "include", "waa_hip_device.h")).read()
    for name in NEW:
        assert re.search(r"(waa_status|uint32_t) waa_%s\(" % name, header), name
        assert name in waa.api.ABI_DEVICE and callable(getattr(hip, name))
        assert getattr(hip.lib, "waa_" + name) is not None
    m = re.search(r"typedef struct waa_loudness_stats \{(.*?)\} waa_loudness_stats;", header, re.S)
    fields = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split()
    assert " ".join(fields) == "double integrated, momentary_max, short_term_max, relative_threshold; uint32_t n_blocks, n_gated;"
    assert C.sizeof(waa.api.LoudnessStats) == 40 and waa.api.LOUDNESS_STATS_DTYPE.itemsize == 40
    for name, _ in waa.api.LoudnessStats._fields_:
        assert getattr(waa.api.LoudnessStats, name).offset == waa.api.LOUDNESS_STATS_DTYPE.fields[name][1], name
    assert [hip.loudness_hop(sr) for sr in (8000.0, 11025.0, 44100.0, 48000.0)] == [800, 1103, 4410, 4800]


def _plan_only(hip, n=2, ch=2, frames=300, sr=48000.0):
    ctx = waa.OfflineAudioContext(ch, frames, sr, n_instances=n, binding=hip, device=waa.PLAN_ONLY)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(np.zeros((n, ch, frames), np.float32), sr)
    src.connect(ctx.destination())
    src.start()
    return ctx.prepare()


def test_refusals_without_a_device(hip):
    ctx = _plan_only(hip)
    h = ctx._handle
    stats = (waa.api.LoudnessStats * 2)()
    z = np.zeros(16)
    zp = z.ctypes.data_as(waa.api._DP)
    for call in (lambda: hip.output_loudness(None, None, stats), lambda: hip.output_loudness(h, None, None),
                 lambda: hip.output_loudness_series(None, zp), lambda: hip.output_loudness_series(h, None)):
        assert call() == 1 and "null batch / destination" in hip.last_error().decode()
    bad = np.array([1.0, -1.0]).ctypes.data_as(waa.api._DP)
    for call in (lambda: hip.output_loudness(h, None, stats), lambda: hip.output_loudness(h, bad, stats), lambda: hip.output_loudness_series(h, zp)):
        assert call() == 5 and hip.last_error().decode() == "plan-only batch has no device"   # (in front of the weights' check)
    for call in (ctx.output_loudness, ctx.output_loudness_series, lambda: ctx.download_pcm16(normalize_loudness=-23.0)):
        with pytest.raises(waa.WaaError, match="nothing rendered yet") as e:
            call()
        assert e.value.status == 3
    gain = np.ones(2, np.float32)
    for kw in (dict(gain=gain, normalize_loudness=-23.0), dict(normalize_peak=0.5, normalize_loudness=-23.0), dict(max_peak=0.5),
               dict(max_peak=0.5, gain=gain), dict(max_peak=0.5, normalize_peak=0.5)):
        with pytest.raises(ValueError):
            ctx.download_pcm16(**kw)
    with pytest.raises(ValueError, match="not both"):   # the message of before
        ctx.download_pcm16(gain=gain, normalize_peak=0.5)
    ctx.close()


def test_another_binding_is_out_of_scope(orc):
    ctx = waa.OfflineAudioContext(1, 256, 48000.0, n_instances=2, binding=orc)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(np.zeros((2, 1, 256), np.float32), 48000.0)
    src.connect(ctx.destination())
    src.start()
    ctx.start_rendering_sync()
    for call in (ctx.output_loudness, ctx.output_loudness_series, lambda: ctx.download_pcm16(normalize_loudness=-23.0),
                 lambda: waa.loudness_from_series(np.ones((1, 8)), 800, binding=orc)):
        with pytest.raises(waa.WaaError, match="feature of the device library") as e:
            call()
        assert e.value.status == 4
    ctx.close()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_loudness_code_object(tmp_path):
    """waa_loudness.hip compiled to ISA with the library's flags, only the metadata read: three kernels, nothing spilled, no scratch,
    no LDS; the two streaming kernels within 128 vector registers (four wavefronts per SIMD)"""
    out = str(tmp_path / "waa_loudness.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fgpu-flush-denormals-to-zero",
                           "--cuda-device-only", "-S", os.path.join(CSRC, "waa_loudness.hip"), "-o", out], stderr=subprocess.DEVNULL)
    res = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)(.*?)\.wavefront_size", open(out).read(), re.S):
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(2)).group(1))  # noqa: E731
        res[re.search(r"\.name:\s+(\S+)", m.group(2)).group(1)] = {
            "vgpr": get("vgpr_count"), "spill": get("vgpr_spill_count"), "sgpr_spill": get("sgpr_spill_count"),
            "scratch": get("private_segment_fixed_size"), "lds": int(m.group(1))}
    names = {k: next(n for n in res if k in n) for k in ("loudness_state_kernel", "loudness_chain_kernel", "loudness_energy_kernel")}
    assert len(res) == 3, sorted(res)
    for r in res.values():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0, res
    assert res[names["loudness_state_kernel"]]["vgpr"] <= 128 and res[names["loudness_energy_kernel"]]["vgpr"] <= 128, res


def test_the_plan_text_is_what_it_was(hip, monkeypatch):
    """nothing of this is a plan step: the plan text of a graph of tests/batch_graphs.py is word for word what tests/golden/
    launch_lists holds for it, names none of the new kernels, and is the same after (refused) calls of the new entry points"""
    cut = lambda t: t.partition("launch 0: ")[0]  # noqa: E731  (the product prints no launch list)
    golden = cut(L._sections(L._golden("named"))["fm_pair"])
    fm_pair = lambda be: G.build(G.b_fm_pair, be, [0, 1, 2], device=waa.PLAN_ONLY, frames=128 * 40)  # noqa: E731
    assert L.describe(hip, fm_pair, {}, monkeypatch.setenv, monkeypatch.delenv) == golden
    assert "loudness" not in golden
    ctx = fm_pair(hip)
    before = ctx.plan_describe()
    stats = (waa.api.LoudnessStats * 3)()
    assert hip.output_loudness(ctx._handle, None, stats) == 5
    assert hip.output_loudness_series(ctx._handle, np.zeros(64).ctypes.data_as(waa.api._DP)) == 5
    after = ctx.plan_describe()
    ctx.close()
    strip = lambda t: t.partition("\n")[0].split(" | timing:")[0] + "\n" + t.partition("\n")[2]  # noqa: E731
    assert strip(before) == strip(after) and "loudness" not in after


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
def passthrough(hip, audio, sr, n_out=None):
    """BufferSource -> destination, one AudioBuffer per context; prepared, not rendered"""
    n, ch, frames = audio.shape
    ctx = waa.OfflineAudioContext(n_out or ch, frames, sr, n_instances=n, binding=hip)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(audio, sr)
    src.connect(ctx.destination())
    src.start()
    return ctx


def assert_loudness(ctx, f32, sr, what, weights=None, rows=None):
    """output_loudness_series and output_loudness of the rendered context against the model of its f32 download.  rows: f32 holds
    these contexts only (a large batch of repeated contexts).  Returns (z of the device, the records)."""
    h = M.hop(sr)
    sel = np.arange(f32.shape[0]) if rows is None else np.asarray(rows)
    z, bz = M.bound(f32, sr)
    assert_bound_is_tight(z, bz, what)
    got_z = ctx.output_loudness_series()
    assert got_z.shape == (ctx.n_instances, f32.shape[1], f32.shape[2] // h)
    record(what, assert_within_bound(got_z[sel], z, bz, what))
    got = ctx.output_loudness(weights)
    assert got.shape == (ctx.n_instances,) and got.dtype == waa.api.LOUDNESS_STATS_DTYPE
    for k, i in enumerate(sel):
        assert_stats(got[i], z[k], bz[k], h, f"{what}: context {i}", weights)
    return got_z, got


def _h(sr):
    return M.hop(sr)


# (rate, frames, contexts, channels): every rate (h % 4 == 0, 2, odd, 800), every length around the first sub-block, the first
# block and the first short-term window, more than 64 sub-blocks per row, 1 / 3 / 67 contexts and 1 / 2 / 3 / 6 channels
GPU_CASES = [
    (48000.0, _h(48000.0) - 1, 1, 1), (48000.0, _h(48000.0), 3, 2), (48000.0, 4 * _h(48000.0) - 1, 1, 3), (48000.0, 4 * _h(48000.0), 3, 1),
    (48000.0, 4 * _h(48000.0) + 1, 67, 2), (48000.0, 7 * _h(48000.0) + 13, 3, 6),
    (44100.0, _h(44100.0) - 1, 3, 2), (44100.0, 4 * _h(44100.0) + 1, 3, 3), (44100.0, 7 * _h(44100.0) + 13, 1, 2),
    (11025.0, _h(11025.0), 1, 6), (11025.0, 4 * _h(11025.0) - 1, 3, 2), (11025.0, 4 * _h(11025.0) + 1, 67, 6), (11025.0, 7 * _h(11025.0) + 13, 1, 1),
    (11025.0, 31 * _h(11025.0), 3, 2),
    (8000.0, 800, 67, 1), (8000.0, 4 * 800, 1, 6), (8000.0, 7 * 800 + 13, 67, 3), (8000.0, 31 * 800, 1, 3), (8000.0, 70 * 800 + 5, 3, 2),
]


@gpu
@pytest.mark.parametrize("sr,frames,n,ch", GPU_CASES)
def test_loudness_equals_the_model(hip, sr, frames, n, ch):
    ctx = passthrough(hip, noise(n, ch, frames, 0, sr), sr)
    try:
        f32 = ctx.start_rendering_sync().data
        assert np.isnan(f32).any()   # the planted values arrived
        z, got = assert_loudness(ctx, f32, sr, f"{sr:.0f} Hz, {n} x {ch} x {frames}")
    finally:
        ctx.close()
    h = M.hop(sr)
    assert (got["n_blocks"] == max(frames // h - 3, 0)).all()
    if frames < h:
        assert z.shape[2] == 0 and all((got[f] == -np.inf).all() for f in FIELDS) and not got["n_gated"].any()
    if frames // h >= 4:
        assert (got["n_gated"] > 0).all() and np.isfinite(got["integrated"]).all()


@gpu
def test_caller_weights_and_a_quiet_section(hip):
    sr, h = 8000.0, 800
    audio = noise(3, 2, 40 * h, 7, sr)
    audio[:, :, 20 * h:] *= np.float32(0.03)   # 30 LU down: behind the relative gate
    ctx = passthrough(hip, audio, sr)
    try:
        f32 = ctx.start_rendering_sync().data
        _, plain = assert_loudness(ctx, f32, sr, "a quiet half")
        _, weighted = assert_loudness(ctx, f32, sr, "a quiet half, caller weights", weights=[0.5, 2.0])
        assert (plain["n_gated"] < plain["n_blocks"] - 10).all() and (plain["integrated"] != weighted["integrated"]).all()
        with pytest.raises(waa.WaaError, match="weight of channel 1") as e:
            ctx.output_loudness([1.0, -0.5])
        assert e.value.status == 1
    finally:
        ctx.close()


@gpu
def test_lanes_off_a_16_byte_boundary(hip):
    """a destination that aliases the source's signal (a pass-through copies nothing into a signal of the destination's own), h odd:
    the rows the planner lays out start on 16-byte boundaries, their sub-blocks — what a lane walks — at every 4-byte offset"""
    sr = 11025.0
    h = M.hop(sr)
    n, ch, frames = 5, 3, 4 * h + 1
    ctx = passthrough(hip, noise(n, ch, frames, 9, sr), sr)
    try:
        f32 = ctx.start_rendering_sync().data
        base, s_i, s_c = ctx.output_device()
        offsets = {(base + 4 * (i * s_i + c * s_c + j * h)) % 16 for i in range(n) for c in range(ch) for j in range(4)}
        assert offsets == {0, 4, 8, 12}
        assert_loudness(ctx, f32, sr, "lanes at every 4-byte offset")
    finally:
        ctx.close()


@gpu
def test_a_channel_the_destination_does_not_carry(hip):
    sr = 44100.0
    frames = 5 * M.hop(sr) + 2
    ctx = passthrough(hip, noise(3, 1, frames, 11, sr), sr, n_out=2)
    ctx.destination().set_channel_count(1)
    try:
        f32 = ctx.start_rendering_sync().data
        assert not f32[:, 1].view(np.uint32).any() and f32[:, 0].view(np.uint32).any()
        z, _ = assert_loudness(ctx, f32, sr, "one of two channels carried")
        assert not z[:, 1].view(np.uint64).any() and z[:, 0].all()
    finally:
        ctx.close()


@gpu
def test_loudness_of_a_render_with_state(hip):
    """BufferSource -> Biquad -> Gain, the smoke graph: the destination's signal is a materialised one"""
    sr, n, frames = 48000.0, 8, 128 * 40 + 17 + 3 * 4800
    ctx = waa.OfflineAudioContext(2, frames, sr, n_instances=n, binding=hip)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(rearm.dense(n, 2, frames), sr)
    src.connect(ctx.create_biquad_filter(type_="lowpass", frequency=200.0, q=1.0)).connect(ctx.create_gain(gain=0.5)).connect(ctx.destination())
    src.start()
    try:
        f32 = ctx.start_rendering_sync().data
        _, got = assert_loudness(ctx, f32, sr, "biquad -> gain")
        assert (got["n_blocks"] == 1).all() and np.isfinite(got["integrated"]).all()
    finally:
        ctx.close()


@gpu
def test_a_row_does_not_depend_on_its_batch_or_the_call(hip):
    sr = 8000.0
    frames = 70 * 800 + 5
    three = noise(3, 2, frames, 12, sr)
    big = noise(67, 2, frames, 13, sr)
    big[[5, 17, 66]] = three
    out = []
    for audio in (three[:1], three, big):
        ctx = passthrough(hip, audio, sr)
        try:
            ctx.start_rendering_sync()
            first, again = ctx.output_loudness_series(), ctx.output_loudness_series()
            assert first.tobytes() == again.tobytes() and first.any()
            assert ctx.output_loudness().tobytes() == ctx.output_loudness().tobytes()
            out.append((first, ctx.output_loudness()))
        finally:
            ctx.close()
    (z1, s1), (z3, s3), (z67, s67) = out
    assert z1.tobytes() == z3[:1].tobytes() and z3.tobytes() == z67[[5, 17, 66]].tobytes()
    assert s1.tobytes() == s3[:1].tobytes() and s3.tobytes() == s67[[5, 17, 66]].tobytes()


@gpu
def test_loudness_follows_a_rearmed_render(hip):
    sr, n, changed = 8000.0, 5, 3
    frames = 9 * 800 + 3
    first = noise(n, 2, frames, 14, sr)
    second = first.copy()
    second[changed] = noise(1, 2, frames, 15, sr)[0] * np.float32(0.5)
    ctx, donor = passthrough(hip, first, sr), passthrough(hip, second, sr)
    try:
        f32 = ctx.start_rendering_sync().data
        z_before, before = assert_loudness(ctx, f32, sr, "the first render")
        assert rearm.refill_from(ctx, donor) == 1
        f32b = rearm.render_again(ctx)
        z_after, after = assert_loudness(ctx, f32b, sr, "the re-armed render")
        others = [i for i in range(n) if i != changed]
        assert z_after[others].tobytes() == z_before[others].tobytes() and after[others].tobytes() == before[others].tobytes()
        assert (z_after[changed] != z_before[changed]).all() and after["integrated"][changed] != before["integrated"][changed]
    finally:
        ctx.close()
        donor.close()


@gpu
def test_more_rows_than_a_grid_dimension(hip):
    """65 537 contexts of one channel and one block at 8 kHz: 61 different clips over and over, so that the model runs on 62 rows
    (the first 61 contexts and the last one) and every other context is compared with the context that holds the same clip"""
    sr, n, frames, distinct = 8000.0, 65537, 4 * 800, 61
    tiled = np.arange(n) % distinct
    ctx = passthrough(hip, noise(distinct, 1, frames, 16, sr)[tiled], sr)
    try:
        picked = list(range(distinct)) + [n - 1]
        f32 = ctx.render_instances(picked)
        z, got = assert_loudness(ctx, f32, sr, "65537 contexts", rows=picked)
    finally:
        ctx.close()
    assert np.array_equal(z.view(np.uint64), z[:distinct][tiled].view(np.uint64))
    assert np.array_equal(got.view(np.uint8), got[:distinct][tiled].view(np.uint8))
    assert (got["n_blocks"] == 1).all() and (got["n_gated"] == 1).all()


@gpu
def test_refused_while_the_render_is_suspended(hip):
    sr, seen = 8000.0, []

    def callback(c):
        for call in (c.output_loudness, c.output_loudness_series, lambda: c.download_pcm16(normalize_loudness=-23.0)):
            with pytest.raises(waa.WaaError) as e:
                call()
            seen.append(e.value.status)

    frames = 128 * 50
    ctx = passthrough(hip, noise(2, 1, frames, 17, sr), sr)
    ctx.suspend_sync(2 * 128 / sr, callback)
    try:
        f32 = ctx.start_rendering_sync().data
        assert seen == [3, 3, 3]
        assert_loudness(ctx, f32, sr, "after the suspended render")
    finally:
        ctx.close()
    ctx = passthrough(hip, noise(2, 1, frames, 17, sr), sr).prepare()
    try:
        hip.check(hip.render_range(ctx._handle, 0, 2))
        stats = (waa.api.LoudnessStats * 2)()
        z = np.zeros((2, 1, frames // 800))
        assert hip.output_loudness(ctx._handle, None, stats) == 3 and "InvalidStateError" in hip.last_error().decode()
        assert hip.output_loudness_series(ctx._handle, z.ctypes.data_as(waa.api._DP)) == 3 and "InvalidStateError" in hip.last_error().decode()
        hip.check(hip.render_range(ctx._handle, 2, 48))
        hip.check(hip.output_loudness(ctx._handle, None, stats))
        assert stats[0].n_blocks == frames // 800 - 3
    finally:
        ctx.close()


# ---- normalising --------------------------------------------------------------------------------------------------------------------
def packed_model(f32, gain, n_out):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.stack([pcm_model.pack(f32[i] * np.float32(gain[i]), n_out) for i in range(f32.shape[0])])


@gpu
def test_normalize_loudness(hip):
    sr, h, n = 8000.0, 800, 6
    frames = 12 * h + 3
    rng = np.random.default_rng(18)
    audio = (rng.uniform(-1.0, 1.0, (n, 2, frames)) * np.array([0.01, 0.03, 0.1, 0.3, 1.0, 1.0]).reshape(n, 1, 1)).astype(np.float32)
    audio[2] = 0.0              # a silent context keeps gain 1
    audio[5, :, 4 * h] = 1.0    # (a peak of its own)
    ctx = passthrough(hip, audio, sr)
    try:
        f32 = ctx.start_rendering_sync().data
        loud = ctx.output_loudness()
        levels = ctx.output_levels()
        got = ctx.download_pcm16(normalize_loudness=-23.0)
        gain = np.ones(n, np.float32)
        ok = np.isfinite(loud["integrated"])
        gain[ok] = np.float32(10.0 ** ((-23.0 - loud["integrated"][ok]) / 20.0))
        assert ok.tolist() == [True, True, False, True, True, True] and gain[2] == 1.0
        assert got.tobytes() == ctx.download_pcm16(gain=gain).tobytes() == packed_model(f32, gain, 2).tobytes()
        limited = ctx.download_pcm16(normalize_loudness=-3.0, max_peak=0.5)
        g3 = np.ones(n, np.float32)
        g3[ok] = np.float32(10.0 ** ((-3.0 - loud["integrated"][ok]) / 20.0))
        peak = levels["peak"].max(axis=1).astype(np.float32)
        cap = np.full(n, np.inf, np.float32)
        np.divide(np.float32(0.5), peak, out=cap, where=peak > 0)
        assert (cap < g3).any()
        assert limited.tobytes() == ctx.download_pcm16(gain=np.minimum(g3, cap)).tobytes()
        assert int(np.abs(limited.astype(np.int32)).max()) <= 16384
    finally:
        ctx.close()
    # the packed clips ARE at -23 LUFS, where the pack clipped nothing
    clipped = (np.abs(f32 * gain[:, None, None]) * np.float32(32768.0) > 32767.0).any(axis=(1, 2))
    assert not clipped[ok].all()
    back = (got.astype(np.float32) / np.float32(32768.0)).transpose(0, 2, 1)
    z, _ = M.bound(back, sr)
    for i in np.flatnonzero(ok & ~clipped):
        r = M.gating(np.asarray(z[i], np.float64), h)
        assert abs(r["integrated"] + 23.0) <= 0.01, (i, r["integrated"])
