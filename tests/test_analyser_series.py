"""AnalyserNode series (spectrograms): waa_node_desc.i[1] = hop H > 0, i[2] = first pull quantum F make the eight analyser getters
answer with the rows of P pulls at the render quanta q_k = F + k H <= n_quanta (include/waa_hip.h).  The program of
the reference it stands for: a fresh analyser pulled inside suspend_sync callbacks at q_k * 128 / sample_rate (offline.rs:359-397),
the pull at q_k == n_quanta after start_rendering_sync; the smoothed spectrum carries from pull to pull (analysis.rs:337-344).

Ground truth.  Unsmoothed rows (tau = 0) do not depend on earlier pulls: the oracle's ONE pull on a context of q_k * 128 frames of
the same graph is pull k (a render is causal).  Smoothed rows: a float64 model of analysis.rs on the oracle's render of the
analyser's input, with a bound computed from the model's own f32 / f64 difference (test 3's docstring).

Byte time-domain rows asked for with n > fft_size: the reference's getter writes 128 into the surplus (its tmp is zeroed,
analysis.rs:266-276), as the single pull of both libraries does; the three other kinds leave the surplus untouched."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import web_audio_api_rs_amd as waa
from graphs import white_noise
from rearm import assert_same_bits, refill_from, render_again

RQ = 128
SR = 48000.0
NQ = 40
# the project's tolerances for ONE analyser pull (tests/test_full_size_all_instances.py:178-185): linear magnitude relative to the
# row's peak, and dB on the bins within 60 dB of the peak
ANALYSER_LIN_TOL = 4e-6
ANALYSER_DB_TOL = 0.035
KINDS = ("float_frequency", "byte_frequency", "float_time_domain", "byte_time_domain")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-audio-api-rs_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def _plain(be, noise, frames, fft, tau, hop=0, first=0, nch=None, device=-1):
    """source -> analyser -> destination (`nch` channels: the analyser's input is the source's layout)"""
    n_inst, n_ch, _ = noise.shape
    ctx = waa.OfflineAudioContext(nch or n_ch, frames, SR, n_instances=n_inst, binding=be, device=device)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(noise, SR)
    kw = dict(series_hop=hop, series_first=first) if hop or first else {}
    an = ctx.create_analyser(fft_size=fft, smoothing_time_constant=tau, min_decibels=-90.0, max_decibels=-10.0, **kw)
    src.connect(an).connect(ctx.destination())
    src.start()
    return ctx, an


def _series(an, n_f=None, n_t=None):
    return tuple(getattr(an, f"get_{k}_data_series")(n_t if "time" in k else n_f) for k in KINDS)


def _single_all(an):
    return tuple(getattr(an, f"get_{k}_data_all")() for k in KINDS)


def _chosen(qs, fft):
    """at most six pulls of a series: the first two, the middle one, the last two, the first whose window lies behind frame 0"""
    P = len(qs)
    idx = {0, min(1, P - 1), P // 2, max(P - 2, 0), P - 1}
    full = [k for k in range(P) if qs[k] * RQ >= fft]
    if full and len(idx) < 6:
        idx.add(full[0])
    return sorted(idx)[:6]


def _lin(db):
    return 10.0 ** (np.asarray(db, np.float64) / 20.0)


def _compare_with_single_pull(row, want, what, worst):
    """row / want: the four kinds [n_inst][...] of one series pull and of the oracle's single pull"""
    (gf, gb, gt, gbt), (of, ob, ot, obt) = row, want
    assert np.array_equal(gt, ot), (what, float(np.abs(gt - ot).max()))
    assert np.array_equal(gbt, obt), what
    gl, ol = _lin(gf), _lin(of)
    peak = ol.max(axis=1, keepdims=True)
    assert (peak > 0).all(), what
    lin = float((np.abs(gl - ol) / peak).max())
    loud = of > (of.max(axis=1, keepdims=True) - 60.0)
    db = float(np.abs(gf[loud].astype(np.float64) - of[loud]).max())
    byte = int(np.abs(gb.astype(int) - ob.astype(int)).max())
    worst["lin"], worst["db"], worst["byte"] = max(worst["lin"], lin), max(worst["db"], db), max(worst["byte"], byte)
    assert lin <= ANALYSER_LIN_TOL and db <= ANALYSER_DB_TOL and byte <= 1, (what, lin, db, byte)


def _assert_zero_ring(rows, what):
    f, b, t, bt = rows
    assert np.all(np.isneginf(f)) and not b.any() and not t.any() and np.all(np.signbit(t) == 0) and np.all(bt == 128), what


def _against_oracle_pulls(orc, build, series_rows, qs, fft, what):
    """series_rows: the four kinds [n_inst][P][...]; build(be, frames, series) -> (ctx, analyser)"""
    worst = dict(lin=0.0, db=0.0, byte=0)
    for k in _chosen(qs, fft):
        row = tuple(r[:, k] for r in series_rows)
        if qs[k] == 0:
            _assert_zero_ring(row, what)
            continue
        ctx, an = build(orc, int(qs[k]) * RQ, False)
        ctx.start_rendering_sync()
        want = _single_all(an)
        ctx.close()
        _compare_with_single_pull(row, want, f"{what} pull {k} (quantum {qs[k]})", worst)
    print(f"{what}: linear diff / row peak {worst['lin']:.3e} (bound {ANALYSER_LIN_TOL:.1e}), dB diff on loud bins {worst['db']:.3e} "
          f"(bound {ANALYSER_DB_TOL}), bytes {worst['byte']}")


# ---- CPU: the Python mirror, the C-ABI validation, plan-only batches ------------------------------------------------------

@pytest.mark.parametrize("frames,first,hop,want", [
    (NQ * RQ, 0, 1, list(range(0, 41))),
    (NQ * RQ, 5, 7, [5, 12, 19, 26, 33, 40]),
    (NQ * RQ, 40, 3, [40]),
    (NQ * RQ, 41, 1, None),
    (NQ * RQ + 37, 38, 3, [38, 41]),   # the truncated last quantum counts: 41 quanta
])
def test_series_quanta_and_pull_count(hip, frames, first, hop, want):
    ctx, an = _plain(hip, np.zeros((2, 1, frames), np.float32), frames, 256, 0.0, hop, first, device=waa.PLAN_ONLY)
    if want is None:
        with pytest.raises(waa.WaaError) as e:
            ctx.prepare()
        assert e.value.status == 1 and "no pull of the series falls inside the render" in str(e.value) and f"AnalyserNode {an.id}" in str(e.value)
        return
    assert an.series_quanta.tolist() == want
    line = [l for l in ctx.plan_describe().splitlines() if l.startswith("analyser series")]
    assert line == [f"analyser series: node {an.id}, {len(want)} pull(s) every {hop} quanta from quantum {first}, fft_size 256"], line
    got = an.get_float_frequency_data_series()
    assert got.shape == (2, len(want), 128) and np.all(np.isneginf(got))
    ctx.close()


@pytest.mark.parametrize("hop,first", [(-1, 0), (2, -3), (0, -1)])
def test_negative_series_fields_are_refused_with_the_node_named(hip, hop, first):
    ctx, an = _plain(hip, np.zeros((1, 1, 512), np.float32), 512, 64, 0.0, hop, first, device=waa.PLAN_ONLY)
    with pytest.raises(waa.WaaError) as e:
        ctx.prepare()
    assert e.value.status == 1 and f"AnalyserNode {an.id}" in str(e.value) and "cannot be negative" in str(e.value)


def test_plan_only_batch_returns_zero_ring_rows_in_the_series_layout(hip):
    frames = NQ * RQ
    ctx, an = _plain(hip, np.zeros((3, 2, frames), np.float32), frames, 64, 0.8, 7, 5, device=waa.PLAN_ONLY)
    ctx.prepare()
    f, b, t, bt = _series(an)
    assert f.shape == b.shape == (3, 6, 32) and t.shape == bt.shape == (3, 6, 64)
    assert f.dtype == t.dtype == np.float32 and b.dtype == bt.dtype == np.uint8
    _assert_zero_ring((f, b, t, bt), "plan-only")
    # the per-instance C getters write [P][n]
    one = np.full((6, 40), 3.0, np.float32)
    ctx._b.check(ctx._b.analyser_get_float_frequency_data(ctx._handle, an.id, 1, one.ctypes.data_as(waa.api._FP), 40))
    assert np.all(np.isneginf(one[:, :32])) and np.all(one[:, 32:] == 3.0)
    ctx.close()


def test_series_and_single_pull_methods_refuse_the_other_kind_of_node(hip, orc):
    frames = 8 * RQ
    ctx, an = _plain(hip, np.zeros((1, 1, frames), np.float32), frames, 64, 0.0, 2, 0, device=waa.PLAN_ONLY)
    plain = ctx.create_analyser(fft_size=64)
    ctx.prepare()
    for k in KINDS:
        with pytest.raises(ValueError, match="_series"):
            getattr(an, f"get_{k}_data")()
        with pytest.raises(ValueError, match="_series"):
            getattr(an, f"get_{k}_data_all")()
        with pytest.raises(ValueError, match="series_hop = 0"):
            getattr(plain, f"get_{k}_data_series")()
    ctx.close()
    # another binding pulls once per render: refused when the batch is built
    ctx, an = _plain(orc, np.zeros((1, 1, frames), np.float32), frames, 64, 0.0, 2, 0)
    with pytest.raises(waa.WaaError) as e:
        ctx.start_rendering_sync()
    assert e.value.status == 4 and "device library" in str(e.value)
    ctx.close()
    # series_first without a hop is not a series: the other binding renders it as the plain node it is
    ctx, an = _plain(orc, np.zeros((1, 1, frames), np.float32), frames, 64, 0.0, 0, 3)
    assert an.series_quanta.size == 0
    ctx.start_rendering_sync()
    assert an.get_float_frequency_data_all().shape == (1, 32)
    ctx.close()
    assert waa.OfflineAudioContext(1, frames, SR, binding=hip, device=waa.PLAN_ONLY).create_analyser(series_hop=2, series_first=-1).series_quanta.size == 0


def test_series_methods_check_a_callers_buffer(hip):
    frames = 8 * RQ
    ctx, an = _plain(hip, np.zeros((3, 1, frames), np.float32), frames, 64, 0.0, 2, 1, device=waa.PLAN_ONLY)
    ctx.prepare()
    good = np.zeros((3, 4, 32), np.float32)
    assert an.get_float_frequency_data_series(out=good) is good and np.all(np.isneginf(good))
    for bad in (np.zeros((3, 5, 32), np.float32), np.zeros((3, 4, 32), np.float64), np.zeros((3, 4, 64), np.float32)[:, :, ::2],
                np.zeros((3, 4, 32), np.uint8), [[0.0]]):
        with pytest.raises(ValueError, match="out: expected"):
            an.get_float_frequency_data_series(out=bad)
    with pytest.raises(ValueError, match="out: expected"):
        an.get_byte_time_domain_data_series(out=np.zeros((3, 4, 64), np.float32))
    assert an.get_byte_time_domain_data_series(n=10, out=np.zeros((3, 4, 10), np.uint8)).shape == (3, 4, 10)
    ctx.close()


def test_series_fields_are_part_of_a_nodes_identity_for_merging(hip):
    from web_audio_api_rs_amd.mixed import bucket_report
    frames = 8 * RQ
    ctxs = []
    for hop, first in ((2, 0), (2, 0), (2, 1), (3, 0), (0, 0)):
        ctx = waa.OfflineAudioContext(1, frames, SR, binding=hip, device=waa.PLAN_ONLY)
        src = ctx.create_buffer_source()
        src.set_buffer(waa.AudioBuffer(np.zeros((1, frames), np.float32), SR))
        src.connect(ctx.create_analyser(fft_size=64, series_hop=hop, series_first=first)).connect(ctx.destination())
        src.start()
        ctxs.append(ctx)
    assert bucket_report(ctxs) == [[0, 1], [2], [3], [4]]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_series_kernels_use_no_scratch_and_do_not_spill(tmp_path):
    """waa_analyser_series.hip compiled to ISA, the kernel descriptors read (as tests/test_kernel_resources.py does): four kernels,
    nothing in scratch memory, no spilled register; the transform stage's 1024-thread workgroups need <= 128 registers"""
    out = str(tmp_path / "series.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fgpu-flush-denormals-to-zero",
                           "--cuda-device-only", "-S", os.path.join(CSRC, "waa_analyser_series.hip"), "-o", out], stderr=subprocess.DEVNULL)
    res = {}
    for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.wavefront_size", open(out).read(), re.S):
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(2)).group(1))  # noqa: E731
        res[m.group(1)] = dict(vgpr=get("vgpr_count"), spill=get("vgpr_spill_count"), sgpr_spill=get("sgpr_spill_count"),
                               scratch=get("private_segment_fixed_size"))
    names = ("analyser_series_fft_kernel", "analyser_series_smooth_kernel", "analyser_series_bytes_kernel", "analyser_series_time_kernel")
    assert len(res) == 4 and all(any(n in k for k in res) for n in names), sorted(res)
    for name, r in res.items():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0 and r["vgpr"] <= 128, (name, r)


def _expected_run(fft, hop, P):
    """analyser_series_shape (waa_analyser_series.hip): up to 8 consecutive pulls per workgroup, fewer while the staged span and the
    transform buffer exceed 48 KB of LDS, one (nothing staged) when windows do not overlap"""
    run = min(8, P)
    while run > 1 and (2 * fft + (run - 1) * hop * RQ) * 4 > 48 * 1024:
        run -= 1
    return 1 if hop * RQ >= fft else run


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    """tools/analyser_series_emulate.cpp: waa_analyser_series.hip compiled for the HOST (kernels as functions, a launch as a loop
    over the blocks) — the index arithmetic of runs, spans, rows and the recursion, without a GPU"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("series") / "analyser_series_emulate"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "tools", "emulate_shim"),
                           os.path.join(ROOT, "tools", "analyser_series_emulate.cpp"), "-o", str(out)])
    return str(out)


@pytest.mark.parametrize("tau", [0.0, 0.7])
@pytest.mark.parametrize("fft,first,hop,nq,nch", [
    (32, 0, 1, 40, 1), (256, 0, 1, 40, 2), (256, 1, 3, 40, 2), (2048, 5, 7, 40, 2), (2048, 4, 4, 41, 4), (4096, 3, 2, 41, 2),
    (8192, 2, 1, 40, 1), (32768, 0, 1, 40, 2), (256, 40, 3, 40, 2), (4096, 0, 8, 40, 2), (4096, 1, 16, 80, 1), (2048, 0, 15, 90, 2)])
def test_host_replay_of_the_series_kernels(emulator, tmp_path, fft, first, hop, nq, nch, tau):
    """every run length and both LDS layouts (staged span / one pull per workgroup), windows that start in front of frame 0, the
    last pull at n_quanta: rows against the float64 model under the bound of test 3, time rows bit for bit"""
    path = str(tmp_path / "out.bin")
    subprocess.check_call([emulator, str(fft), str(first), str(hop), str(nq), str(nch), str(tau), path])
    raw = open(path, "rb").read()
    P, run, staged = np.frombuffer(raw, np.int32, 3)
    qs = np.arange(first, nq + 1, hop)
    assert P == len(qs) and staged == (run > 1)
    assert run == _expected_run(fft, hop, P)
    M, ni, off = fft // 2, 3, 12

    def take(dtype, shape):
        nonlocal off
        a = np.frombuffer(raw, dtype, int(np.prod(shape)), off).reshape(shape)
        off += a.nbytes
        return a
    db, by, tim, tby, by2 = (take(np.float32, (ni, P, M)), take(np.uint8, (ni, P, M)), take(np.float32, (ni, P, fft)),
                             take(np.uint8, (ni, P, fft)), take(np.uint8, (ni, P, M)))
    x = take(np.float32, (ni, nch, nq * RQ))
    assert off == len(raw)
    mono = {1: lambda: x[:, 0], 2: lambda: np.float32(0.5) * (x[:, 0] + x[:, 1]),
            4: lambda: np.float32(0.25) * (x[:, 0] + x[:, 1] + x[:, 2] + x[:, 3])}[nch]()
    padded = np.concatenate([np.zeros((ni, fft), np.float32), mono], axis=1)
    want_t = np.stack([padded[:, q * RQ:q * RQ + fft] for q in qs], axis=1)
    assert_same_bits(tim, want_t, "time-domain rows", axes=("instance", "pull", "frame"))
    assert np.array_equal(tby, np.clip(np.float32(128.0) * (np.float32(1.0) + want_t), 0.0, 255.0).astype(np.uint8))
    assert np.array_equal(by, by2)
    rows = _model_rows(mono[:, None, :], qs, fft)
    ratio, e_rec = _smoothing_bound_ratio(db, rows, tau)
    print(f"host replay fft {fft} F {first} H {hop} tau {tau}: run {run}, worst |rows - model| / bound = {ratio:.3f} (E_rec {e_rec:.3e})")
    assert ratio <= 1.0, (ratio, e_rec)
    if first == 0:
        assert np.all(np.isneginf(db[:, 0])) and not by[:, 0].any()


# ---- GPU ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n_inst", [3, 65])
@pytest.mark.parametrize("first,hop", [(0, 1), (1, 3), (5, 7)])
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("fft", [32, 256, 2048, 32768])
def test_unsmoothed_rows_match_the_oracles_single_pulls(hip, orc, fft, nch, first, hop, n_inst):
    """1. tau = 0: every chosen row of the series is the oracle's single pull on a context that ends at that quantum"""
    noise = white_noise(n_inst, nch, NQ * RQ, seed0=0x5E71E5 + fft)

    def build(be, frames, series):
        return _plain(be, noise, frames, fft, 0.0, hop if series else 0, first if series else 0)
    ctx, an = build(hip, NQ * RQ, True)
    ctx.start_rendering_sync()
    rows = _series(an)
    again = _series(an)  # (repeated calls return the same data)
    ctx.close()
    for a, b in zip(rows, again):
        assert_same_bits(a, b, "the second call", axes=("instance", "pull", "element"))
    qs = an.series_quanta
    assert rows[0].shape == (n_inst, len(qs), fft // 2) and rows[2].shape == (n_inst, len(qs), fft)
    _against_oracle_pulls(orc, build, rows, qs, fft, f"fft {fft} {nch}ch F {first} H {hop} x{n_inst}")


@pytest.mark.gpu
@pytest.mark.parametrize("tau", [0.0, 0.8])
@pytest.mark.parametrize("fft,first,hop", [(4096, 0, 8), (4096, 2, 6)])
def test_runs_that_the_lds_budget_shortens(hip, orc, fft, first, hop, tau):
    """1b. fft 4096 with hops of 8 and 6 quanta: the staged span of 8 pulls does not fit 48 KB of LDS, the workgroups own runs of 5
    and 6 pulls (and a shorter last run).  tau = 0 against the oracle's single pulls, tau = 0.8 against the model of test 3"""
    n_inst = 3
    P = len(range(first, NQ + 1, hop))
    assert 1 < _expected_run(fft, hop, P) < min(8, P)
    noise = white_noise(n_inst, 2, NQ * RQ, seed0=0x1D5 + hop)

    def build(be, frames, series):
        return _plain(be, noise, frames, fft, tau, hop if series else 0, first if series else 0)
    ctx, an = build(hip, NQ * RQ, True)
    ctx.start_rendering_sync()
    rows = _series(an)
    ctx.close()
    if tau == 0.0:
        _against_oracle_pulls(orc, build, rows, an.series_quanta, fft, f"fft {fft} F {first} H {hop}: LDS-limited run")
        return
    octx, _ = _plain(orc, noise, NQ * RQ, fft, tau)
    x = octx.start_rendering_sync().data
    octx.close()
    ratio, e_rec = _smoothing_bound_ratio(rows[0], _model_rows(x, an.series_quanta, fft), tau)
    print(f"LDS-limited run, fft {fft} F {first} H {hop} tau {tau}: worst |device - model| / bound = {ratio:.3f} (E_rec {e_rec:.3e})")
    assert ratio <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("tau", [0.0, 0.8])
def test_the_order_of_the_pulls_does_not_change_the_rows(hip, tau):
    """bytes first on a fresh batch (tau = 0: the transform stage writes bytes only, float rows asked for afterwards transform
    again), float first, and both orders on a second render, when every kind has a buffer and one pass fills both: the same bits"""
    noise = white_noise(3, 2, NQ * RQ, seed0=55)
    res = []
    for order in (("byte_frequency", "float_frequency"), ("float_frequency", "byte_frequency")):
        ctx, an = _plain(hip, noise, NQ * RQ, 512, tau, 3, 1)
        ctx.start_rendering_sync()
        got = {k: getattr(an, f"get_{k}_data_series")() for k in order}
        render_again(ctx)
        again = {k: getattr(an, f"get_{k}_data_series")() for k in order}
        ctx.close()
        res += [got, again]
    for other in res[1:]:
        for k in ("byte_frequency", "float_frequency"):
            assert_same_bits(other[k], res[0][k], f"{k} rows pulled in another order", axes=("instance", "pull", "bin"))
    assert np.isfinite(res[0]["float_frequency"]).all() and res[0]["byte_frequency"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("n_inst", [3, 65])
def test_series_node_and_plain_analyser_on_the_same_signal(hip, n_inst):
    """2. the last pull of a series that ends at n_quanta is the plain node's pull; the plain node's path is untouched: a twin
    context without the series node gives the same bits"""
    noise = white_noise(n_inst, 2, NQ * RQ, seed0=77)

    def build(with_series):
        ctx = waa.OfflineAudioContext(2, NQ * RQ, SR, n_instances=n_inst, binding=hip)
        src = ctx.create_buffer_source()
        src.set_buffer_batch(noise, SR)
        g = src.connect(ctx.create_gain(gain=0.25))
        plain = ctx.create_analyser(fft_size=1024, smoothing_time_constant=0.0)
        g.connect(plain).connect(ctx.destination())
        ser = None
        if with_series:
            ser = ctx.create_analyser(fft_size=1024, smoothing_time_constant=0.0, series_hop=4, series_first=4)
            g.connect(ser)
        src.start()
        return ctx, plain, ser
    ctx, plain, ser = build(True)
    out = ctx.start_rendering_sync().data
    assert ser.series_quanta[-1] == NQ
    rows = _series(ser)
    got = _single_all(plain)
    ctx.close()
    twin, tplain, _ = build(False)
    tout = twin.start_rendering_sync().data
    want = _single_all(tplain)
    twin.close()
    assert_same_bits(out, tout, "the render next to a series node")
    for a, b, k in zip(got, want, KINDS):
        assert_same_bits(a, b, f"the plain analyser's {k} pull next to a series node", axes=("instance", "element"))
    worst = dict(lin=0.0, db=0.0, byte=0)
    _compare_with_single_pull(tuple(r[:, -1] for r in rows), got, "last row against the plain node", worst)
    print(f"last row against the plain node: linear {worst['lin']:.3e}, dB {worst['db']:.3e}, bytes {worst['byte']}")


_LIBM_COSF = None


def _cosf(x):
    """the host libm's cosf, element by element: the library builds its window with it (numpy's float32 cosine is another
    implementation, and one ulp of a cosine is a relative 1e-3 of a window value near the window's ends, where it cancels)"""
    global _LIBM_COSF
    if _LIBM_COSF is None:
        import ctypes
        import ctypes.util
        fn = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").cosf
        fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
        _LIBM_COSF = fn
    return np.array([_LIBM_COSF(float(v)) for v in x], np.float32)


_WINDOWS = {}


def _blackman_f32(n):
    """generate_blackman (analysis.rs:14-24) in f32, as the library computes it on the host"""
    if n not in _WINDOWS:
        f = np.float32
        i = np.arange(n, dtype=np.float32)
        alpha = f(0.16)
        a0, a1, a2 = (f(1) - alpha) / f(2), f(1) / f(2), alpha / f(2)
        pi = f(np.pi)
        _WINDOWS[n] = (a0 - a1 * _cosf(f(2) * pi * i / f(n)) + a2 * _cosf(f(4) * pi * i / f(n))).astype(np.float32)
    return _WINDOWS[n]


def _model_rows(x, qs, fft):
    """x [n_inst][channels][frames] f32, the analyser's input: the unsmoothed rows |X| / N [n_inst][P][fft / 2] in f64 — down-mix
    and Blackman window in f32, numpy's rfft in f64"""
    if x.shape[1] == 1:
        mono = x[:, 0]
    else:
        mono = np.float32(0.5) * (x[:, 0] + x[:, 1])
    mono = np.concatenate([np.zeros((x.shape[0], fft), np.float32), mono.astype(np.float32)], axis=1)
    win = _blackman_f32(fft)
    rows = []
    with np.errstate(invalid="ignore", over="ignore"):
        for q in qs:
            seg = mono[:, q * RQ:q * RQ + fft] * win      # frames [q * 128 - fft, q * 128)
            rows.append(np.abs(np.fft.rfft(seg.astype(np.float64), axis=-1))[:, :fft // 2] / fft)
    return np.stack(rows, axis=1)


def _recursion(rows, tau, dtype):
    """analysis.rs:337-344 over the pulls, in `dtype`, in the reference's order: tau * last + (1 - tau) * norm, non-finite -> 0"""
    t = dtype(tau)
    one_minus = dtype(1) - t
    rows = rows.astype(dtype)
    out = np.empty_like(rows)
    last = np.zeros_like(rows[:, 0])
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(rows.shape[1]):
            v = t * last + one_minus * rows[:, k]
            last = np.where(np.isfinite(v), v, dtype(0)).astype(dtype)
            out[:, k] = last
    return out


def _smoothing_bound_ratio(dev_db, rows, tau):
    """rows: the model's unsmoothed rows (f64).  The recursion in f64 is the truth; run a second time in f32 it gives
    E_rec = max |f32 - f64| relative to the largest (unsmoothed) row peak so far.  A smoothed row is a convex combination of
    unsmoothed rows, each within ANALYSER_LIN_TOL of its own peak on the device, and two f32 evaluations of the recursion are
    each within E_rec of the f64 one: |device - model| <= (ANALYSER_LIN_TOL + 2 E_rec) * (largest row peak among pulls 0..k).
    Returns (worst ratio to that bound, E_rec)."""
    s64 = _recursion(rows, tau, np.float64)
    s32 = _recursion(rows, tau, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        peaks = np.where(np.isfinite(rows), rows, 0.0).max(axis=2)
    runpeak = np.maximum.accumulate(peaks, axis=1)[:, :, None]      # [n_inst][P][1]
    ok = runpeak[:, :, 0] > 0
    e_rec = float((np.abs(s32 - s64).max(axis=2)[ok] / runpeak[:, :, 0][ok]).max()) if ok.any() else 0.0
    bound = (ANALYSER_LIN_TOL + 2 * e_rec) * runpeak
    diff = np.abs(_lin(dev_db) - s64)
    assert (diff[~ok] == 0).all()          # (nothing but zeros so far: -inf dB exactly)
    ratio = float((diff[ok] / np.broadcast_to(bound, diff.shape)[ok]).max()) if ok.any() else 0.0
    return ratio, e_rec


@pytest.mark.gpu
@pytest.mark.parametrize("n_inst", [3, 65])
@pytest.mark.parametrize("hop", [1, 4])
@pytest.mark.parametrize("fft", [256, 2048])
@pytest.mark.parametrize("tau", [0.8, 0.3, 1.0])
def test_smoothed_rows_follow_the_recursion_of_the_reference(hip, orc, tau, fft, hop, n_inst):
    """3. the smoothed spectrum carries from pull to pull: a float64 model of analysis.rs on the oracle's render of the analyser's
    input, under the computed bound of _smoothing_bound_ratio (the worst ratio to the bound is printed)."""
    noise = white_noise(n_inst, 2, NQ * RQ, seed0=0x7A0 + fft + hop)
    ctx, an = _plain(hip, noise, NQ * RQ, fft, tau, hop, 0)
    ctx.start_rendering_sync()
    f, b, _, _ = _series(an)
    ctx.close()
    octx, _ = _plain(orc, noise, NQ * RQ, fft, tau)
    x = octx.start_rendering_sync().data       # source -> analyser -> destination: the output IS the analyser's input
    octx.close()
    if tau == 1.0:
        assert np.all(np.isneginf(f)) and not b.any()
        return
    rows = _model_rows(x, an.series_quanta, fft)
    ratio, e_rec = _smoothing_bound_ratio(f, rows, tau)
    print(f"smoothing tau {tau} fft {fft} H {hop} x{n_inst}: worst |device - model| / bound = {ratio:.3f} (E_rec {e_rec:.3e})")
    assert ratio <= 1.0
    # bytes: analysis.rs:395-399 applied to the device's own dB rows, exactly
    scaled = np.float32(255.0) / (np.float32(-10.0) - np.float32(-90.0)) * (f - np.float32(-90.0))
    want_b = np.clip(scaled, 0.0, 255.0).astype(np.uint8)
    assert np.array_equal(b, want_b)


@pytest.mark.gpu
def test_a_non_finite_sample_resets_the_smoothed_spectrum(hip, orc):
    """4. analysis.rs:343: a non-finite value becomes 0.  Context 1's buffer holds +inf at frame 700: the rows whose window holds
    it are -inf / byte 0, the first row behind it restarts from a zero spectrum, the other contexts do not notice"""
    fft, tau, n_inst = 256, 0.5, 3
    clean = white_noise(n_inst, 1, NQ * RQ, seed0=404)
    dirty = clean.copy()
    dirty[1, 0, 700] = np.inf
    res = []
    for noise in (dirty, clean):
        ctx, an = _plain(hip, noise, NQ * RQ, fft, tau, 1, 0)
        ctx.start_rendering_sync()
        res.append(_series(an)[:2])
        ctx.close()
    (f, b), (cf, cb) = res
    qs = an.series_quanta
    inside = [k for k, q in enumerate(qs) if q * RQ - fft <= 700 < q * RQ]
    assert inside == [6, 7]
    assert np.all(np.isneginf(f[1, inside])) and not b[1, inside].any()
    for i in (0, 2):
        assert_same_bits(f[i], cf[i], f"context {i} next to the non-finite sample", axes=("pull", "bin"))
        assert_same_bits(b[i], cb[i], f"context {i} next to the non-finite sample", axes=("pull", "bin"))
    assert_same_bits(f[1, :6], cf[1, :6], "context 1 in front of the non-finite sample", axes=("pull", "bin"))
    # behind it: the model restarted from a zero spectrum at pull 8 (input: the clean signal, which the windows from there on see)
    rows = _model_rows(clean[1:2], qs[8:], fft)
    ratio, e_rec = _smoothing_bound_ratio(f[1:2, 8:], rows, tau)
    print(f"finite rule: worst |device - restarted model| / bound behind the sample = {ratio:.3f} (E_rec {e_rec:.3e})")
    assert ratio <= 1.0
    assert np.isfinite(f[1, 8:]).all() and not np.array_equal(f[1, 8], cf[1, 8])  # (the clean render still carries pulls 0..7)


@pytest.mark.gpu
def test_series_behind_an_input_that_changes_its_channel_count(hip, orc):
    """5a. the graph of tests/test_dynamic_counts.py (analyser behind a 4-channel bus whose sources come and go): the down-mix
    follows the count of every quantum"""
    n = 3

    def build(be, frames, series):
        c = waa.OfflineAudioContext(2, frames, SR, n_instances=n, binding=be)

        def buf(nch, length, start, seed):
            s = c.create_buffer_source()
            s.set_buffer_batch(white_noise(n, nch, length, seed0=seed) * 0.5, SR)
            s.start_at(start)
            return s
        bus = c.create_gain(gain=0.8, channel_count=4, channel_count_mode="max", channel_interpretation="speakers")
        kw = dict(series_hop=5, series_first=3) if series else {}
        an = c.create_analyser(fft_size=2048, smoothing_time_constant=0.0, **kw)
        for s in (buf(1, NQ * RQ, 0.0, 41), buf(4, RQ * 12, RQ * 20.25 / SR, 42), buf(2, RQ * 8, RQ * 28.0 / SR, 43)):
            s.connect(bus)
        bus.connect(an).connect(c.create_biquad_filter(type_="highpass", frequency=500.0)).connect(c.destination())
        return c, an
    ctx, an = build(hip, NQ * RQ, True)
    assert "dynamic-count group" in ctx.plan_describe()
    ctx.start_rendering_sync()
    rows = _series(an)
    ctx.close()
    _against_oracle_pulls(orc, build, rows, an.series_quanta, 2048, "dynamic counts")


@pytest.mark.gpu
def test_series_inside_an_echo_loop(hip, orc):
    """5b. the analyser aliases the delay line of an echo loop: loops are settled before the pulls"""
    noise = white_noise(3, 2, NQ * RQ, seed0=17)

    def build(be, frames, series):
        c = waa.OfflineAudioContext(2, frames, SR, n_instances=3, binding=be)
        src = c.create_buffer_source()
        src.set_buffer_batch(noise, SR)
        ws = c.create_wave_shaper()
        delay = c.create_delay(1.0, delay_time=6 * RQ / SR)
        kw = dict(series_hop=3, series_first=2) if series else {}
        an = c.create_analyser(fft_size=512, smoothing_time_constant=0.0, **kw)
        src.connect(ws).connect(delay)
        delay.connect(c.create_gain(gain=0.5)).connect(ws)
        ws.connect(an)
        src.connect(c.destination())
        delay.connect(c.destination())
        src.start()
        return c, an
    ctx, an = build(hip, NQ * RQ, True)
    ctx.start_rendering_sync()
    rows = _series(an)
    ctx.close()
    _against_oracle_pulls(orc, build, rows, an.series_quanta, 512, "echo loop")


@pytest.mark.gpu
def test_series_behind_a_connection_made_and_cut_at_suspend_points(hip, orc):
    """5c. a gain joins the analyser's input at quantum 6 and leaves at 15"""
    noise = white_noise(3, 2, NQ * RQ, seed0=23)

    def build(be, frames, series):
        c = waa.OfflineAudioContext(2, frames, SR, n_instances=3, binding=be)
        src = c.create_buffer_source()
        src.set_buffer_batch(noise, SR)
        kw = dict(series_hop=2, series_first=1) if series else {}
        an = c.create_analyser(fft_size=256, smoothing_time_constant=0.0, **kw)
        g = c.create_gain(gain=0.5)
        src.connect(an).connect(c.destination())
        src.connect(g)
        src.start()
        nq = frames // RQ
        if 6 < nq:
            c.suspend_sync(6 * RQ / SR, lambda _: g.connect(an))
        if 15 < nq:
            c.suspend_sync(15 * RQ / SR, lambda _: g.disconnect(an))
        return c, an
    ctx, an = build(hip, NQ * RQ, True)
    ctx.start_rendering_sync()
    rows = _series(an)
    ctx.close()
    qs = an.series_quanta
    # (the pulls at quanta 7..15 hear 1.5 x the source in their last quanta: the rows differ from a render without the edit)
    _against_oracle_pulls(orc, build, rows, qs, 256, "edited graph")
    ks = [int(np.flatnonzero(qs == q)[0]) for q in (5, 7, 15, 17)]
    worst = dict(lin=0.0, db=0.0, byte=0)
    for k in ks:
        o, oan = build(orc, int(qs[k]) * RQ, False)
        o.start_rendering_sync()
        _compare_with_single_pull(tuple(r[:, k] for r in rows), _single_all(oan), f"edited graph pull at quantum {qs[k]}", worst)
        o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tau", [0.0, 0.8])
def test_series_after_rearm_equals_a_fresh_batch(hip, tau):
    """5d. waa_batch_rearm and a render of new audio drop the cached series: bit for bit a fresh batch's"""
    a, b = white_noise(3, 2, NQ * RQ, seed0=1), white_noise(3, 2, NQ * RQ, seed0=2)
    ctx, an = _plain(hip, a, NQ * RQ, 512, tau, 3, 1)
    ctx.start_rendering_sync()
    first = _series(an)
    donor, _ = _plain(hip, b, NQ * RQ, 512, tau, 3, 1)
    assert refill_from(ctx, donor) == 1
    render_again(ctx)
    got = _series(an)
    ctx.close()
    fresh, fan = _plain(hip, b, NQ * RQ, 512, tau, 3, 1)
    fresh.start_rendering_sync()
    want = _series(fan)
    fresh.close()
    for g, w, f, k in zip(got, want, first, KINDS):
        assert_same_bits(g, w, f"{k} series after re-arm", axes=("instance", "pull", "element"))
        assert not np.array_equal(g, f), k


@pytest.mark.gpu
@pytest.mark.parametrize("tau", [0.0, 0.6])
def test_layout_of_the_batch_and_per_instance_getters(hip, tau):
    """6. the per-instance C getter writes [P][n] = slice [instance] of the batch getter's [n_instances][P][n]; n smaller than the
    row: the first n bins / the most recent n frames; n larger: the surplus stays untouched (byte time-domain data: 128, as the
    reference's getter writes it)"""
    n_inst, fft = 4, 128
    ctx, an = _plain(hip, white_noise(n_inst, 1, NQ * RQ, seed0=9), NQ * RQ, fft, tau, 6, 2)
    ctx.start_rendering_sync()
    P = len(an.series_quanta)
    full = dict(zip(KINDS, _series(an)))
    b, h = ctx._b, ctx._handle
    for kind in KINDS:
        dtype = np.float32 if "float" in kind else np.uint8
        ptr_t = waa.api._FP if dtype == np.float32 else waa.api.C.POINTER(waa.api.C.c_uint8)
        width = fft if "time" in kind else fft // 2
        sentinel = dtype(77)
        for n in (width, 10, width + 9):
            allv = np.full((n_inst, P, n), sentinel, dtype)
            b.check(getattr(b, f"analyser_get_{kind}_data_batch")(h, an.id, allv.ctypes.data_as(ptr_t), n))
            one = np.full((P, n), sentinel, dtype)
            b.check(getattr(b, f"analyser_get_{kind}_data")(h, an.id, 2, one.ctypes.data_as(ptr_t), n))
            assert_same_bits(one, allv[2], f"{kind} n = {n}: instance 2", axes=("pull", "element"))
            m = min(n, width)
            want = full[kind][:, :, width - m:] if "time" in kind else full[kind][:, :, :m]
            assert_same_bits(allv[:, :, :m], np.ascontiguousarray(want), f"{kind} n = {n}", axes=("instance", "pull", "element"))
            assert np.all(allv[:, :, m:] == (128 if kind == "byte_time_domain" else sentinel)), (kind, n)
            # the Python mirror hands the library a zeroed array: the same rows, the surplus as the library leaves it
            mirror = getattr(an, f"get_{kind}_data_series")(n)
            assert_same_bits(np.ascontiguousarray(mirror[:, :, :m]), np.ascontiguousarray(allv[:, :, :m]), f"{kind} n = {n}: the Python mirror",
                             axes=("instance", "pull", "element"))
            assert np.all(mirror[:, :, m:] == (128 if kind == "byte_time_domain" else 0)), (kind, n)
    assert np.abs(full["float_time_domain"]).max() > 0.1 and np.isfinite(full["float_frequency"][:, 1:]).all()
    ctx.close()
