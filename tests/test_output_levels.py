"""Levels of the rendered output computed on the device (waa_output_levels, waa_output_level_series) and the gained PCM pack
(waa_download_all_pcm16_gain), include/waa_hip_device.h; the Python mirror OfflineAudioContext.output_levels / output_level_series /
download_pcm16.

Every GPU test compares with the numpy model (tests/levels_model.py, tests/pcm_model.py) applied to what waa_download_all returned
from the SAME batch, so nothing here depends on what a graph does to a sample.  All comparisons are bit equality (uint32 / uint64
views of the floats); there is no tolerance anywhere."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import web_audio_api_rs_amd as waa
import batch_graphs as G
import levels_model as M
import pcm_model
import rearm
import test_launch_list as L
from test_caller_boundary import SPECIALS as PACK_SPECIALS, pack_source

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "web-audio-api-rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SR, RQ = 48000.0, 128
I16P = C.POINTER(C.c_int16)
FIELDS = ("sum_sq", "n_nonfinite", "first_nonfinite", "n_clipped", "peak")

# the values section 1 of the definitions names: non-finite, both zeros, a denormal, a finite value whose product with 32768
# overflows, and the two clamp edges from both sides
SPECIALS = np.array([np.nan, 3e38, np.inf, -np.inf, -0.0, 1e-40, 1.0, -1.0, 32767.0 / 32768.0,
                     float(np.nextafter(np.float32(-1.0), np.float32(-2.0))), -3e38], np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize])


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    diff = bits(got) != bits(want)
    if diff.any():
        k = tuple(int(v) for v in np.unravel_index(int(np.argmax(diff)), diff.shape))
        raise AssertionError(f"{what}: {int(diff.sum())} of {got.size} differ; the first at {k}: got {got[k]!r}, want {want[k]!r}")


def assert_stats(got, want, what):
    for f in FIELDS:
        assert_bits(got[f], want[f], f"{what}: {f}")


def assert_levels(ctx, f32, what):
    """output_levels and output_level_series of the rendered context against the model of its f32 download; returns the stats"""
    got = ctx.output_levels()
    assert got.shape == f32.shape[:2]
    assert_stats(got, M.stats(f32), what)
    peak, sum_sq = ctx.output_level_series()
    want_p, want_e = M.series(f32)
    assert_bits(peak, want_p, f"{what}: p_q")
    assert_bits(sum_sq, want_e, f"{what}: e_q")
    return got


# ---- the model against itself ---------------------------------------------------------------------------------------------------
def _scalar_stats(x):
    """section 1 restated sample by sample in plain Python (floats are f64; f32 steps go through numpy scalars)"""
    L_ = len(x)
    nq = -(-L_ // RQ)
    p_q, e_q = [], []
    n_nonfinite, first, n_clipped = 0, 0xFFFFFFFFFFFFFFFF, 0
    for q in range(nq):
        s, top = [0.0] * RQ, 0
        for j in range(RQ):
            f = q * RQ + j
            if f >= L_:
                continue
            a = int(np.float32(x[f]).view(np.uint32)) & 0x7FFFFFFF
            e = a >> 23
            if e == 255:
                n_nonfinite += 1
                first = min(first, f)
                continue
            top = max(top, a)
            if 1 <= e <= 254:
                s[j] = float(x[f]) * float(x[f])
            with np.errstate(over="ignore"):
                v = np.float32(x[f]) * np.float32(32768.0)
            if v > np.float32(32767.0) or v < np.float32(-32768.0):
                n_clipped += 1
        while len(s) > 1:
            s = [s[2 * k] + s[2 * k + 1] for k in range(len(s) // 2)]
        p_q.append(top)
        e_q.append(s[0])
    total = 0.0
    for m in range(-(-nq // 64)):
        blk = (e_q[64 * m:64 * m + 64] + [0.0] * 64)[:64]
        while len(blk) > 1:
            blk = [blk[2 * k] + blk[2 * k + 1] for k in range(len(blk) // 2)]
        total = total + blk[0]
    return p_q, e_q, dict(sum_sq=total, n_nonfinite=n_nonfinite, first_nonfinite=first, n_clipped=n_clipped, peak=max(p_q))


def test_the_model_equals_a_scalar_restatement():
    rng = np.random.default_rng(300)
    x = rng.uniform(-1.2, 1.2, 300).astype(np.float32)
    x[[0, 5, 127, 128, 255, 256, 299]] = SPECIALS[[4, 0, 1, 2, 5, 6, 9]]
    x[40:44] = SPECIALS[[3, 7, 8, 10]]
    p_q, e_q, st = _scalar_stats(x)
    got_p, got_e = M.series(x)
    assert [int(v) for v in bits(got_p)] == p_q
    assert [float(v).hex() for v in got_e] == [v.hex() for v in e_q]
    got = M.stats(x)
    assert float(got["sum_sq"]).hex() == st["sum_sq"].hex() and int(bits(got["peak"]).reshape(-1)[0]) == st["peak"]
    assert (int(got["n_nonfinite"]), int(got["first_nonfinite"]), int(got["n_clipped"])) == (st["n_nonfinite"], st["first_nonfinite"], st["n_clipped"])
    assert st["n_nonfinite"] == 3 and st["first_nonfinite"] == 5 and st["n_clipped"] > 3
    # rows are independent of each other and of the shape they come in
    both = np.stack([x, x[::-1]]).reshape(1, 2, 300)
    assert_stats(M.stats(both)[0, 0], got, "row 0 of a batch")
    empty = M.stats(np.zeros((2, 0), np.float32))
    assert (empty["first_nonfinite"] == M.NONE).all() and not empty["sum_sq"].any()


@pytest.mark.parametrize("n", [1, 127, 128, 129, 8192, 8193, 16677])
def test_the_models_energy_is_within_the_first_order_bound_of_fsum(n):
    """any order of adding N non-negative terms is within N * 2^-53 * sum of the exact sum, to first order"""
    x = np.random.default_rng(n).uniform(-1.2, 1.2, n).astype(np.float32)
    exact = math.fsum(float(v) * float(v) for v in x)
    assert abs(float(M.stats(x)["sum_sq"]) - exact) <= n * 2.0 ** -53 * exact


@pytest.mark.parametrize("lanes", [32, 64])
def test_an_xor_butterfly_gives_every_lane_the_trees_root(lanes):
    rng = np.random.default_rng(lanes)
    v = rng.uniform(0.0, 2.0, (50, lanes)) * 10.0 ** rng.integers(-12, 12, (50, lanes))
    fly = M.butterfly(v)
    assert_bits(fly, np.repeat(M.pair_tree(v)[:, None], lanes, axis=1), f"{lanes} lanes")
    # a lane's four frames first, then 32 lanes: the 128-frame tree
    s = rng.uniform(0.0, 1.5, (50, 128))
    lane = (s[:, 0::4] + s[:, 1::4]) + (s[:, 2::4] + s[:, 3::4])
    assert_bits(M.butterfly(lane)[:, 0], M.pair_tree(s), "four frames per lane, 32 lanes")


def test_the_clip_count_on_the_edge_values():
    table = [(1.0, True), (-1.0, False), (32767.0 / 32768.0, False), (float(np.nextafter(np.float32(-1.0), np.float32(-2.0))), True),
             (float(np.nextafter(np.float32(32767.0 / 32768.0), np.float32(2.0))), True), (3e38, True), (-3e38, True),
             (np.inf, False), (-np.inf, False), (np.nan, False), (0.0, False), (-0.0, False), (1e-40, False), (-1e-40, False), (0.5, False)]
    x = np.array([v for v, _ in table], np.float32)
    assert M.clipped(x).tolist() == [c for _, c in table]
    assert int(M.stats(x)["n_clipped"]) == 5 and int(M.stats(x)["n_nonfinite"]) == 3 and int(M.stats(x)["first_nonfinite"]) == 7
    # these are the samples the packer's clamp changes: v = x * 32768 differs from the clamped v (the packer's own expression)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x * np.float32(32768.0)
        clamped = np.where(v < np.float32(-32768.0), np.float32(-32768.0), np.where(v > np.float32(32767.0), np.float32(32767.0), v))
    assert ((v != clamped) & np.isfinite(x)).tolist() == [c for _, c in table]
    assert float(M.stats(x)["peak"]) == float(np.float32(3e38))
    assert bits(M.stats(np.float32([1e-40, 0.0]))["peak"]) == bits(np.float32(1e-40))  # a denormal counts with its own bits


# ---- the C ABI and its mirror, without a device -------------------------------------------------------------------------------------
NEW = ("output_levels", "output_level_series", "download_all_pcm16_gain")


def test_the_header_declares_the_library_exports_and_api_binds(hip):
    header = open(os.path.join(ROOT, "include", "waa_hip_device.h")).read()
    for name in NEW:
        assert re.search(r"waa_status waa_%s\(waa_batch\*" % name, header), name
        assert name in waa.api.ABI_DEVICE and callable(getattr(hip, name))
        assert getattr(hip.lib, "waa_" + name) is not None
    m = re.search(r"typedef struct waa_level_stats \{(.*?)\} waa_level_stats;", header, re.S)
    fields = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split()
    assert " ".join(fields) == "double sum_sq; uint64_t n_nonfinite, first_nonfinite, n_clipped; float peak; uint32_t reserved;"
    assert C.sizeof(waa.api.LevelStats) == 40 and waa.api.LEVEL_STATS_DTYPE.itemsize == 40
    for name, _ in waa.api.LevelStats._fields_:
        assert getattr(waa.api.LevelStats, name).offset == waa.api.LEVEL_STATS_DTYPE.fields[name][1], name
    # (the library's side of "40 bytes" is a static_assert next to the entry points: a library that exports them was built with it)


def _plan_only(hip, n=2, ch=2, frames=300):
    ctx = waa.OfflineAudioContext(ch, frames, SR, n_instances=n, binding=hip, device=waa.PLAN_ONLY)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(np.zeros((n, ch, frames), np.float32), SR)
    src.connect(ctx.destination())
    src.start()
    return ctx.prepare()


def test_refusals_without_a_device(hip):
    ctx = _plan_only(hip)
    h = ctx._handle
    stats = (waa.api.LevelStats * 4)()
    peak, pcm, gain = np.zeros(2 * 2 * 3, np.float32), np.zeros(2 * 300 * 2, np.int16), np.ones(2, np.float32)
    fp, ip = waa.api._fp, lambda a: a.ctypes.data_as(I16P)
    null = [(lambda: hip.output_levels(None, stats), "null batch / destination"), (lambda: hip.output_levels(h, None), "null batch / destination"),
            (lambda: hip.output_level_series(None, fp(peak), None), "both destinations null"),
            (lambda: hip.output_level_series(h, None, None), "both destinations null"),
            (lambda: hip.download_all_pcm16_gain(None, ip(pcm), fp(gain)), "null batch / destination / gains"),
            (lambda: hip.download_all_pcm16_gain(h, None, fp(gain)), "null batch / destination / gains"),
            (lambda: hip.download_all_pcm16_gain(h, ip(pcm), None), "null batch / destination / gains")]
    for call, text in null:
        assert call() == 1 and text in hip.last_error().decode(), text
    for call in (lambda: hip.output_levels(h, stats), lambda: hip.output_level_series(h, fp(peak), None),
                 lambda: hip.download_all_pcm16_gain(h, ip(pcm), fp(gain))):
        assert call() == 5 and hip.last_error().decode() == "plan-only batch has no device"
    # the mirror: nothing rendered yet
    for call in (ctx.output_levels, ctx.output_level_series, ctx.download_pcm16, lambda: ctx.download_pcm16(gain=gain)):
        with pytest.raises(waa.WaaError, match="nothing rendered yet") as e:
            call()
        assert e.value.status == 3
    with pytest.raises(ValueError, match="not both"):
        ctx.download_pcm16(gain=gain, normalize_peak=0.5)
    ctx.close()


def test_another_binding_is_out_of_scope(orc):
    ctx = waa.OfflineAudioContext(1, 256, SR, n_instances=2, binding=orc)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(np.zeros((2, 1, 256), np.float32), SR)
    src.connect(ctx.destination())
    src.start()
    ctx.start_rendering_sync()
    for call in (ctx.output_levels, ctx.output_level_series, lambda: ctx.download_pcm16(gain=[1.0, 1.0]), lambda: ctx.download_pcm16(normalize_peak=0.5)):
        with pytest.raises(waa.WaaError, match="feature of the device library") as e:
            call()
        assert e.value.status == 4
    ctx.close()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_levels_code_object(tmp_path):
    """waa_levels.hip compiled to ISA with the library's flags, only the metadata read (as tests/test_compressor_reduction.py reads its
    file): the three kernels spill nothing and use no scratch; the streaming pass stays within 64 vector registers — 512 / 64 is eight
    wavefronts per SIMD, so registers never limit how many loads are in flight"""
    out = str(tmp_path / "waa_levels.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fgpu-flush-denormals-to-zero",
                           "--cuda-device-only", "-S", os.path.join(CSRC, "waa_levels.hip"), "-o", out], stderr=subprocess.DEVNULL)
    res = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)(.*?)\.wavefront_size", open(out).read(), re.S):
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(2)).group(1))  # noqa: E731
        res[re.search(r"\.name:\s+(\S+)", m.group(2)).group(1)] = {
            "vgpr": get("vgpr_count"), "spill": get("vgpr_spill_count"), "sgpr_spill": get("sgpr_spill_count"),
            "scratch": get("private_segment_fixed_size"), "lds": int(m.group(1))}
    names = {k: next(n for n in res if k in n) for k in ("output_levels_kernel", "output_level_rows_kernel", "pcm16_pack_gain_kernel")}
    assert len(res) == 3, sorted(res)
    for r in res.values():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, res
    assert res[names["output_levels_kernel"]]["vgpr"] <= 64, res
    assert res[names["output_levels_kernel"]]["lds"] <= 1024 and res[names["pcm16_pack_gain_kernel"]]["lds"] == 0, res


@pytest.mark.parametrize("library", ["product", pytest.param("measure", marks=pytest.mark.measure)])
def test_the_plan_text_is_what_it_was(hip, monkeypatch, library):
    """nothing of this is a plan step: the plan text of two graphs of tests/batch_graphs.py is word for word what
    tests/golden/launch_lists holds for them, and names none of the new kernels — also after the new calls were made.  The golden
    text ends with the launch list, which only the measurement build prints (WAA_PLAN_LAUNCHES): the product's text is the part in
    front of it."""
    full = library == "measure"
    cut = (lambda t: t) if full else (lambda t: t.partition("launch 0: ")[0])  # noqa: E731
    golden = cut(L._sections(L._golden("named"))["fm_pair"])
    # b_fm_pair of contexts 0 .. 2 at 40 quanta is the golden's "fm_pair"; b_iir (one coefficient set per context) is in no golden
    # file: it is compared with itself across the new calls below
    fm_pair = lambda be: G.build(G.b_fm_pair, be, [0, 1, 2], device=waa.PLAN_ONLY, frames=RQ * 40)  # noqa: E731
    build = lambda be: G.build(G.b_iir, be, [0, 1, 2], device=waa.PLAN_ONLY)  # noqa: E731
    assert L.describe(hip, fm_pair, {}, monkeypatch.setenv, monkeypatch.delenv) == golden
    text = L.describe(hip, build, {}, monkeypatch.setenv, monkeypatch.delenv)
    for t in (golden, text):
        assert ("\nlaunch 0: " in t) == full and "iir" in text and "output_level" not in t and "pcm16_pack" not in t
    # a refused call of each new entry point leaves the plan as it was
    monkeypatch.setenv("WAA_PLAN_LAUNCHES", "1")
    ctx = build(hip)
    before = ctx.plan_describe()
    stats = (waa.api.LevelStats * 6)()
    assert hip.output_levels(ctx._handle, stats) == 5
    assert hip.output_level_series(ctx._handle, None, np.zeros(6 * 17).ctypes.data_as(waa.api._DP)) == 5
    after = ctx.plan_describe()
    ctx.close()
    strip = lambda t: t.partition("\n")[0].split(" | timing:")[0] + "\n" + t.partition("\n")[2]  # noqa: E731
    assert strip(before) == strip(after) == text


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
def passthrough(hip, audio, n_out=None):
    """BufferSource -> destination, one AudioBuffer per context; prepared, not rendered"""
    n, ch, frames = audio.shape
    ctx = waa.OfflineAudioContext(n_out or ch, frames, SR, n_instances=n, binding=hip)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(audio, SR)
    src.connect(ctx.destination())
    src.start()
    return ctx


def planted(n, ch, frames, seed=0):
    """white noise in +-1.2 with the special values planted at the first and the last frame of every row and on both sides of the
    16-byte (3 | 4), quantum (127 | 128, 255 | 256) and block (8191 | 8192, 16383 | 16384) edges, in another rotation for every row"""
    rng = np.random.default_rng([n, ch, frames, seed])
    x = rng.uniform(-1.2, 1.2, (n, ch, frames)).astype(np.float32)
    at = sorted({f for f in (0, 3, 4, 126, 127, 128, 129, 255, 256, 8190, 8191, 8192, 8193, 16383, 16384, frames - 2, frames - 1) if 0 <= f < frames})
    for i in range(n):
        for c in range(ch):
            for k, f in enumerate(at):
                x[i, c, f] = SPECIALS[(k + i * ch + c) % SPECIALS.size]
    return x


LENGTHS = [1, 127, 128, 129, 8191, 8192, 8193, 128 * 130 + 37]


@gpu
@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 3, 67])
@pytest.mark.parametrize("frames", LENGTHS)
def test_levels_equal_the_model(hip, frames, n, ch):
    ctx = passthrough(hip, planted(n, ch, frames))
    try:
        f32 = ctx.start_rendering_sync().data
        got = assert_levels(ctx, f32, f"{n} x {ch} x {frames}")
    finally:
        ctx.close()
    # the test's subject arrived: non-finite samples and samples the clamp changes (one sample in all cannot be both)
    arrived = [int(got["n_nonfinite"].sum()) > 0, int(got["n_clipped"].sum()) > 0]
    assert all(arrived) if n * ch * frames > 1 else any(arrived), got
    assert int(got["first_nonfinite"][0, 0]) == 0  # (row 0 starts with the NaN)


@gpu
def test_rows_of_zeros(hip):
    """a context with nothing connected to its destination, and a 2-channel context whose destination carries one channel"""
    frames = 128 * 3 + 5
    ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=3, binding=hip)
    ctx.create_buffer_source().set_buffer_batch(planted(3, 2, frames), SR)
    try:
        f32 = ctx.start_rendering_sync().data
        assert not bits(f32).any()
        got = assert_levels(ctx, f32, "nothing connected")
        assert not got["sum_sq"].any() and not got["peak"].any() and (got["first_nonfinite"] == M.NONE).all()
    finally:
        ctx.close()
    ctx = passthrough(hip, planted(3, 1, frames), n_out=2)
    ctx.destination().set_channel_count(1)
    try:
        f32 = ctx.start_rendering_sync().data
        assert not bits(f32[:, 1]).any() and bits(f32[:, 0]).any()
        got = assert_levels(ctx, f32, "one of two channels carried")
        assert (got["n_clipped"][:, 0] > 0).all() and not got["n_clipped"][:, 1].any() and not got["peak"][:, 1].any()
    finally:
        ctx.close()


@gpu
def test_levels_of_a_render_with_state(hip):
    """BufferSource -> Biquad -> Gain(3.0): the destination's signal is a materialised one, written by the streaming filter"""
    n, frames = 67, 128 * 70 + 5
    ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=n, binding=hip)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(rearm.dense(n, 2, frames), SR)
    src.connect(ctx.create_biquad_filter(type_="lowpass", frequency=3000.0, q=1.0)).connect(ctx.create_gain(gain=3.0)).connect(ctx.destination())
    src.start()
    try:
        f32 = ctx.start_rendering_sync().data
        got = assert_levels(ctx, f32, "biquad -> gain")
        assert (got["n_clipped"] > 0).all() and not got["n_nonfinite"].any()
    finally:
        ctx.close()


def _levels(ctx):
    peak, sum_sq = ctx.output_level_series()
    return ctx.output_levels(), peak, sum_sq


@gpu
def test_a_row_does_not_depend_on_its_batch_or_the_call(hip):
    frames = 128 * 70 + 5
    three = planted(3, 2, frames, seed=1)
    big = planted(67, 2, frames, seed=2)
    big[[5, 17, 66]] = three
    out = []
    for audio in (three, big):
        ctx = passthrough(hip, audio)
        try:
            f32 = ctx.start_rendering_sync().data
            first, again = _levels(ctx), _levels(ctx)
            assert_stats(first[0], M.stats(f32), "the first call")
            assert_stats(again[0], first[0], "two calls in a row")
            assert_bits(again[1], first[1], "two calls in a row: p_q")
            assert_bits(again[2], first[2], "two calls in a row: e_q")
            out.append(first)
        finally:
            ctx.close()
    (s3, p3, e3), (s67, p67, e67) = out
    assert_stats(s67[[5, 17, 66]], s3, "contexts 5, 17, 66 of 67 against a batch of 3")
    assert_bits(p67[[5, 17, 66]], p3, "p_q")
    assert_bits(e67[[5, 17, 66]], e3, "e_q")


@gpu
def test_levels_follow_a_rearmed_render(hip):
    """waa_batch_rearm with new audio in ONE context: nothing is kept from the first render — that context's rows change, no other"""
    n, frames, changed = 5, 128 * 9 + 3, 3
    first = planted(n, 2, frames, seed=3)
    second = first.copy()
    second[changed] = planted(1, 2, frames, seed=4)[0] * np.float32(0.5)
    ctx, donor = passthrough(hip, first), passthrough(hip, second)
    try:
        f32 = ctx.start_rendering_sync().data
        before = _levels(ctx)
        assert_stats(before[0], M.stats(f32), "the first render")
        assert rearm.refill_from(ctx, donor) == 1
        f32b = rearm.render_again(ctx)
        after = _levels(ctx)
        assert_stats(after[0], M.stats(f32b), "the re-armed render")
        assert_bits(after[1], M.series(f32b)[0], "the re-armed render: p_q")
        assert_bits(after[2], M.series(f32b)[1], "the re-armed render: e_q")
        others = [i for i in range(n) if i != changed]
        assert_stats(after[0][others], before[0][others], "the other contexts")
        assert_bits(after[2][others], before[2][others], "the other contexts: e_q")
        assert (bits(after[0]["sum_sq"][changed]) != bits(before[0]["sum_sq"][changed])).all()
    finally:
        ctx.close()
        donor.close()


@gpu
def test_more_rows_than_a_grid_dimension(hip):
    n, frames = 65537, 130
    audio = planted(n, 1, frames, seed=5)
    ctx = passthrough(hip, audio)
    try:
        f32 = ctx.start_rendering_sync().data
        got = assert_levels(ctx, f32, "65537 contexts")
        assert int(got["n_nonfinite"].sum()) > n and int(got["n_clipped"].sum()) > n
    finally:
        ctx.close()


@gpu
def test_refused_while_the_render_is_suspended(hip):
    seen = []

    def callback(c):
        for call in (c.output_levels, c.output_level_series, lambda: c.download_pcm16(gain=np.ones(2, np.float32))):
            with pytest.raises(waa.WaaError) as e:
                call()
            seen.append(e.value.status)

    frames = 128 * 6
    ctx = passthrough(hip, planted(2, 1, frames))
    ctx.suspend_sync(2 * 128 / SR, callback)
    try:
        f32 = ctx.start_rendering_sync().data
        assert seen == [3, 3, 3]
        assert_levels(ctx, f32, "after the suspended render")
    finally:
        ctx.close()
    # the C ABI in front of the last range of a ranged render
    ctx = passthrough(hip, planted(2, 1, frames)).prepare()
    try:
        hip.check(hip.render_range(ctx._handle, 0, 2))
        stats = (waa.api.LevelStats * 2)()
        assert hip.output_levels(ctx._handle, stats) == 3 and "InvalidStateError" in hip.last_error().decode()
        pcm = np.zeros((2, frames, 1), np.int16)
        assert hip.download_all_pcm16_gain(ctx._handle, pcm.ctypes.data_as(I16P), waa.api._fp(np.ones(2, np.float32))) == 3
        hip.check(hip.render_range(ctx._handle, 2, 4))
        hip.check(hip.output_levels(ctx._handle, stats))
    finally:
        ctx.close()


# ---- the gained pack ----------------------------------------------------------------------------------------------------------------
def packed_model(f32, gain, n_out):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.stack([pcm_model.pack(f32[i] * np.float32(gain[i]), n_out) for i in range(f32.shape[0])])


def gains_for(n, seed):
    rng = np.random.default_rng(seed)
    table = np.float32([0.0, -1.0, 0.5, 1e-30, 1e30])
    g = np.where(rng.random(n) < 0.5, table[rng.integers(0, table.size, n)], rng.uniform(-3.0, 3.0, n).astype(np.float32))
    g[:table.size] = table
    return g.astype(np.float32)


@gpu
def test_a_gain_of_one_is_the_plain_pack(hip):
    ctx = passthrough(hip, pack_source(67, 2, 1000))
    try:
        ctx.start_rendering_sync()
        plain = ctx.download_pcm16()
        assert_bits(ctx.download_pcm16(gain=np.ones(67, np.float32)), plain, "gain 1")
        assert np.abs(plain.astype(np.int32)).max() == 32768
    finally:
        ctx.close()


@gpu
def test_the_gained_pack_equals_the_model(hip):
    n = 67
    audio = pack_source(n, 2, 1000)
    audio[:, :, 100:100 + SPECIALS.size] = SPECIALS
    gain = gains_for(n, 67)
    ctx = passthrough(hip, audio)
    try:
        f32 = ctx.start_rendering_sync().data
        assert np.isnan(f32).any() and np.isinf(f32).any()
        got = ctx.download_pcm16(gain=gain)
    finally:
        ctx.close()
    assert_bits(got, packed_model(f32, gain, 2), "67 x 2 x 1000")
    assert len({got[i].tobytes() for i in range(n)}) > n // 2


@gpu
def test_products_on_ties_and_on_the_clamp_edges(hip):
    """x * gain is exact here (gain a power of two), so the products ARE the packer's ties and edges"""
    want = np.float32(PACK_SPECIALS[np.isfinite(PACK_SPECIALS)])
    gain = np.float32([0.5, -0.5, 2.0, -0.25])
    audio = np.stack([(want / g)[None, :] for g in gain]).astype(np.float32)  # [4, 1, frames]
    ctx = passthrough(hip, audio)
    try:
        f32 = ctx.start_rendering_sync().data
        got = ctx.download_pcm16(gain=gain)
    finally:
        ctx.close()
    assert_bits(got, packed_model(f32, gain, 1), "ties and edges")
    normal = np.abs(want) >= np.finfo(np.float32).tiny
    for i, g in enumerate(gain):   # the render handed the normal values on, so every context holds the plain pack's codes of `want`
        assert_bits(f32[i, 0][normal] * g, want[normal], f"context {i}")
        assert_bits(got[i, :, 0][normal], pcm_model.pack(want[None, :], 1)[:, 0][normal], f"context {i}")
    assert {32767, -32768, 2, 4, -2, -4} <= set(got.ravel().tolist())


@gpu
def test_the_gained_pack_zero_fills_channels_the_destination_does_not_carry(hip):
    audio = pack_source(3, 1, 257)
    ctx = passthrough(hip, audio, n_out=3)
    ctx.destination().set_channel_count(1)
    gain = np.float32([2.0, -0.5, 1e30])
    try:
        f32 = ctx.start_rendering_sync().data
        got = ctx.download_pcm16(gain=gain)
    finally:
        ctx.close()
    assert_bits(got, packed_model(f32, gain, 3), "1 of 3 channels carried")
    assert not got[:, :, 1:].any() and got[:, :, 0].any()


@gpu
def test_the_gained_pack_of_more_contexts_than_grid_rows(hip):
    n = 70000
    rng = np.random.default_rng(70000)
    audio = rng.uniform(-1.2, 1.2, (n, 1, 3)).astype(np.float32)
    gain = gains_for(n, 70)
    ctx = passthrough(hip, audio)
    try:
        f32 = ctx.start_rendering_sync().data
        got = ctx.download_pcm16(gain=gain)
    finally:
        ctx.close()
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        want = pcm_model.pack((f32[:, 0, :] * gain[:, None]).reshape(1, -1), 1).reshape(n, 3, 1)
    assert_bits(got, want, "70 000 contexts")


@gpu
def test_a_non_finite_gain_is_refused(hip):
    ctx = passthrough(hip, pack_source(8, 1, 100))
    try:
        ctx.start_rendering_sync()
        for bad in (np.nan, np.inf, -np.inf):
            gain = np.ones(8, np.float32)
            gain[5] = bad
            with pytest.raises(waa.WaaError, match="instance 5") as e:
                ctx.download_pcm16(gain=gain)
            assert e.value.status == 1
        with pytest.raises(ValueError):
            ctx.download_pcm16(gain=np.ones(7, np.float32))
    finally:
        ctx.close()


@gpu
@pytest.mark.parametrize("async_", [False, True])
def test_normalize_peak(hip, async_):
    n, frames = 6, 128 * 5 + 3
    rng = np.random.default_rng(6)
    audio = (rng.uniform(-1.0, 1.0, (n, 2, frames)) * rng.uniform(0.01, 2.0, (n, 1, 1))).astype(np.float32)
    audio[2] = 0.0             # a silent context keeps gain 1
    audio[4, 1, 77] = np.nan   # not part of the peak
    ctx = passthrough(hip, audio)
    try:
        if async_:
            ctx.render_async()
            f32 = np.empty((n, 2, frames), np.float32)
            hip.check(hip.download_all(ctx._handle, waa.api._fp(f32)))
        else:
            f32 = ctx.start_rendering_sync().data
        levels = ctx.output_levels()
        assert_stats(levels, M.stats(f32), "levels")
        gain = M.normalize_gains(levels["peak"], 0.5)
        assert gain[2] == 1.0 and np.isfinite(gain).all() and (np.delete(gain, 2) != 1.0).all()
        got = ctx.download_pcm16(normalize_peak=0.5)
    finally:
        ctx.close()
    assert_bits(got, packed_model(f32, gain, 2), "normalize_peak=0.5")
    top = np.abs(got.astype(np.int32)).max(axis=(1, 2))
    assert top[2] == 0 and (np.delete(top, 2) >= 16383).all() and (np.delete(top, 2) <= 16385).all()
