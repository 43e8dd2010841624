"""The boundary between caller memory and the device — what every batch passes through on the way in and out, whatever its graph:
the transfers of waa_xfer.cpp (pageable memory through the 8 MiB pinned block: a row in pieces, rows in groups, pitched copies;
pinned memory directly), the device's 16-bit PCM decoder (pcm16_resample_kernel) with its host twins (waa_buffer_resample,
orc_buffer_resample), and the PCM packer (pcm16_pack_kernel).

The expected values come from tests/pcm_model.py, a numpy model written from the reference (decoding.rs:15-54,
buffer.rs:311-363) and from the packer's documented contract — not from the project's C.  Every comparison is bit for bit (NaNs
compare equal to NaNs: the payload of 0 / 0 is the machine's); no tolerance is measured anywhere.  The graphs are
BufferSource -> destination, which renders the source's AudioBuffer unchanged and zeros behind it."""
import ctypes as C
import functools

import numpy as np
import pytest

import web_audio_api_rs_amd as waa
import pcm_model

RQ = 128
I16P = C.POINTER(C.c_int16)
STAGE_FLOATS = (8 << 20) // 4   # STAGE_BYTES of waa_xfer.cpp in f32 samples: 2^21


# ----------------------------------------------------------------------------------------------------------------- comparisons
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def assert_bits(got, want, what, nan_ok=False):
    """got == want bit for bit (-0.0 is not +0.0); nan_ok: a NaN equals any NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = _bits(got) != _bits(want)
    if nan_ok:
        bad &= ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        k = tuple(int(v) for v in np.unravel_index(int(np.argmax(bad)), bad.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} elements differ; the first at {k}: got {got[k]!r} "
                             f"(0x{int(_bits(got)[k]):x}), expected {want[k]!r} (0x{int(_bits(want)[k]):x})")


def assert_zero(a, what):
    assert not np.any(_bits(a)), f"{what}: {int(np.count_nonzero(_bits(a)))} elements behind the buffer are not +0.0"


# ------------------------------------------------------------------------------------------------------------ the decode table
PAIRS = [(44100.0, 48000.0), (48000.0, 44100.0), (3000.0, 768000.0), (768000.0, 3000.0)]
LENGTHS = (1, 2, 3, 5)
TARGETS = (1, 2, 255, 256, 257, 511, 512, 513)   # the decoder's 256-thread block edge, one and two blocks
CHANNELS = (1, 2, 3, 6, 32)
# one f32 ulp at 44100 is 0.00390625: 25 ulps above (44100.09765625) lie inside the reference's `abs <= 0.1` window, 26 ulps
# above (44100.1015625) outside it
INSIDE, OUTSIDE = 44100.09765625, 44100.1015625


def frames_for_target(target, src_sr, ctx_sr):
    """the shortest source that resamples to `target` frames, None where the ratio skips that length"""
    guess = int(target * src_sr / ctx_sr)
    for frames in range(max(1, guess - 300), guess + 301):
        if pcm_model.target_length(frames, src_sr, ctx_sr) == target:
            return frames
    return None


def _decode_table():
    shapes = []
    for src_sr, ctx_sr in PAIRS:
        shapes += [(f, src_sr, ctx_sr) for f in LENGTHS]
        shapes += [(f, src_sr, ctx_sr) for f in (frames_for_target(t, src_sr, ctx_sr) for t in TARGETS) if f is not None]
    shapes.append((frames_for_target(70001, 44100.0, 48000.0), 44100.0, 48000.0))
    shapes.append((2, 96000.0, 8000.0))          # target length 1: position = 0 / 0
    for a, b in ((44100.0, INSIDE), (44100.0, OUTSIDE), (INSIDE, 44100.0), (OUTSIDE, 44100.0)):
        shapes += [(513, a, b), (1, a, b)]
    shapes = list(dict.fromkeys(shapes))
    table = [(f, CHANNELS[k % len(CHANNELS)], s, c) for k, (f, s, c) in enumerate(shapes)]
    # every channel count at a two-block target, at the NaN case and at the shortest buffer
    for ch in CHANNELS:
        table += [(frames_for_target(257, 44100.0, 48000.0), ch, 44100.0, 48000.0), (2, ch, 96000.0, 8000.0), (1, ch, 48000.0, 44100.0)]
    return list(dict.fromkeys(table))


DECODE_TABLE = _decode_table()


def _case_id(case):
    frames, ch, src_sr, ctx_sr = case
    return f"{frames}f-{ch}ch-{src_sr:g}-{ctx_sr:.10g}"


def test_the_decode_table_holds_what_it_is_meant_to():
    targets = {(s, c): set() for _, _, s, c in DECODE_TABLE}
    for frames, _, s, c in DECODE_TABLE:
        targets[(s, c)].add(pcm_model.target_length(frames, s, c))
    assert {1, 2, 255, 256, 257, 511, 512, 513} <= targets[(48000.0, 44100.0)]
    assert {1, 2, 255, 256, 257, 511, 512, 513} <= targets[(768000.0, 3000.0)]
    assert {2, 255, 256, 257, 511, 512, 513, 70001} <= targets[(44100.0, 48000.0)]   # (upsampling: no buffer resamples to 1 frame)
    assert {256, 512, 768, 1280} <= targets[(3000.0, 768000.0)]                      # (a ratio of 256: multiples of it only)
    assert targets[(96000.0, 8000.0)] == {1}
    assert targets[(44100.0, INSIDE)] == {513, 1} and targets[(44100.0, OUTSIDE)] == {514, 2}
    assert targets[(INSIDE, 44100.0)] == {513, 1} and targets[(OUTSIDE, 44100.0)] == {513, 1}
    assert pcm_model.will_resample(513, OUTSIDE, 44100.0) and not pcm_model.will_resample(513, INSIDE, 44100.0)
    assert {ch for _, ch, _, _ in DECODE_TABLE} == set(CHANNELS)


def make_pcm(frames, ch, seed):
    """[frames, ch] int16, every channel with its own data; -32768 and 32767 in the first frame, in the last frame and in the
    frame in front of it (the `prev` of the samples whose `next` is clamped to the last frame)"""
    rng = np.random.default_rng([frames, ch, seed])
    pcm = rng.integers(-32768, 32768, (frames, ch), dtype=np.int16)
    lo_hi = np.where(np.arange(ch) % 2 == 0, -32768, 32767).astype(np.int16)
    hi_lo = np.where(np.arange(ch) % 2 == 0, 32767, -32768).astype(np.int16)
    if frames >= 4:
        pcm[-2] = lo_hi
    pcm[0] = lo_hi
    if frames >= 2:
        pcm[-1] = hi_lo
    return pcm


@functools.lru_cache(maxsize=None)
def _case_data(case, n_inst=3):
    """(pcm [n_inst, frames, ch], model planes [n_inst, ch, target]) of a table entry — computed once, never written to"""
    frames, ch, src_sr, ctx_sr = case
    pcm = np.stack([make_pcm(frames, ch, seed) for seed in range(n_inst)])
    want = np.stack([pcm_model.decode(pcm[i], src_sr, ctx_sr) for i in range(n_inst)])
    pcm.setflags(write=False)
    want.setflags(write=False)
    return pcm, want


# ------------------------------------------------------------------------------------------------ CPU: the model, the host twins
def test_model_passes_the_references_own_resample_tests():
    """buffer.rs:736-817 (test_upsample, test_downsample, test_resample_stereo) on the model"""
    up = pcm_model.resample(np.float32([[1, 2, 3, 4, 5]]), 48000.0, 96000.0)
    expected = np.float32(1.0) + np.float32(4.0 / 9.0) * np.arange(10, dtype=np.float32)
    assert up.shape == (1, 10) and np.max(np.abs(up[0] - expected)) <= 1e-6
    down = pcm_model.resample(np.float32([[1, 2, 3, 4, 5]]), 96000.0, 48000.0)
    assert np.array_equal(down, np.float32([[1, 3, 5]]))
    pi = np.float32(np.pi)
    for sr in (22500, 38000, 48000, 96000):
        ph = np.arange(sr, dtype=np.float32) / np.float32(sr) * np.float32(2.0) * pi
        got = pcm_model.resample(np.stack([np.sin(ph), np.cos(ph)]).astype(np.float32), float(sr), 44100.0)
        j = np.arange(44100, dtype=np.float32) / np.float32(44100) * np.float32(2.0) * pi
        assert got.shape == (2, 44100)
        assert np.max(np.abs(got[0] - np.sin(j))) <= 1e-3 and np.max(np.abs(got[1] - np.cos(j))) <= 1e-3
    # the same through the 16-bit front door: a power-of-two scale commutes with every f32 operation of the interpolation
    pcm = np.int16([[1], [2], [3], [4], [5]])
    assert_bits(pcm_model.decode(pcm, 48000.0, 96000.0) * np.float32(32768.0), up, "decode of [1..5] scaled back")
    assert_bits(pcm_model.decode(pcm, 96000.0, 48000.0) * np.float32(32768.0), down, "decode of [1..5] scaled back")


@pytest.mark.parametrize("case", DECODE_TABLE, ids=_case_id)
def test_both_host_resamplers_equal_the_model(hip, orc, case):
    """waa_buffer_resample and orc_buffer_resample are host code: no device is needed for either.  Through waa.resample, and once
    more with a NaN behind every source row and a sentinel either side of every destination row: the last sample's `next` is the
    last frame itself (`.min(source_length - 1)`) — its weight is exactly 0, so only a non-finite neighbour shows a missing clamp"""
    frames, ch, src_sr, ctx_sr = case
    pcm, want = _case_data(case)
    target = pcm_model.target_length(frames, src_sr, ctx_sr)
    planes = np.ascontiguousarray(np.transpose(pcm[0]).astype(np.float32) / np.float32(32768.0))
    guarded = np.full((ch, frames + 1), np.nan, np.float32)
    guarded[:, :frames] = planes
    for name, be in (("waa_buffer_resample", hip), ("orc_buffer_resample", orc)):
        got = waa.resample(be, planes, src_sr, ctx_sr)
        assert got.shape == (ch, target), (name, got.shape)
        assert_bits(got, want[0], f"{name} {_case_id(case)}", nan_ok=True)
        out = np.full((ch, target + 2), 7.0, np.float32)
        for c in range(ch):
            assert be.buffer_resample(waa.api._fp(guarded[c]), frames, src_sr, ctx_sr, waa.api._fp(out[c, 1:]), target) == target
        assert_bits(out[:, 1:-1], want[0], f"{name} {_case_id(case)} (guarded rows)", nan_ok=True)
        assert np.all(out[:, 0] == 7.0) and np.all(out[:, -1] == 7.0), f"{name} wrote outside its {target} frames"


def test_a_target_length_of_one_is_one_nan_from_both_host_resamplers(hip, orc):
    """2 frames at 96 kHz in an 8 kHz context: ceil(2 * 8000 / 96000) = 1 frame, position = 0 / (1 - 1).  The reference casts the
    NaN playhead with `as usize` (0) and emits k_inv * s[0] + k * s[1] with k NaN (buffer.rs:336-351); so does a one-frame buffer
    (NaN * 0 is NaN)"""
    for be in (hip, orc):
        for planes in (np.float32([[0.25, -0.5]]), np.float32([[0.25]])):
            n = be.buffer_resample(waa.api._fp(planes[0]), planes.shape[1], 96000.0, 8000.0, None, 0)
            assert n == 1
            guarded = np.full(3, 7.0, np.float32)
            assert be.buffer_resample(waa.api._fp(planes[0]), planes.shape[1], 96000.0, 8000.0, waa.api._fp(guarded[1:]), 1) == 1
            assert np.isnan(guarded[1]) and guarded[0] == 7.0 and guarded[2] == 7.0
            assert np.isnan(pcm_model.resample(planes, 96000.0, 8000.0)).all()


# --------------------------------------------------------------------------------- decode on the device (and in the oracle)
def _passthrough(be, n_ch, length, sr, n_inst):
    ctx = waa.OfflineAudioContext(n_ch, length, sr, n_instances=n_inst, binding=be)
    src = ctx.create_buffer_source()
    src.connect(ctx.destination())
    src.start()
    return ctx, src


def _render(ctx):
    try:
        return ctx.start_rendering_sync().data
    finally:
        ctx.close()


def _assert_decoded(out, want, what):
    """out [n, ch, length]: the model's planes, zeros behind them"""
    target = want.shape[-1]
    assert_bits(out[..., :target], want, what, nan_ok=True)
    assert_zero(out[..., target:], what)


@pytest.mark.parametrize("case", DECODE_TABLE, ids=_case_id)
def test_set_buffer_pcm16_batch_equals_the_model(be, case):
    frames, ch, src_sr, ctx_sr = case
    pcm, want = _case_data(case)
    ctx, src = _passthrough(be, ch, want.shape[2] + 5, ctx_sr, pcm.shape[0])
    src.set_buffer_pcm16_batch(pcm, src_sr)
    _assert_decoded(_render(ctx), want, f"set_buffer_pcm16_batch {_case_id(case)}")


def _groups():
    """the table by (context rate, channels): one batch each, every instance with its own length and source rate"""
    groups = {}
    for case in DECODE_TABLE:
        groups.setdefault((case[3], case[1]), []).append(case)
    return sorted(groups.items())


@pytest.mark.parametrize("key,cases", _groups(), ids=lambda v: f"{v[0]:.10g}-{v[1]}ch" if isinstance(v, tuple) else None)
def test_set_buffer_pcm16_per_instance_equals_the_model(be, key, cases):
    """set_buffer_pcm16(instance=i): instance i takes table entry i, the last instance what ALL was given"""
    ctx_sr, ch = key
    data = [_case_data(case) for case in cases]
    length = max(want.shape[2] for _, want in data) + 3
    ctx, src = _passthrough(be, ch, length, ctx_sr, len(cases) + 1)
    src.set_buffer_pcm16(data[0][0][1], cases[0][2])   # ALL; overwritten for every instance but the last
    for i, (case, (pcm, _)) in enumerate(zip(cases, data)):
        src.set_buffer_pcm16(pcm[0], case[2], instance=i)
    out = _render(ctx)
    for i, (case, (_, want)) in enumerate(zip(cases, data)):
        _assert_decoded(out[i], want[0], f"set_buffer_pcm16(instance={i}) {_case_id(case)}")
    _assert_decoded(out[-1], data[0][1][1], f"set_buffer_pcm16(ALL) {_case_id(cases[0])}")


CONVOLVER_CASES = [(f, {3: 4, 6: 1, 32: 2}.get(ch, ch), s, c) for f, ch, s, c in DECODE_TABLE
                   if (s, c) in PAIRS[:2] or (s, c) == (96000.0, 8000.0) or INSIDE in (s, c) or OUTSIDE in (s, c)]
CONVOLVER_CASES = [case for case in dict.fromkeys(CONVOLVER_CASES) if case[0] < 1000]


def test_the_convolver_cases_hold_what_they_are_meant_to():
    assert {ch for _, ch, _, _ in CONVOLVER_CASES} == {1, 2, 4}
    targets = {pcm_model.target_length(f, s, c) for f, _, s, c in CONVOLVER_CASES}
    assert {1, 2, 255, 256, 257, 511, 512, 513, 514} <= targets
    # a one-frame response that is not NaN (copied), and the one-frame response that is (resampled)
    assert any(pcm_model.target_length(f, s, c) == 1 and not pcm_model.will_resample(f, s, c) for f, _, s, c in CONVOLVER_CASES)
    assert (2, 1, 96000.0, 8000.0) in CONVOLVER_CASES


@pytest.mark.parametrize("case", CONVOLVER_CASES, ids=_case_id)
def test_convolver_set_buffer_pcm16_equals_set_buffer_of_the_model(be, case):
    """ConvolverNode.set_buffer_pcm16 against set_buffer of the model's planes: the same render, bit for bit"""
    frames, ch, src_sr, ctx_sr = case
    pcm, want = _case_data(case)
    n_inst, length = 2, RQ * 6 + 37
    rng = np.random.default_rng(11)
    noise = rng.uniform(-1.0, 1.0, (n_inst, 2, length)).astype(np.float32)
    outs = []
    for use_pcm in (True, False):
        ctx = waa.OfflineAudioContext(2, length, ctx_sr, n_instances=n_inst, binding=be)
        src = ctx.create_buffer_source()
        src.set_buffer_batch(noise, ctx_sr)
        conv = ctx.create_convolver()
        if use_pcm:
            conv.set_buffer_pcm16(pcm[0], src_sr)
        else:
            conv.set_buffer(waa.AudioBuffer(want[0], ctx_sr))
        src.connect(conv).connect(ctx.destination())
        src.start()
        outs.append(_render(ctx))
    assert_bits(outs[0], outs[1], f"convolver {_case_id(case)}", nan_ok=True)
    if np.isnan(want[0]).any():
        assert np.isnan(outs[0]).any()
    else:
        assert float(np.abs(outs[0]).max()) > 1e-3


@pytest.mark.gpu
def test_decode_of_more_contexts_than_grid_rows(hip):
    """70 000 contexts x 5 frames, mono, 44100 -> 48000: the decoder puts the context on gridDim.y (65535 rows at most) and
    walks the rest with `item += gridDim.y`"""
    n, frames = 70000, 5
    rng = np.random.default_rng(5)
    pcm = rng.integers(-32768, 32768, (n, frames, 1), dtype=np.int16)
    pcm[[0, -1, 65534, 65535, 65536], 0, 0] = [-32768, 32767, -32768, 32767, -32768]
    # one resample of a 70 000-channel buffer: the contexts share length and rates, so a context is a channel of the model
    want = pcm_model.decode(np.ascontiguousarray(pcm[:, :, 0].T), 44100.0, 48000.0)
    assert want.shape == (n, 6)
    ctx, src = _passthrough(hip, 1, 8, 48000.0, n)
    src.set_buffer_pcm16_batch(pcm, 44100.0)
    out = _render(ctx)
    for i in (0, 1, 65534, 65535, 65536, 65537, n - 1):
        assert_bits(out[i, 0, :6], pcm_model.decode(pcm[i], 44100.0, 48000.0)[0], f"context {i}")
    assert_bits(out[:, 0, :6], want, "70 000 contexts")
    assert_zero(out[:, :, 6:], "70 000 contexts")


# ------------------------------------------------------------------------------------------------------------- the pack table
def _f32(x):
    return np.float32(x)


TIES = [(k + 0.5) / 32768.0 for k in (0, 1, 2, 3, 100, 101, 32765, 32766, -1, -2, -3, -4, -101, -102, -32767, -32768)]
SPECIALS = np.array(
    TIES
    + [1.0, -1.0, 32767.5 / 32768.0, -32768.5 / 32768.0, 4.0, -4.0, np.inf, -np.inf]   # the saturation edges
    + [np.nan, 0.0, -0.0, 1e-40, -1e-40, 1e-6, -1e-6]
    # one ulp either side of a tie, and of the two saturation edges: not ties
    + [float(np.nextafter(_f32(2.5 / 32768.0), _f32(1.0))), float(np.nextafter(_f32(2.5 / 32768.0), _f32(0.0))),
       float(np.nextafter(_f32(-3.5 / 32768.0), _f32(-1.0))), float(np.nextafter(_f32(-3.5 / 32768.0), _f32(0.0))),
       float(np.nextafter(_f32(32767.0 / 32768.0), _f32(0.0))), float(np.nextafter(_f32(-1.0), _f32(-2.0)))],
    dtype=np.float32)
# what the contract makes of them
SPECIAL_CODES = np.int16([0, 2, 2, 4, 100, 102, 32766, 32766, -0, -2, -2, -4, -100, -102, -32766, -32768]
                         + [32767, -32768, 32767, -32768, 32767, -32768, 32767, -32768]
                         + [0, 0, 0, 0, 0, 0, 0]
                         + [3, 2, -4, -3, 32767, -32768])


def test_the_model_packs_the_special_values_as_the_contract_says():
    """written out by hand from the contract (x 32768, clamp to [-32768, 32767], NaN -> 0, nearest, ties to even)"""
    assert SPECIALS.size == SPECIAL_CODES.size
    for v in TIES:
        assert float(_f32(v)) == v   # (k + 0.5) / 32768 is exact in f32: these are ties, not near-ties
    assert np.array_equal(pcm_model.pack(SPECIALS[None, :], 1)[:, 0], SPECIAL_CODES)
    assert np.array_equal(pcm_model.pack(SPECIALS[None, :], 3), np.stack([SPECIAL_CODES, 0 * SPECIAL_CODES, 0 * SPECIAL_CODES], axis=1))


def pack_source(n_inst, n_ch, frames):
    """noise in [-1.2, 1.2) with the special values at both ends of every plane, in another rotation for every plane"""
    rng = np.random.default_rng([n_inst, n_ch, frames])
    x = rng.uniform(-1.2, 1.2, (n_inst, n_ch, frames)).astype(np.float32)
    s = SPECIALS.size
    assert frames >= 2 * s
    for i in range(n_inst):
        for c in range(n_ch):
            x[i, c, :s] = np.roll(SPECIALS, 7 * i + 3 * c)
            x[i, c, -s:] = np.roll(SPECIALS[::-1], 5 * i + 2 * c)
    return x


def assert_handed_on(be, f32, x, what):
    """What the pass-through hands on to the download.  The oracle copies every bit pattern.  The device library renders with f32
    denormals flushed (its kernels are built that way: the reference renders under FTZ + DAZ), and which kernel carries a source
    to the destination depends on the graph: with 1 and 2 channels a subnormal and -0.0 arrive as +0.0, with 6 channels they
    arrive unchanged (a finding of this test, recorded here; all of them pack to code 0 either way).  So a sample below the
    smallest normal may arrive as it was or as +0.0 from the device library; everything else — the ties, the saturation edges,
    +-inf, NaN, +-1e-6 — arrives unchanged from both."""
    expected = x
    if be.prefix == "waa_":
        flushed = (np.abs(x) < np.finfo(np.float32).tiny) & (_bits(f32) == 0)
        expected = np.where(flushed, np.float32(0.0), x)
    assert_bits(f32, expected, what, nan_ok=True)


def _download_f32_and_pcm16(ctx):
    b, h = ctx._b, ctx._handle
    f32 = np.empty((ctx.n_instances, ctx.number_of_channels, ctx.length), np.float32)
    b.check(b.download_all(h, waa.api._fp(f32)))
    pcm = np.full((ctx.n_instances, ctx.length, ctx.number_of_channels), 0x5A5A, np.int16)
    b.check(b.download_all_pcm16(h, pcm.ctypes.data_as(I16P)))
    return f32, pcm


def _assert_packed(f32, pcm, n_out, what):
    for i in range(f32.shape[0]):
        assert_bits(pcm[i], pcm_model.pack(f32[i], n_out), f"{what}, context {i}")


@pytest.mark.parametrize("n_out", [1, 2, 6])
@pytest.mark.parametrize("frames", [255, 256, 257])
def test_download_all_pcm16_equals_the_model_on_the_batchs_own_f32_download(be, frames, n_out):
    """The packer against the model applied to the SAME batch's f32 download: the render's rounding is not part of the test.
    What the pass-through hands on is asserted first (assert_handed_on); the expectation follows the f32 download."""
    n_inst = 3
    x = pack_source(n_inst, n_out, frames)
    ctx, src = _passthrough(be, n_out, frames, 48000.0, n_inst)
    src.set_buffer_batch(x, 48000.0)
    try:
        ctx.render_async()
        f32, pcm = _download_f32_and_pcm16(ctx)
    finally:
        ctx.close()
    assert_handed_on(be, f32, x, f"the f32 download of the pass-through ({frames} frames, {n_out} channels)")
    assert np.isnan(f32).sum() == 2 * n_inst * n_out and np.isinf(f32).sum() == 4 * n_inst * n_out
    _assert_packed(f32, pcm, n_out, f"download_all_pcm16 ({frames} frames, {n_out} channels)")


@pytest.mark.parametrize("n_out", [2, 6])
def test_download_all_pcm16_zero_fills_the_channels_the_destination_does_not_carry(be, n_out):
    """A destination whose channelCount was set below the context's (AudioDestinationNode::set_channel_count allows any count up
    to max_channel_count): its signal has one channel, the AudioBuffers have n_out.  waa_download_all takes its per-channel branch
    (s.nch != n_out: channels >= nch are memset), the packer its `c >= nch_in` arm."""
    n_inst, frames = 3, 257
    x = pack_source(n_inst, 1, frames)
    ctx, src = _passthrough(be, n_out, frames, 48000.0, n_inst)
    ctx.destination().set_channel_count(1)
    src.set_buffer_batch(x, 48000.0)
    try:
        ctx.render_async()
        f32, pcm = _download_f32_and_pcm16(ctx)
    finally:
        ctx.close()
    assert_handed_on(be, f32[:, :1], x, "channel 0 of the f32 download")
    assert_zero(f32[:, 1:], "channels 1.. of the f32 download")
    _assert_packed(f32, pcm, n_out, f"download_all_pcm16 (1 of {n_out} channels carried)")
    assert_zero(pcm[:, :, 1:], "channels 1.. of the PCM download")
    assert np.abs(pcm[:, :, 0].astype(np.int32)).max() == 32768


# ------------------------------------------------------------------------------------------------------ the staging block's edges
# (contexts, channels, frames per row): a row is one channel of one context
STAGING_SHAPES = [
    (1, 1, STAGE_FLOATS - 1),   # one float short of the block; not a multiple of 4: the device stride differs, a pitched copy
    (1, 1, STAGE_FLOATS),       # exactly the block
    (1, 1, STAGE_FLOATS + 1),   # a row longer than the block: in pieces (8 MiB, then 4 bytes)
    (3, 1, 699051),             # 2 rows fit the block, the third is a ragged last group; 699051 = 4 * 174762 + 3: pitched
    (2, 2, 1 << 20),            # 4 rows of 4 MiB: two full groups, nothing left over; stride == width: plain copies
]
TAIL = 5


def _allocator(pinned):
    """numpy arrays in pageable memory, or views of page-locked torch tensors (what a host that cares about the link hands over)"""
    if not pinned:
        return lambda shape, dtype: np.empty(shape, dtype)
    import torch
    kinds = {np.float32: torch.float32, np.int16: torch.int16}
    return lambda shape, dtype: torch.empty(tuple(shape), dtype=kinds[dtype], pin_memory=True).numpy()


def _filled(alloc, shape, seed):
    a = alloc(shape, np.float32)
    a[...] = np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)
    a[..., 0], a[..., -1] = 0.75, -0.625   # (a row's first and last sample: what a dropped piece or group would lose)
    return a


def _assert_passed_through(out, audio, what):
    frames = audio.shape[-1]
    assert_bits(out[..., :frames], audio, what)
    assert_zero(out[..., frames:], what)


def staging_round_trip_f32(be, alloc, n_inst, n_ch, frames, length):
    """f32 in through set_buffer_batch, the refill of a re-armed batch and set_buffer; out through waa_download_all and
    waa_download.  Every buffer the library reads or writes comes from `alloc`."""
    fp = waa.api._fp
    first, second = _filled(alloc, (n_inst, n_ch, frames), 1), _filled(alloc, (n_inst, n_ch, frames), 2)
    ctx, src = _passthrough(be, n_ch, length, 48000.0, n_inst)
    try:
        src.set_buffer_batch(first, 48000.0)
        ctx.render_async()
        b, h = ctx._b, ctx._handle
        out = alloc((n_inst, n_ch, length), np.float32)
        out.fill(np.nan)
        b.check(b.download_all(h, fp(out)))
        _assert_passed_through(out, first, "set_buffer_batch -> download_all")
        b.check(b.batch_rearm(h))
        b.check(b.source_set_buffer_batch(h, src.id, fp(second), n_ch, frames, 48000.0))
        b.check(b.render(h))
        out.fill(np.nan)
        for i in range(n_inst):
            for c in range(n_ch):
                b.check(b.download(h, i, c, fp(out[i, c]), length))
        _assert_passed_through(out, second, "refill of the re-armed batch -> download")
    finally:
        ctx.close()
    ctx, src = _passthrough(be, n_ch, length, 48000.0, n_inst)
    try:
        for i in range(n_inst):
            src.set_buffer(waa.AudioBuffer(second[i], 48000.0), instance=i)
        ctx.render_async()
        out.fill(np.nan)
        ctx._b.check(ctx._b.download_all(ctx._handle, fp(out)))
        _assert_passed_through(out, second, "set_buffer -> download_all")
    finally:
        ctx.close()


def staging_round_trip_pcm16(be, alloc, n_inst, frames, length):
    """16-bit PCM in (batch setter, and the refill of a re-armed batch) at the context's rate, 16-bit PCM out: k / 32768 is exact
    in f32 and packs back to k"""
    def pcm_of(seed):
        a = alloc((n_inst, frames, 1), np.int16)
        a[...] = np.random.default_rng(seed).integers(-32768, 32768, a.shape, dtype=np.int16)
        a[:, 0, 0], a[:, -1, 0] = -32768, 32767
        return a
    first, second = pcm_of(1), pcm_of(2)
    ctx, src = _passthrough(be, 1, length, 48000.0, n_inst)
    try:
        src.set_buffer_pcm16_batch(first, 48000.0)
        ctx.render_async()
        b, h = ctx._b, ctx._handle
        out = alloc((n_inst, length, 1), np.int16)
        for audio in (first, second):
            if audio is second:
                b.check(b.batch_rearm(h))
                b.check(b.source_set_buffer_pcm16_batch(h, src.id, audio.ctypes.data_as(I16P), 1, frames, 48000.0))
                b.check(b.render(h))
            out.fill(0x5A5A)
            b.check(b.download_all_pcm16(h, out.ctypes.data_as(I16P)))
            assert_bits(out[:, :frames], audio, "PCM in -> PCM out")
            assert_zero(out[:, frames:], "PCM in -> PCM out")
    finally:
        ctx.close()


def _staging_id(v):
    return f"{v[0]}x{v[1]}x{v[2]}" if isinstance(v, tuple) else None


@pytest.mark.gpu
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("edge", ["upload", "download"])
@pytest.mark.parametrize("shape", STAGING_SHAPES, ids=_staging_id)
def test_f32_transfers_at_the_staging_blocks_edges(hip, shape, edge, pinned):
    """edge = upload: the source's rows have the table's length (and the render is 5 frames longer: zeros behind the buffer);
    edge = download: the rendered rows have it (and the source is 5 frames shorter).  Pageable and pinned caller memory are both
    compared with the caller's own input, so the two paths give identical bytes."""
    n_inst, n_ch, size = shape
    frames, length = (size, size + TAIL) if edge == "upload" else (size - TAIL, size)
    staging_round_trip_f32(hip, _allocator(pinned), n_inst, n_ch, frames, length)


@pytest.mark.gpu
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_pcm16_transfers_just_above_the_staging_block(hip, pinned):
    """2 contexts x 2 200 000 mono frames: 8.8 MB of interleaved PCM in one row, both ways — a block and a 411 392-byte piece"""
    staging_round_trip_pcm16(hip, _allocator(pinned), 2, 2_200_000, 2_200_000 + 7)
