"""numpy model of the two conversions at the caller-memory boundary, written from the reference and from the documented packer
contract — not from the project's C (tests/test_caller_boundary.py compares both host resamplers, the device decoder and the
device packer with it, bit for bit).

decode: what the reference makes of decoded 16-bit PCM.  Its decoder converts a sample with symphonia's i16 -> f32 conversion,
`sample / 32768` (decoding.rs:15-54), and AudioBuffer::resample brings the buffer to the context's rate (buffer.rs:311-363):

    if float_eq!(self.sample_rate, sample_rate, abs <= 0.1) { return }        f32 difference, f32 bound
    if self.length() == 0 { return }
    ratio = target_sr as f64 / source_sr as f64
    target_length = (length as f64 * ratio).ceil() as usize
    for i in 0..target_length
        position = i as f64 / (target_length - 1) as f64                      0 / 0 = NaN when target_length == 1
        playhead = position * (source_length - 1) as f64
        prev_index = playhead.floor() as usize                                `as` saturates: NaN -> 0
        next_index = (prev_index + 1).min(source_length - 1)
        k = (playhead - playhead.floor()) as f32;  k_inv = 1. - k             f32
        value = k_inv * prev_sample + k * next_sample                         two f32 products, one f32 sum (Rust never fuses)

pack: the contract of waa_download_all_pcm16 (include/waa_hip.h, waa_decode.hip) — the reference has no such step:
sample * 32768 in f32, clamped to [-32768, 32767] in f32, NaN -> 0, rounded to nearest with ties to even; channels the
rendered signal does not carry are 0.

numpy rounds every f32 array operation to f32 on its own, so nothing here is contracted into a fused multiply-add.
"""
import numpy as np

F32 = np.float32
F64 = np.float64


def will_resample(frames: int, src_sr: float, ctx_sr: float) -> bool:
    return not (np.abs(F32(src_sr) - F32(ctx_sr)) <= F32(0.1) or frames == 0)


def target_length(frames: int, src_sr: float, ctx_sr: float) -> int:
    if not will_resample(frames, src_sr, ctx_sr):
        return int(frames)
    ratio = F64(F32(ctx_sr)) / F64(F32(src_sr))
    return int(np.ceil(F64(frames) * ratio))


def resample(planes, src_sr: float, ctx_sr: float) -> np.ndarray:
    """AudioBuffer::resample for float32[ch, frames] (the part of `decode` behind the sample conversion)"""
    planes = np.asarray(planes)
    assert planes.dtype == np.float32 and planes.ndim == 2
    frames = planes.shape[1]
    if not will_resample(frames, src_sr, ctx_sr):
        return np.ascontiguousarray(planes)
    target = target_length(frames, src_sr, ctx_sr)
    i = np.arange(target, dtype=F64)
    with np.errstate(invalid="ignore", divide="ignore"):
        position = i / F64(target - 1)
        playhead = position * F64(frames - 1)
        floored = np.floor(playhead)
        prev = np.where(np.isnan(floored), 0.0, floored).astype(np.int64)  # `as usize`: NaN -> 0
        nxt = np.minimum(prev + 1, frames - 1)
        k = (playhead - floored).astype(F32)
        k_inv = F32(1.0) - k
        return np.ascontiguousarray(k_inv[None, :] * planes[:, prev] + k[None, :] * planes[:, nxt])


def decode(pcm, src_sr: float, ctx_sr: float) -> np.ndarray:
    """pcm[frames, ch] int16 at src_sr -> float32[ch, target] at ctx_sr"""
    pcm = np.asarray(pcm)
    assert pcm.dtype == np.int16 and pcm.ndim == 2
    planes = np.ascontiguousarray(pcm.T).astype(F32) / F32(32768.0)
    return resample(planes, src_sr, ctx_sr)


def pack(planes, n_out: int) -> np.ndarray:
    """float32[ch, frames] -> int16[frames, n_out]"""
    planes = np.asarray(planes)
    assert planes.dtype == np.float32 and planes.ndim == 2
    ch, frames = planes.shape
    with np.errstate(invalid="ignore", over="ignore"):
        v = planes * F32(32768.0)
        v = np.where(v < F32(-32768.0), F32(-32768.0), np.where(v > F32(32767.0), F32(32767.0), v))
        v = np.where(np.isnan(v), F32(0.0), v)
        codes = np.rint(v)  # round half to even
    assert codes.dtype == np.float32
    out = np.zeros((frames, int(n_out)), np.int16)
    n = min(ch, int(n_out))
    out[:, :n] = codes[:n].T.astype(np.int16)
    return out
