"""The arithmetic of ChannelSplitterNode / ChannelMergerNode restated in numpy f32 (tests/test_channel_routing.py).

ChannelMergerNode (src/node/channel_merger.rs:145-172): every input port has channel count 1, explicit; a connection is mixed to
ONE channel by AudioRenderQuantum::mix (src/render/quantum.rs:285-432) and the connections of a port are added left to right.
With the speakers interpretation the three down-mixes to mono are, each as one expression in the reference's order,

    2 -> 1   0.5 * (l + r)
    4 -> 1   0.25 * (l + r + sl + sr)                       (left to right)
    6 -> 1   sqrt05.mul_add(l + r, 0.5.mul_add(sl + sr, c))  (both multiply-adds FUSED, quantum.rs:428; the LFE is dropped)

every other count — and the discrete interpretation always — keeps channel 0.  A fused multiply-add is computed here in f64 from
f32 operands and rounded once: the products (24 x 24 bits) are exact in f64 and the sum is correct to 2^-53, so the result is
the fma's except in double-rounding ties no test vector relies on (the GPU test bounds these two cases by 1e-6 rel RMS as well).

ChannelSplitterNode (src/node/channel_splitter.rs:183-210): output k is channel k of the input bus (count N, explicit,
discrete: connection c contributes its channels 0 .. min(C, N) - 1), silence beyond."""
import numpy as np

F32 = np.float32
SQRT05 = F32(np.sqrt(F32(0.5)))  # (0.5_f32).sqrt()


def fma32(a, b, c):
    """a * b + c with one rounding, f32 operands"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def down_mix_to_mono(x, interpretation="speakers"):
    """x [channels, frames] f32 -> [frames] f32: AudioRenderQuantum::mix(1, interpretation)"""
    x = np.asarray(x, F32)
    n = x.shape[0]
    if interpretation == "discrete" or n not in (2, 4, 6):
        return x[0].copy()
    if n == 2:
        return F32(0.5) * (x[0] + x[1])
    if n == 4:
        return F32(0.25) * (((x[0] + x[1]) + x[2]) + x[3])
    return fma32(SQRT05, x[0] + x[1], fma32(F32(0.5), x[4] + x[5], x[2]))


def merger_port(connections, interpretation="speakers"):
    """the connections of one input port ([channels, frames] each) -> [frames]: mixed to mono, added left to right in f32"""
    acc = None
    for c in connections:
        m = down_mix_to_mono(c, interpretation)
        acc = m if acc is None else (acc + m).astype(F32)
    return acc


def merger(ports, frames, interpretation="speakers"):
    """ports: per input port a list of connections (empty: unconnected) -> [n_ports, frames]"""
    out = np.zeros((len(ports), frames), F32)
    for k, conns in enumerate(ports):
        if conns:
            out[k] = merger_port(conns, interpretation)
    return out


def splitter(connections, n_outputs, frames):
    """connections ([channels, frames] each) -> [n_outputs, frames]: output k = sum over the connections that have a channel k"""
    out = np.zeros((n_outputs, frames), F32)
    for k in range(n_outputs):
        acc = None
        for c in connections:
            if k < c.shape[0]:
                acc = np.asarray(c[k], F32).copy() if acc is None else (acc + c[k]).astype(F32)
        if acc is not None:
            out[k] = acc
    return out
