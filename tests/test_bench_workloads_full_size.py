"""Every bench.py workload not covered by tests/test_full_size_all_instances.py, at the size the bench renders it: bench defaults
(DEFAULT_INSTANCES, else 1024 contexts) x 10 s, EVERY context against the oracle, on the re-rendered step (-m gpu).

The graphs are bench.build_workload's own, fed as the bench feeds them: a caller-owned torch device tensor adopted by the
BufferSource (adopt_device_buffer).  The batch is rendered once (the bench's planning step) and downloaded, then rendered again
— what every timed step of the bench is — and the second render must equal the first bit for bit (every piece of state a kernel
carries across the render must be reset in front of a render).  The second render is then compared with the oracle for every
(instance, channel) row: 1e-6 RMS per channel and the workload's max |diff| bound (tests/bench_workloads.py), and one route of
its launch plan is asserted, so that a change of route cannot retire the coverage quietly.  The oracle's chunked builder of the
same graph is pinned to bench.build_workload on the CPU (tests/test_bench_workloads_builders.py).

The a-rate Biquad (c1a: the worst-conditioned graph, seconds at 10-50 Hz with poles near 1) is also tested past the bench graph:
four filter types, 100 contexts (200 streams: three full 64-lane groups and a partial one), per-instance start and stop times
inside quanta (sources that stop ring the filter down to its flush), a cutoff held at 10 Hz, and one instance with its own
detune block (the per-instance coefficient path)."""
import numpy as np
import pytest

import web_audio_api_rs_amd as waa
from bench_workloads import FRAMES, HRTF_PER_CONTEXT, HRTF_PER_CONTEXT_ROUTE, SR, WORKLOADS, load_bench, oracle_builder
from every_instance import _compare_all, _rerender_bit_identical

pytestmark = pytest.mark.gpu
RQ = 128


@pytest.fixture(scope="module")
def bench():
    return load_bench()


def _device_noise(torch, n_inst, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return torch.empty((n_inst, 2, FRAMES), dtype=torch.float32, device="cuda").uniform_(-1.0, 1.0, generator=gen)


def _render_twice(ctx):
    """first render (downloaded), second render bit-identical to it; returns the second"""
    ctx.prepare()
    ctx.render_async()
    ctx.sync()
    out = np.empty((ctx.n_instances, ctx.number_of_channels, ctx.length), np.float32)
    ctx._b.check(ctx._b.download_all(ctx._handle, out.ctypes.data_as(waa.api._FP)))
    _rerender_bit_identical(ctx, out)
    return out


@pytest.mark.parametrize("name,per_context", [(n, False) for n in sorted(WORKLOADS)] + [("hrtf", True)])
def test_bench_workload_every_instance_rerendered(hip, orc, bench, name, per_context, monkeypatch):
    import torch
    if per_context:
        monkeypatch.setenv(HRTF_PER_CONTEXT, "1")
    else:
        monkeypatch.delenv(HRTF_PER_CONTEXT, raising=False)
    w = WORKLOADS[name]
    n_inst = bench.DEFAULT_INSTANCES.get(name, 1024)
    noise = _device_noise(torch, n_inst, 0xB0E + len(name)) if w.has_input else None
    ctx, _ = bench.build_workload(waa, hip, name, n_inst, FRAMES, 0, None if noise is None else noise.data_ptr())
    out = _render_twice(ctx)
    plan = ctx.plan_describe()
    ctx.close()
    host_noise = None
    if noise is not None:
        host_noise = noise.cpu().numpy()
        del noise
        torch.cuda.empty_cache()
    route = HRTF_PER_CONTEXT_ROUTE if per_context else w.route
    assert route in plan, plan
    build = oracle_builder(bench, name, host_noise, n_inst, FRAMES)
    _compare_all(orc, out, build, chunk=128, max_abs=w.max_abs)


C1A_TYPES = ["lowpass", "peaking", "highshelf", "bandpass"]


def _c1a_edges(binding, lo, hi, ftype, hold, own_detune, feed, device=0):
    """BufferSource -> Biquad(ftype, gain 6 dB) -> destination, 10 s; cutoff 10 Hz -> 10 kHz (exponential) or held at 10 Hz;
    context i starts inside quantum i % 9 and every third one stops between 3 and 9.4 s, inside a quantum"""
    ctx = waa.OfflineAudioContext(2, FRAMES, SR, n_instances=hi - lo, binding=binding, device=device)
    src = ctx.create_buffer_source()
    feed(src, lo, hi)
    bq = ctx.create_biquad_filter(type_=ftype, frequency=200.0, q=1.0, gain=6.0)
    bq.frequency.set_value_at_time(10.0, 0.0)
    if not hold:
        bq.frequency.exponential_ramp_to_value_at_time(10000.0, FRAMES / SR)
    for i in range(lo, hi):
        src.start_at(((i % 9) * RQ + 37 + (i % 5) * 13) / SR, instance=i - lo)
        if i % 3 == 1:
            src.stop_at(3.0 + (i % 11) * 0.58 + 61.0 / SR, instance=i - lo)
    if own_detune is not None and lo <= own_detune < hi:
        bq.detune.set_block(700, np.linspace(-1200.0, 1200.0, 1500 * RQ).astype(np.float32).reshape(1500, RQ),
                            instance=own_detune - lo)
    src.connect(bq).connect(ctx.destination())
    return ctx, {}


@pytest.mark.parametrize("ftype", C1A_TYPES)
@pytest.mark.parametrize("variant", ["ramp", "hold_10hz", "own_detune"])
def test_c1a_edges_every_instance_rerendered(hip, orc, ftype, variant):
    import torch
    n_inst = 100
    hold, own = variant == "hold_10hz", (37 if variant == "own_detune" else None)
    noise = _device_noise(torch, n_inst, 0xC1A)
    ctx, _ = _c1a_edges(hip, 0, n_inst, ftype, hold, own,
                        lambda src, lo, hi: src.adopt_device_buffer(noise.data_ptr(), 2, FRAMES, SR))
    out = _render_twice(ctx)
    plan = ctx.plan_describe()
    ctx.close()
    host_noise = noise.cpu().numpy()
    del noise
    # one table of per-frame coefficients for the whole batch: the lane kernel; a context with its own detune block: the
    # per-instance coefficient table of the streaming kernel
    route = "biquad_stream(a-rate, per-instance table)" if own is not None else "biquad_lanes(a-rate, shared table"
    assert route in plan, plan
    # (the same arithmetic as bench's c1a — see WORKLOADS["c1a"] — on outputs up to 2x larger: the 6 dB peaking / shelf gain)
    _compare_all(orc, out, lambda be, lo, hi: _c1a_edges(be, lo, hi, ftype, hold, own,
                                                        lambda src, lo_, hi_: src.set_buffer_batch(host_noise[lo_:hi_], SR)),
                 chunk=100, max_abs=2.0 * WORKLOADS["c1a"].max_abs)
