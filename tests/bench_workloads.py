"""The table behind tests/test_bench_workloads_full_size.py (-m gpu) and tests/test_bench_workloads_builders.py (CPU): every bench.py
workload that tests/test_full_size_all_instances.py does not already check at its benchmarked size, the route of the launch plan
its test exists to exercise, its max |diff| bound against the oracle, and the oracle's chunked builder of the SAME graph
bench.build_workload times.

bench.build_workload sets a few values by the index and the count of the instances of the context it builds (the oscillator's
detune every n // 64 instances, the per-context HRTF source positions); a chunk lo..hi of the oracle is a context of hi - lo
instances, so `oracle_builder` re-applies the full batch's values of instances lo..hi on top (the fix-ups below).  The CPU test
pins the chunked builder to the unchunked one bit for bit."""
import importlib.util
import os
from dataclasses import dataclass

import numpy as np

import web_audio_api_rs_amd as waa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000.0
FRAMES = 480000  # bench.py's default 10 s at 48 kHz = 3750 render quanta
HRTF_PER_CONTEXT = "WAA_BENCH_HRTF_PER_CONTEXT"  # bench.build_workload reads it: one source position per context


def load_bench():
    """bench.py as a module (it is a script, not part of the package)"""
    spec = importlib.util.spec_from_file_location("waa_bench_workloads_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@dataclass(frozen=True)
class Workload:
    route: str          # a substring of plan_describe() naming the kernel route the test exists to exercise
    max_abs: float      # max |device - oracle| over every sample of every context (see the bounds' comments)
    has_input: bool = True  # False: oscillator graphs, no BufferSource


# Max |diff| bounds.  An f32 output o, rounded from a value both sides compute in f64 to far better than f32 precision, can
# still land on the neighbouring float: one ulp, 2^-23 = 1.2e-7 below magnitude 1, 2^-22 = 2.4e-7 below 2.
ULP_BELOW_2 = 2.0 ** -22
WORKLOADS = {
    # a-rate Biquad (lowpass, cutoff ramp 10 Hz -> 10 kHz): per-frame coefficients from the device's sin / cos / pow (within 1-2
    # ulp of the host libm the oracle uses) and the cutoff ramp itself evaluated on the device; at 10-50 Hz the poles lie within
    # 1e-3 of 1 and the recursion carries a coefficient's last-bit difference for ~1e3 frames with a gain of ~1e3.  The bound of
    # test_c1_a_rate_biquad (tests/test_gpu_parity.py) for the same kernel and the same coefficient arithmetic.
    "c1a": Workload("biquad_lanes(a-rate, shared table", 2e-6),
    # k-rate Biquad (100 Hz -> 8 kHz, one coefficient set per quantum, f64 recursion) -> Gain(0.5): outputs below 2, the
    # coefficients from the device's sin / cos: one output ulp below 2
    "c2k": Workload("biquad_stream(k-rate)", ULP_BELOW_2),
    # IIR scan (Butterworth orders 2-12 at 0.25): the tile scan reassociates the f64 recursion (powers of the transition
    # matrix), orders of magnitude below f32 precision for these well-conditioned filters: one output ulp below 2
    "iir2": Workload("iir_stream states=2", ULP_BELOW_2),
    "iir4": Workload("iir_stream states=4", ULP_BELOW_2),
    "iir8": Workload("iir_stream states=8", ULP_BELOW_2),
    "iir12": Workload("iir_stream states=12", ULP_BELOW_2),
    # order 19: the exact row kernel runs the oracle's operations in the oracle's order (test_iir_exact_kernels_are_bit_identical)
    "iir19": Workload("iir_exact(row) states=19", 0.0),
    # delay lines copy f32 samples, Gain(0.5) is exact, a sum of two f32 terms is one correctly rounded addition on both sides:
    # bit-identical (as test_parity_feedback_delay's loops without a filter)
    "echo": Workload("LDS-ring kernel with nothing fed back", 0.0),
    "fb": Workload("feedback loop: block-scheduled", 0.0),
    "comb": Workload("feedback loop: block-scheduled, 1 tile(s)", 0.0),
    # the same loops with a lowpass Biquad (4 kHz, f64 recursion, f32 output) inside: one ulp per pass of the loop, fed back with
    # gain 0.5 (a geometric series: at most 2 ulp), on outputs below 4 (|dry + 0.5 wet| with a wet peak below 2) — 2 x 2^-21
    "fbq": Workload("block-scheduled, 5 tile(s) = 10240 frames per block, 3 step(s) per block", 2.0 * 2.0 ** -21),
    "pluck": Workload("block-scheduled, 1 tile(s) = 2048 frames per block, 3 step(s) per block", 2.0 * 2.0 ** -21),
    # tremolo: g = 0.6 + 0.4 sin(2 pi 5 t) from the device's closed-form phase (one rounding of the f32 phase: |d sin| <= 2^-24 x
    # 2 pi x 5 / 48000 x frame, 6e-7 at the last frame); the f32 product x g: |x| < 1, 0.4 x 6e-7 + one ulp of the product
    "trem": Workload("LFO: launch 1 (the param's sum", 0.4 * 6e-7 + 2.0 ** -23),
    # sawtooth (time-parallel closed-form phase against the oracle's running sum): isolated samples next to an edge differ by up
    # to 1e-4 (test_parity_fm_long_render's bound), the lowpass Biquad (1.2 kHz, Q 2: impulse response peak < 0.3) and Gain(0.5)
    # scale that down: 1e-4 x 0.3 x 0.5 = 1.5e-5
    "osc": Workload("sawtooth (time-parallel, closed-form phase)", 1.5e-5, has_input=False),
    # FM: the carrier's phase is a prefix sum of frequencies 440 +- 300 Hz against the oracle's running sum over 480 000 frames;
    # the bound of test_parity_fm_long_render (an edge-free sine here)
    "fm": Workload("folded into the carrier's prefix-sum kernel", 1e-4, has_input=False),
    # HRTF: 415 f32 taps per ear as 4 partitions of 256-point f32 transforms against the oracle's direct sum: the transform's
    # rounding (~ sqrt(log2 256) x 6e-8 relative to the sum of |h| |x| over the taps, |h| summing to ~ 10) plus the partition
    # sums: the bound of test_hrtf's transform form against the reference, 2e-5
    "hrtf": Workload("one direction for the whole batch", 2e-5),
}
# the per-context variant of hrtf (HRTF_PER_CONTEXT set): a table of transforms per context
HRTF_PER_CONTEXT_ROUTE = "one direction per context"

# bench workloads whose full-size every-instance test lives in tests/test_full_size_all_instances.py
ELSEWHERE = {
    "c2": "test_c2_every_instance",
    "c3": "test_c3_every_instance_real_ir",
    "c4": "test_c4_every_instance_real_ir_and_every_analyser_pull",
    "c5": "test_c5_every_instance",
    "t1": "test_t1_every_instance_real_ir",
    "os2": "test_oversampled_waveshaper_every_instance",
    "os4": "test_oversampled_waveshaper_every_instance",
}


def _fix_osc(ctx, osc, lo, hi, n_total):
    """bench: detune i % 1200 on every (n // 64)-th instance i of the batch; a chunk's context set it by its own count"""
    step = max(1, n_total // 64)
    for i in range(lo, hi):
        osc.detune.set_value(float(i % 1200) if i % step == 0 else osc.detune.value, instance=i - lo)


def _fix_hrtf(ctx, src, lo, hi, n_total):
    """bench (HRTF_PER_CONTEXT): context i's source at (2 cos 0.37 i, y, 2 sin 0.37 i); a chunk's context counted i from 0"""
    if not os.environ.get(HRTF_PER_CONTEXT):
        return
    pan = next(nd for nd in ctx._nodes if isinstance(nd, waa.PannerNode))
    for i in range(lo, hi):
        pan.position_x.set_value(float(np.cos(0.37 * i) * 2.0), instance=i - lo)
        pan.position_z.set_value(float(np.sin(0.37 * i) * 2.0), instance=i - lo)


FIXUPS = {"osc": _fix_osc, "hrtf": _fix_hrtf}


def oracle_builder(bench, name, noise, n_total, frames):
    """build(binding, lo, hi) -> (ctx, {}): instances lo..hi of bench.build_workload's batch of n_total contexts, input noise[lo:hi]
    (None for the oscillator workloads)"""
    def build(binding, lo, hi):
        ctx, src = bench.build_workload(waa, binding, name, hi - lo, frames, 0, None)
        if noise is not None:
            src.set_buffer_batch(noise[lo:hi], SR)
        fix = FIXUPS.get(name)
        if fix is not None:
            fix(ctx, src, lo, hi, n_total)
        return ctx, {}
    return build
