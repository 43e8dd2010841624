"""Every launch kind at the batch sizes where its grid changes.

Every kernel places the context index somewhere in its grid: one workgroup (or wavefront) per context or stream, 64 contexts per
wavefront, or the context / stream / context pair on gridDim.y or gridDim.z.  The table below names, for every StepKind of
waa_host.hpp (KIND_NAMES of tests/test_launch_list.py), the launcher's mapping as read from its launch_* function and the planner's
thresholds, and the batch sizes at which that mapping changes; the graphs (tests/batch_graphs.py) give every context its own audio
and, where the kind has one, its own value.

gridDim.y / gridDim.z: hipDeviceProp_t::maxGridSize of the MI355X (gfx950, ROCm 7.2) reads (2147483647, 65536, 65536) — one row
more than the 65535 the project had on record (and CUDA has); test_row_limit_of_the_device reads it.  The launchers that carry the
batch there launch a batch of more than MAX_GRID_ROWS = 65535 rows (waa_internal.hpp: the recorded limit, which fits either) in
slices; ROW_LIMIT lists them with batches that cross both figures.  (Measured with these tests on the parent commit's build: this
runtime ACCEPTS grids of 65537 and more rows in y and z and the unsliced launches render the same batches correctly — the figure
it reports is not enforced at launch, where the runtime of the PCM packer's record refused 70 000 rows.  The slices keep every
launch inside the reported limit rather than rely on that.)

StepKind            mapping of the batch (launcher)                                                     sizes, and why
chain               (waves + 3) / 4 workgroups, 8 wavefronts per context and tile (launch_chain);       1 2 3: a context always fills whole workgroups,
                    the feed-forward echo: one workgroup per context from 256 contexts on                no straddle exists; 255 256 257: WAA_ECHO_FF_MIN_INST
                    (waa_plan_loops.cpp, "one per CU"), the tile-parallel launch below;
                    source [-> WaveShaper] -> signal (launch_resample, the chain step's own kernel):    1 7 8 9 31 32 33: the ragged last wavefront of 8
                    8 contexts per wavefront, 4 wavefronts per workgroup                                contexts, one workgroup (of one sub-tile) +- 1
biquad_stream       one wavefront per stream, n_inst * nch workgroups (launch_biquad_stream); the        1 3: no batch-dependent rule
                    chained scan and its biquad_scan_powers ((n + 63) / 64) are opt-in (WAA_BIQUAD_SCAN,
                    a measurement switch): not rendered here
conv_fft            pair p = contexts 2p, 2p + 1 in one transform, pairs on gridDim.z (forward,          1 3 65: the last pair has one member; 2: full pair;
                    inverse), pair * cout on gridDim.y (products); n = 16384: a workgroup walks all     1022 1024 1025 mono, two blocks (8325 frames): 511 / 512 /
                    blocks of a stream from 512 streams on, a part of them below (f3_blocks_per_wg;     513 streams, one block / both blocks per workgroup;
                    with one block per stream, as in the 2181-frame graphs, always that one)            131073 mono, 65537 stereo: past the row limit
zero_fill           hipMemsetAsync of the node's whole signal                                           no grid: 1 3
conv_direct         context on gridDim.z (launch_conv_direct, launch_conv_inst_direct)                  1 3; 65537: past the row limit
biquad_coefs        rows * frames / 256 workgroups, rows = 1 for a shared table                         no batch-dependent mapping (shared table): 1 3
iir_stream          one wavefront per stream (iir_stream_kernel); the exact forms of an                 1 2 3 (2 .. 6 streams)
                    ill-conditioned filter — 4 streams per workgroup, 64 per wavefront — are not
                    rendered here: tests/test_iir_per_instance.py holds them bit for bit per context
                    at 7 and 70 contexts (a ragged last workgroup and wavefront)
delay               stream = context * nch + channel on gridDim.y (launch_delay)                        1 2 3 65; 32769 stereo, 65537 mono: past the row limit
loop                one wavefront per context (launch_loop), one workgroup per context                  1 3: no batch-dependent rule
                    (launch_echo_ring)
osc                 time-parallel forms: context on gridDim.y (osc_par_kernel, osc_par_lds_kernel,      1 3 (2 3 where the value per context makes the form);
                    osc_types_par_kernel); prefix-sum: context on gridDim.x; serial form                65537: past the row limit
                    ((n + 63) / 64, WAA_OSC_EXACT) is a measurement switch
dyn                 n_inst * q_split workgroups; q_split = min(max(16384 / n_inst, 16), quanta / 6)     1 3 65 in a quantum-blocked loop (q_split 1); 512 513 at
                    (launch_dyn; stateless groups only): the batch enters above 96 quanta per launch    193 quanta outside a loop: q_split 32 / 31
conv_codes          (n_inst + 63) / 64 wavefronts, lane = context                                       1 3 65
biquad_hp           one workgroup per tile                                                              no batch-dependent mapping: 31 32 33 (with the lanes)
panner_geom         rows * frames / 256, rows = 1 (listener automation is one table)                    no batch-dependent mapping: 1 3
timeline            (rows + 63) / 64 wavefronts, lane = one (context, param) row                        1 63 64 65 (device only: a plan-only batch replays on the host)
link                (n_inst + 63) / 64 wavefronts, lane = context (dynamic plans only: a static         1 3 65 (in a quantum-blocked loop)
                    plan computes the table on the host)
qgemm               context * nch on gridDim.z (launch_qgemm; WAA_OS_MATRIX, measurement build)         refused at plan time past the row limit: tested
hrtf                transform form: 16 runs = one workgroup, a context's runs padded to 16s;            1 2 3; direct forms 1 3; 65537: past the row limit
                    direct forms (under 16 quanta per launch, or a moving direction): context on
                    gridDim.y (hrtf8_kernel, hrtf_kernel); one profile slot for the three, the
                    device's plan text says which the render takes
biquad_tile_digest  one workgroup per tile                                                              no batch-dependent mapping: 31 32 33 (with the lanes)
biquad_lanes        64 streams per wavefront: (n_inst * nch + 63) / 64 groups per tile                  31 32 33 (62 64 66 streams), 1
os_fft              16 runs per workgroup, n_inst * n_seg runs (launch_osfft); 3 runs per context       1 5 6 11: 15 / 18 runs, a workgroup holds two contexts' runs
                    here
compressor          level, apply: context on gridDim.y; detector: 64 contexts per wavefront             1 63 64 65; 65537: past the row limit
route               frames / 2048 * rows * n_inst workgroups                                            1 3: no batch-dependent rule
"""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

import batch_graphs as G
import compressor_model as cm
import web_audio_api_rs_amd as waa
from every_instance import usable_cpus
from graphs import assert_all_finite, assert_le, rms_err, strict_max
from rearm import first_difference, refill_from, render_again
from source_schedules import ran
from test_launch_list import KIND_NAMES

RQ, SR = G.RQ, G.SR

# the bound of the kind's existing parity test: RMS per (context, channel), max |diff|; scaled: both times max(1, |oracle| max);
# bits: bit equality
Bound = namedtuple("Bound", "test rms max_abs scaled bits", defaults=(False, False))
CONV = Bound("tests/test_gpu_parity.py::test_t1_small_multi_partition", 1e-6, 2e-6)
CONV_INST = Bound("tests/test_convolver_per_instance.py::test_every_path_odd_and_even_batches", 1e-6, 2e-6)
OSC = Bound("tests/test_oscillator.py::test_parity_long_render_closed_form_phase", 1e-6, 2e-5)
HRTF = Bound("tests/test_hrtf.py::test_hrtf_many_instances_sampled", 1e-6, np.inf)
FROZEN_LOOP = Bound("tests/test_frozen_loops.py::test_echo_with_a_frozen_state_node_in_the_loop", 1e-6, 2e-5, True)

# name -> builder, the StepKinds it is in the table for, bound, batch sizes (stereo unless the builder is mono by nature), the
# profile slots that must have run (a function of the size where the size decides), phrases of the plan text (same), the size of
# the neighbour test; chunk: contexts per oracle batch (1: the oracle keeps one value per batch where the device has one per
# context); pair: contexts 2p, 2p + 1 share a transform; kw: mono / frames of the row's batches; device_plan: phrases of the plan
# text of the batch on the DEVICE (what a plan-only batch cannot say)
Row = namedtuple("Row", "build kinds bound sizes slots plan edge chunk pair kw device_plan", defaults=(None, False, {}, ()))


def _ff_slots(n):
    return ("echo_ring_kernel",) if n >= 256 else ("chain_kernel",)


def _ff_plan(n):
    return (("+", "LDS-ring kernel with nothing fed back"),) if n >= 256 else (("-", "LDS-ring kernel"),)


TABLE = {
    "gain": Row(G.b_gain, ("chain",), Bound("tests/test_gpu_parity.py::test_gain_fast_paths", 0.0, 0.0, bits=True), (1, 2, 3),
                ("chain_kernel",), ("chain parallel C=2 in=[source:2ch]->2ch ops=[GAIN]",), 3),
    "feed_forward_echo": Row(G.b_feed_forward_echo, ("chain",),
                             Bound("tests/test_delay.py::test_parity_feed_forward_echo_out_of_the_ring", 0.0, 0.0, bits=True), (3, 255, 256, 257),
                             _ff_slots, _ff_plan, 257),
    "resample_plain": Row(G.b_resample_plain, ("chain",), Bound("tests/test_gpu_parity.py::test_c5_small", 1e-6, 1e-6), (1, 7, 8, 9, 31, 32, 33),
                          ("resample_kernel",), ("chain parallel C=2 in=[source:2ch]->2ch ops=[] out=2ch", ("-", "in place")), 9),
    "resample_shaper": Row(G.b_resample_shaper, ("chain",), Bound("tests/test_gpu_parity.py::test_c5_small", 1e-6, 1e-6), (1, 7, 8, 9, 31, 32, 33),
                           ("resample_kernel",), ("chain parallel C=2 in=[source:2ch]->2ch ops=[WAVESHAPER] out=2ch",), 33),
    "c2": Row(G.b_c2, ("biquad_stream",), Bound("tests/test_gpu_parity.py::test_c2_small", 1e-6, 1e-7), (1, 3),
              ("biquad_stream_kernel",), ("biquad_stream in=source:2ch",), 3),
    "biquad_k_rate": Row(G.b_biquad_k_rate, ("biquad_stream",), Bound("tests/test_gpu_parity.py::test_k_rate_biquad_streaming_kernel", 1e-6, 1e-6),
                         (1, 3), ("biquad_stream_kernel",), ("biquad_stream(k-rate)",), 3),
    "biquad_a_rate_shared": Row(G.b_biquad_a_rate_shared, ("biquad_coefs", "biquad_hp", "biquad_tile_digest", "biquad_lanes"),
                                Bound("tests/test_gpu_parity.py::test_c1_a_rate_biquad", 1e-6, 2e-6), (1, 31, 32, 33),
                                ("biquad_coef_kernel", "biquad_tile_digest_kernel", "biquad_lanes_kernel"),
                                ("biquad_lanes(a-rate, shared table: one lane per stream, tiles in parallel)",), 33),
    "iir": Row(G.b_iir, ("iir_stream",), Bound("tests/test_iir_per_instance.py::test_scan_kernel_each_instance_its_own_order", 1e-6, 1e-6, True),
               (1, 2, 3), ("iir_stream_kernel",), ("iir_stream states=2",), 3, 1),
    "delay_gather": Row(G.b_delay_gather, ("delay", "conv_fft", "chain"), CONV, (1, 2, 3, 65), ("delay_kernel", "conv_fft_kernel<fwd>"),
                        ("delay node 1: 2ch delayTime=const", "fft B=128 N=256"), 65, None, True),
    "conv_direct": Row(G._conv_shared("direct"), ("conv_direct",), CONV, (1, 3), ("conv_direct_kernel",), ("direct FIR taps=128",), 3),
    "conv_r4": Row(G._conv_shared("r4"), ("conv_fft",), CONV, (1, 2, 3, 65), ("conv_fft_kernel<fwd>", "conv_mac_kernel", "conv_fft_kernel<inv>"),
                   ("fft B=128 N=256 P=2",), 65, None, True),
    "conv_3pass": Row(G._conv_shared("3pass"), ("conv_fft",), CONV, (1, 3), ("conv_fft_kernel<fwd>", "conv_mac_kernel", "conv_fft_kernel<inv>"),
                      ("fft B=8192 N=16384 P=7",), 3, None, True),
    "conv_3pass_two_blocks": Row(G._conv_shared("3pass"), ("conv_fft",), CONV, (1022, 1024, 1025), ("conv_fft_kernel<fwd>", "conv_mac_kernel", "conv_fft_kernel<inv>"),
                                 ("fft B=8192 N=16384 P=7 blocks=2 ",), None, None, True, dict(mono=True, frames=8192 + 133)),
    "conv_3pass_biquad": Row(G.b_conv_3pass_biquad, ("conv_fft",), Bound("tests/test_gpu_parity.py::test_biquad_folded_into_the_forward_transform", 1e-6, np.inf),
                             (2, 3), ("conv_fft_kernel<fwd>",), ("filtered by the forward transform's input stage", "(+ the Biquad in front, in the forward transform)"), 3, None, True),
    "conv_inst_direct": Row(G._conv_inst("direct"), ("conv_direct",), CONV_INST, (1, 3), lambda n: ("conv_inst_direct_kernel" if n > 1 else "conv_direct_kernel",),
                            ("direct FIR taps=128",), 3, 1),
    "conv_inst_r4": Row(G._conv_inst("r4"), ("conv_fft",), CONV_INST, (1, 2, 3, 65), lambda n: ("conv_inst_mac_kernel" if n > 1 else "conv_mac_kernel",),
                        lambda n: ("fft B=128 N=256 P=2", ("+" if n > 1 else "-", "per-instance impulse responses")), 65, 1, True),
    "osc_par": Row(G.b_osc_par, ("osc",), OSC, (1, 3), ("osc_par_kernel",), ("sawtooth (time-parallel, closed-form phase)",), None),
    "osc_post_gain": Row(G.b_osc_post_gain, ("osc",), OSC, (1, 3), ("osc_par_kernel",), ("oscillator node 1 renders 1 gain(s)",), None),
    "osc_waves": Row(G.b_osc_waves, ("osc",), OSC, (2, 3), ("osc_par_kernel",), ("one PeriodicWave per instance", "custom (time-parallel, closed-form phase)"), None, 1),
    "osc_types": Row(G.b_osc_types, ("osc",), OSC, (2, 3), ("osc_par_kernel",), ("one type per instance", "(time-parallel, closed-form phase)"), None, 1),
    "fm_pair": Row(G.b_fm_pair, ("osc", "chain"), Bound("tests/test_oscillator.py::test_parity_fm_fold", 2e-5, 2e-4), (1, 3), ("osc_scan_kernel",),
                   ("sine (prefix-sum phase)", "folded into the carrier's prefix-sum kernel"), None),
    "compressor": Row(G.b_compressor, ("compressor",), Bound("tests/test_compressor.py::test_256_contexts (check_batch: the model)", 0.0, 0.0),
                      (1, 63, 64, 65), ("compressor_level_kernel", "compressor_detector_kernel", "compressor_apply_kernel"),
                      lambda n: (f"compressor_detector_kernel ({(n + 63) // 64} wavefront(s), one lane per context)",), 65),
    "timeline": Row(G.b_timeline, ("timeline",), Bound("tests/test_automation.py::test_per_instance_automation_is_replayed_on_the_device", 1e-6, 2e-5),
                    (1, 63, 64, 65), lambda n: ("timeline_kernel",) if n > 1 else (), ("ops=[GAIN]",), 65),
    "hrtf_static": Row(G.b_hrtf_static, ("hrtf",), HRTF, (1, 2, 3), ("hrtf_kernel",), ("panner node 1: HRTF, 415-tap",), 3,
                       device_plan=("partitions of 128 taps as 256-point transforms", ("-", "takes the direct form"))),
    "hrtf_short": Row(G.b_hrtf_short, ("hrtf",), HRTF, (1, 3), ("hrtf_kernel",), ("panner node 1: HRTF, 415-tap",), 3,
                      device_plan=("a launch of fewer than 16 quanta takes the direct form with the host-interpolated pair (hrtf8_kernel): this render does",)),
    "hrtf_moving": Row(G.b_hrtf_moving, ("hrtf",), HRTF, (1, 3), ("hrtf_kernel",), ("row(s) x 6, direct FIR per render quantum",), 3,
                       device_plan=("row(s) x 6, direct FIR per render quantum", ("-", "256-point transforms"))),
    "oversampled_shaper": Row(G.b_oversampled_shaper, ("os_fft",), Bound("tests/test_oversample.py::test_oversample_many_instances_sampled", 1e-6, np.inf),
                              (1, 5, 6, 11), ("osfft_kernel",), ("4x oversampling as 10 256-point transforms per quantum in one launch (runs of 8 quanta, 3 per instance)",), 6),
    "echo_ring": Row(G.b_echo_ring, ("loop",), Bound("tests/test_cycles.py::test_parity_random_echo_loops", 0.0, 0.0, bits=True), (1, 3), ("echo_ring_kernel",),
                     ("rendered by the LDS-ring kernel in ONE launch",), 3),
    "loop_kernel": Row(G.b_loop_kernel, ("loop",), Bound("tests/test_cycles.py::test_parity_feedback_delay", 1e-6, np.inf), (1, 3), ("loop_kernel",),
                       ("feedback loop: 3 item(s) per quantum",), 3),
    "qloop_hrtf": Row(G.b_qloop_hrtf, ("dyn", "link", "hrtf"), FROZEN_LOOP, (1, 3), ("dyn_kernel", "link_kernel", "hrtf_kernel"),
                      ("feedback loop with a frozen-state node inside", "dynamic-count group"), 3),
    "qloop_shaper_2x": Row(G.b_qloop_shaper_2x, ("dyn", "link", "os_fft"), FROZEN_LOOP, (1, 3, 65), ("dyn_kernel", "link_kernel", "osfft_kernel"),
                           ("feedback loop with a frozen-state node inside", "dynamic-count group"), 3),
    "qloop_conv_and_shaper": Row(G.b_qloop_conv_and_shaper, ("conv_codes", "dyn", "conv_fft"),
                                 Bound("tests/test_frozen_loops.py::test_convolver_and_oversampled_shaper_in_one_loop", 1e-6, 2e-5, True), (1, 3, 65),
                                 ("dyn_kernel", "conv_code_kernel", "conv_fft_kernel<fwd>"), ("feedback loop with a frozen-state node inside", "fft B=128 N=256 P=3"), 3,
                                 None, True),
    "dyn_split": Row(G.b_dyn_split, ("dyn",), Bound("tests/test_hrtf.py::test_transform_form_where_a_node_behind_the_panner_decides_on_exact_zeros", 1e-6, 2e-5, True),
                     (512, 513), ("dyn_kernel",), ("[GAIN2,convIn1], no item keeps state from quantum to quantum: the quanta are spread over workgroups", ("-", "feedback loop")), None),
    "splitter_merger": Row(G.b_splitter_merger, ("route",), Bound("tests/test_channel_routing.py::test_splitter_with_two_connections (the written definition)", 0.0, 0.0, bits=True),
                           (1, 3), ("route_kernel",), ("-> route_kernel (2 term(s))",), 3),
    "listener_in_a_loop": Row(G.b_listener_in_a_loop, ("panner_geom",), Bound("tests/test_gpu_parity.py::test_audio_rate_listener_automation", 1e-6, 5e-6), (1, 3),
                              ("panner_geom_kernel",), ("per-frame geometry on the device (1 table row(s))",), 3),
    "block_loop_zero_conv": Row(G.b_block_loop_zero_conv, ("zero_fill",), Bound("tests/test_cycles.py::test_parity_convolver_inside_a_block_scheduled_loop", 1e-6, 2e-5, True),
                                (1, 3), (), ("all-zero impulse response -> zero fill",), 3),
}
CASES = [(name, n) for name, row in TABLE.items() for n in row.sizes]

# the launches with the batch on gridDim.y / gridDim.z: graph -> (contexts, mono, frames, rows per context) of the batches that
# cross 65535 rows — the shortest render the path admits
Big = namedtuple("Big", "n mono frames rows_per_context")
ROW_LIMIT = {
    "delay_gather": (Big(32769, False, 1200, 2.0), Big(65537, True, 1200, 1.0)),     # launch_delay: n_inst * nch rows (1200 frames: the longest delay is 832)
    "osc_par": (Big(65537, True, 133, 1.0),),                                         # osc_par_kernel
    "osc_post_gain": (Big(65537, True, 133, 1.0),),                                   # ... with a folded gain: one value per context in its store
    "osc_waves": (Big(65537, True, 133, 1.0),),                                       # osc_par_lds_kernel
    "osc_types": (Big(65537, True, 133, 1.0),),                                       # osc_types_par_kernel
    "compressor": (Big(65537, True, RQ * 6, 1.0),),                                   # level, apply (6 quanta: 3 are the look-ahead)
    "conv_direct": (Big(65537, True, 133, 1.0),),                                     # launch_conv_direct
    "conv_inst_direct": (Big(65537, True, 133, 1.0),),                                # launch_conv_inst_direct
    "conv_r4": (Big(131073, True, 133, 0.5), Big(65537, False, 133, 1.0)),            # forward / inverse: pairs on z; products: pair * cout on y
    "conv_inst_r4": (Big(65537, False, 133, 1.0),),                                   # launch_conv_inst_mac, and the per-instance spectra (context on z)
    "conv_3pass": (Big(131073, True, 133, 0.5),),                                     # waa_conv3.hip: pairs on z
    "conv_3pass_biquad": (Big(131073, True, RQ * 2, 0.5),),                           # conv_fft3_fwd_bq_kernel: coefficients and state per context
    "hrtf_short": (Big(65537, True, None, 1.0),),                                     # hrtf8_kernel<true> (the graph's own 6 quanta)
    "hrtf_moving": (Big(65537, True, None, 1.0),),                                    # hrtf_kernel
}
BIG_CASES = [(name, big) for name, bigs in ROW_LIMIT.items() for big in bigs]


def _of(spec, n):
    return spec(n) if callable(spec) else spec


def _phrases(row, n, spec=None):
    return [p if isinstance(p, tuple) else ("+", p) for p in _of(row.plan if spec is None else spec, n)]


# ---- references ---------------------------------------------------------------------------------------------------------------
def _audio(row, ids, **kw):
    """the source audio [n, channels, frames] the builder gives the contexts `ids` (from a context that is never prepared)"""
    c = G.build(row.build, waa.default_binding(), ids, device=waa.PLAN_ONLY, **kw)
    return G._node(c, waa.AudioBufferSourceNode)._batch[0]


def reference(orc, name, ids, **kw):
    """what the contexts `ids` of the graph render: the oracle's batch of them (row.chunk at a time) — or, for the two kinds the oracle
    does not have, the written definition (splitter -> merger with the channels swapped, channel 1 through Gain 0.5) / None
    (compressor: compared by check_compressor against the model)"""
    row = TABLE[name]
    if name == "splitter_merger":
        x = _audio(row, ids, **kw)
        return np.stack([x[:, 1] * np.float32(0.5), x[:, 0]], axis=1)
    if name == "compressor":
        return None
    orc.lib.orc_set_threads.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    ids = np.asarray(ids)
    step = row.chunk or len(ids)
    parts = []
    for lo in range(0, len(ids), step):
        c = G.build(row.build, orc, ids[lo:lo + step], **kw)
        c.prepare()
        orc.lib.orc_set_threads(c._handle, usable_cpus())
        parts.append(c.start_rendering_sync().data)
        c.close()
    return np.concatenate(parts)


def check_compressor(what, got, ids, **kw):
    """tests/test_compressor.py's comparison: every context against the model run on its own audio with its own params"""
    from test_compressor import check_batch
    x = _audio(TABLE["compressor"], ids, **kw)
    check_batch(what, got, x, lambda k: cm.param_rows(x.shape[2] // RQ, **G.comp_params(int(ids[k]) % G.K)), SR)


def compare(what, got, ref, bound):
    """every (context, channel) of got against ref under the kind's bound; a non-finite sample on either side fails"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert_all_finite(got, f"{what}: device render")
    assert_all_finite(ref, f"{what}: reference")
    peak = float(np.abs(ref).max())
    assert peak > 1e-3, (what, "the reference is silent")
    if bound.bits:
        d = first_difference(got, ref)
        assert d is None, f"{what}: {d[0]} of {got.size} samples differ from the reference; the first at (context, channel, frame) {d[1]}: {d[2]!r}, reference {d[3]!r}"
        return
    scale = max(1.0, peak) if bound.scaled else 1.0
    err = rms_err(got, ref)
    k = np.unravel_index(int(np.argmax(err)), err.shape)
    worst, worst_abs = strict_max(0.0, err[k]), strict_max(0.0, np.abs(got - ref).max())
    print(f"{what}: worst per-channel RMS error {worst:.3e} at (context, channel) {tuple(int(v) for v in k)}, max |diff| {worst_abs:.3e}, peak {peak:.3f}")
    assert_le(worst, bound.rms * scale, (what, "RMS", tuple(int(v) for v in k)))
    assert_le(worst_abs, bound.max_abs * scale, (what, "max |diff|"))


def check(orc, name, what, got, ids, **kw):
    if name == "compressor":
        check_compressor(what, got, ids, **kw)
        assert_all_finite(got, what)
    else:
        compare(what, got, reference(orc, name, ids, **kw), TABLE[name].bound)


def render(hip, name, n, **kw):
    """the batch of contexts 0 .. n-1 on the device, profiled: (context kept open, its render); the slots the table names ran"""
    row = TABLE[name]
    c = G.build(row.build, hip, range(n), device=0, **{**row.kw, **kw})
    c.profile()
    out = c.start_rendering_sync().data
    c.sync()   # (folds the launches' event pairs into the profile)
    for slot in _of(row.slots, n):
        assert ran(c, slot) > 0, (name, n, slot, c.profile_entries(), c.plan_describe())
    text = c.plan_describe()
    for sign, phrase in _phrases(row, n, row.device_plan):
        assert (phrase in text) == (sign == "+"), (name, n, sign, phrase, text)
    return c, out


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_the_table_covers_every_kind():
    kinds = {k for row in TABLE.values() for k in row.kinds} | {"qgemm"}   # (qgemm: test_matrix_form_* below)
    assert kinds == set(KIND_NAMES), sorted(set(KIND_NAMES) ^ kinds)
    for name in TABLE:
        assert f"::test_" in TABLE[name].bound.test, name
    assert set(ROW_LIMIT) <= set(TABLE)


@pytest.mark.parametrize("name", list(TABLE))
def test_every_size_plans_and_names_its_kernel(hip, name):
    """plan-only, every size of the row and the batches past the row limit: the plan text says what the table says the size
    selects (both sides of a threshold: the phrase is there at one size and absent at the other)"""
    row = TABLE[name]
    cases = [(n, dict(row.kw)) for n in row.sizes] + [(b.n, dict(mono=b.mono, frames=b.frames, periodic=True)) for b in ROW_LIMIT.get(name, ())]
    for n, kw in cases:
        c = G.build(row.build, hip, range(n), device=waa.PLAN_ONLY, **kw)
        text = c.plan_describe()
        c.close()
        assert text.startswith(f"batch: {n} instance(s) x "), (name, n, text[:200])
        for sign, phrase in _phrases(row, n):
            if kw.get("mono"):
                phrase = phrase.replace("2ch", "1ch").replace("C=2", "C=1")
            assert (phrase in text) == (sign == "+"), (name, n, sign, phrase, text)
        if row.pair:
            assert f"pairs={(n + 1) // 2} " in text, (name, n, text)


def test_thresholds_are_asserted_on_both_sides():
    """the sizes of a threshold row lie on both sides of it"""
    ff = TABLE["feed_forward_echo"]
    assert {_ff_slots(n) for n in ff.sizes} == {("echo_ring_kernel",), ("chain_kernel",)} and 255 in ff.sizes and 256 in ff.sizes
    assert {(n + 63) // 64 for n in TABLE["compressor"].sizes} == {1, 2} and {(n + 63) // 64 for n in TABLE["timeline"].sizes} == {1, 2}
    assert {(2 * n + 63) // 64 for n in TABLE["biquad_a_rate_shared"].sizes} == {1, 2}
    assert {(3 * n + 15) // 16 for n in TABLE["oversampled_shaper"].sizes} == {1, 2, 3}   # (15 / 18 runs: the second workgroup holds two contexts' runs)
    # f3_blocks_per_wg / pipe_blocks_per_wg (waa_conv3.hip, waa_conv.hip) of the two-block rows: one block per workgroup below 512 streams
    def blocks_per_wg(streams, nbl=2):
        segs = 1 if streams >= 512 else min(nbl, (512 + streams - 1) // streams)
        return (nbl + segs - 1) // segs
    assert [blocks_per_wg((n + 1) // 2) for n in TABLE["conv_3pass_two_blocks"].sizes] == [1, 2, 2] and blocks_per_wg(32769, 1) == blocks_per_wg(2, 1) == 1
    # launch_dyn's q_split of the stateless groups of dyn_split (193 quanta)
    assert [min(max(16384 // n, 16), 193 // 6) for n in TABLE["dyn_split"].sizes] == [32, 31]
    assert {(n + 7) // 8 for n in TABLE["resample_plain"].sizes} == {1, 2, 4, 5}   # (wavefronts of 8 contexts per sub-tile; 4 = one workgroup)
    for name, bigs in ROW_LIMIT.items():
        for b in bigs:
            assert b.n * b.rows_per_context > 65536 and waa_row_limit() > (b.n - 5) * b.rows_per_context, (name, b)   # (just past the limit)


def waa_row_limit():
    return 65535   # MAX_GRID_ROWS, waa_internal.hpp


@pytest.mark.measure
def test_matrix_form_is_refused_past_the_row_limit(hip, monkeypatch):
    """launch_qgemm (WAA_OS_MATRIX, measurement build only) has one grid row per (context, channel): it is not sliced, the planner
    refuses with the launch and the limit named; one context below the limit plans"""
    monkeypatch.setenv("WAA_OS_MATRIX", "1")
    for n, ok in ((32767, True), (32768, False)):
        c = G.build(G.b_oversampled_shaper, hip, range(n), device=waa.PLAN_ONLY, periodic=True)
        if ok:
            assert "as two matrix products over render quanta" in c.plan_describe()
        else:
            with pytest.raises(waa.WaaError, match=r"launch_qgemm \(WAA_OS_MATRIX\) has one grid row per \(context, channel\), 65536 here, and a grid has at most 65535") as e:
                c.plan_describe()
            assert e.value.status == 4
        c.close()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_row_limit_of_the_device():
    """the slices the launchers make fit the device's grid; the figure as read goes into this file's header"""
    hiprt = ctypes.CDLL("libamdhip64.so")
    v, grid = ctypes.c_int(), []
    for attr in (29, 30, 31):   # hipDeviceAttributeMaxGridDimX / Y / Z (hip_runtime_api.h of ROCm 7: the same values hipDeviceProp_t::maxGridSize holds)
        assert hiprt.hipDeviceGetAttribute(ctypes.byref(v), attr, 0) == 0
        grid.append(v.value)
    print("maxGridSize", tuple(grid))
    assert grid[0] >= 2 ** 31 - 1 and waa_row_limit() <= min(grid[1:]) <= 65536, grid   # (every batch of ROW_LIMIT crosses 65536 too)


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", CASES, ids=[f"{name}-{n}" for name, n in CASES])
def test_small_sizes_every_context_against_the_oracle(hip, orc, name, n):
    """GPU test 1: the kernel the table names ran (profile slots), and every context of the batch is the oracle's"""
    c, out = render(hip, name, n)
    c.close()
    check(orc, name, f"{name}, {n} context(s)", out, np.arange(n), **TABLE[name].kw)
    if n > 1 and name not in ("biquad_a_rate_shared",):
        assert len({out[i].tobytes() for i in range(n)}) == n, (name, n, "two contexts rendered the same samples")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [name for name, row in TABLE.items() if row.edge])
def test_neighbours_do_not_hear_each_other(hip, name):
    """GPU test 2: the same plan rendered again with the audio of ONE context j replaced (re-armed batch): every other context keeps
    its bits; j's partner in a packed convolver pair keeps them within the convolver's bound (the documented crosstalk)"""
    row = TABLE[name]
    n = row.edge
    c, first = render(hip, name, n)
    for j in sorted({0, n // 2, n - 1}):
        donor = G.build(row.build, hip, range(n), device=waa.PLAN_ONLY, other=j, **row.kw)
        assert refill_from(c, donor) >= 1
        donor.close()
        second = render_again(c)
        assert_all_finite(second, f"{name}: second render")
        assert first_difference(second[j], first[j]) is not None, (name, j, "the replaced audio changed nothing")
        partner = j ^ 1 if row.pair and (j ^ 1) < n else None
        for i in range(n):
            if i == j:
                continue
            d = first_difference(second[i], first[i])
            if i == partner:
                if d is not None:
                    compare(f"{name}: context {i}, the pair partner of the replaced context {j}", second[i:i + 1], first[i:i + 1], row.bound)
                continue
            assert d is None, f"{name}, {n} contexts: new audio in context {j} changed context {i}: {d[0]} samples, the first at (channel, frame) {d[1]}: {d[2]!r}, before {d[3]!r}"
    c.close()


def _selected(big):
    """contexts 0 .. K-1, the four on each side of the contexts that hold rows 65535 / 65536, the last four"""
    n = big.n
    lo, hi = int(65535 / big.rows_per_context), int(65536 / big.rows_per_context)
    ids = set(range(G.K)) | set(range(lo - 4, hi + 5)) | set(range(n - 4, n))
    return np.array(sorted(i for i in ids if 0 <= i < n))


@pytest.mark.gpu
@pytest.mark.parametrize("name,big", BIG_CASES, ids=[f"{name}-{b.n}-{'mono' if b.mono else 'stereo'}" for name, b in BIG_CASES])
def test_more_rows_than_the_grid_allows(hip, orc, name, big):
    """GPU test 3: a batch whose row count crosses 65535.  Audio and values repeat with period K in the context index, so context i
    must equal context i % K bit for bit (but the single last context of an odd batch on a packed-pair path: within the path's
    bound); contexts 0 .. K-1, those around the rows 65535 / 65536 and the last four are compared with the oracle's small batch"""
    row, kw = TABLE[name], dict(mono=big.mono, frames=big.frames, periodic=True)
    c, out = render(hip, name, big.n, **kw)
    c.close()
    assert_all_finite(out, f"{name}: device render")
    base = out[:G.K]
    assert float(np.abs(base).max()) > 1e-3 and float(np.abs(out[-1]).max()) > 1e-3, (name, "silent")
    alone = big.n - 1 if row.pair and big.n % 2 else None
    bits = out.view(np.uint32)
    for k in range(G.K):
        same = (bits[k::G.K] == bits[k]).all(axis=(1, 2))
        bad = [k + G.K * int(m) for m in np.flatnonzero(~same) if k + G.K * int(m) != alone]
        assert not bad, f"{name}: {len(bad)} context(s) differ from context {k} (same audio, same values), the first {bad[:8]}"
    if alone is not None:
        compare(f"{name}: the last context, alone in its pair", out[alone:alone + 1], base[alone % G.K][None], row.bound)
    ids = _selected(big)
    check(orc, name, f"{name}, {big.n} contexts: {len(ids)} of them", out[ids], ids, **kw)
