/*
 * waa_hip_device.h — entry points of the device library that have no counterpart in the CPU oracle.
 *
 * include/waa_hip.h is the boundary both libraries export (the oracle with the prefix orc_).  What is declared here is a
 * capability of the batch that the oracle's one-context-at-a-time model does not have and does not need: parity tests
 * render the oracle one context per instance instead (tests/test_iir_per_instance.py).
 */
#ifndef WAA_HIP_DEVICE_H
#define WAA_HIP_DEVICE_H

#include "waa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* IIRFilterNode::new(IIRFilterOptions{feedforward, feedback}) of ONE context of the batch (src/node/iir_filter.rs:163-189,
 * :282-320): in the reference every context constructs its own IIRFilterNode from its own options.  Replaces what took one
 * batch, one plan and one launch sequence per distinct filter: a sweep over filter designs, a thousand clips each through
 * its own equaliser, serving requests that differ only in their filter.
 *
 * Same validation and normalisation as waa_iir_set_coefficients (1..20 coefficients each, feedforward not all zero,
 * feedback[0] != 0; padded to equal length and divided by feedback[0]); refused once the batch is planned
 * (InvalidStateError), for an instance >= n_instances and for a node of another kind (WAA_ERR_INVALID_ARGUMENT).
 * instance = WAA_ALL_INSTANCES is waa_iir_set_coefficients.  The first call puts the node into per-instance mode;
 * instances without a set of their own use the one given with waa_iir_set_coefficients, and an instance that has neither
 * fails the plan with an InvalidStateError naming the node and the instance.
 *
 * Lengths may differ between instances: the plan pads every instance with zero coefficients to the node's longest.  That
 * is exact for finite input (a padded state evaluates (0 x - 0 y) + 0 = +0); a non-finite input sample
 * makes 0 x a NaN where the reference's shorter filter has no such term.  If the state transition of
 * ANY instance is too ill-conditioned for the scan kernel, the whole node is rendered by an exact kernel.
 * waa_batch_rearm keeps the coefficients, like everything but the audio. */
waa_status waa_iir_set_coefficients_instance(waa_batch* batch, uint32_t node, uint32_t instance, const double* feedforward,
                                             uint32_t n_feedforward, const double* feedback, uint32_t n_feedback);

/* OscillatorNode::set_periodic_wave(PeriodicWave::new(PeriodicWaveOptions{real, imag, disable_normalization})) of ONE context of
 * the batch (src/periodic_wave.rs:88-190, src/node/oscillator.rs:318-321): in the reference every context builds its own
 * PeriodicWave.  Replaces one batch, one plan and one launch sequence per distinct timbre: a thousand notes each with its own
 * additive spectrum, a sweep over synthesiser settings, sound matching.  _set_wavetable_instance hands over the finished
 * 8192-point table instead (what waa_oscillator_set_wavetable is to waa_oscillator_set_periodic_wave).
 *
 * Same validation as the shared calls (`real` / `imag` not both null, n >= 2; a table has exactly 8192 points); refused once the
 * batch is planned (InvalidStateError), for an instance >= n_instances and for a node of another kind
 * (WAA_ERR_INVALID_ARGUMENT).  instance = WAA_ALL_INSTANCES is the shared call.  The first call puts the node into per-instance
 * mode; an instance without a wave of its own uses the shared one — its host-built table, bit for bit what it renders with in
 * shared mode — and an instance that has neither fails the plan with an InvalidStateError naming the node and the instance.
 *
 * The tables of coefficient sets are generated ON THE DEVICE when the batch is planned, one per distinct set (instances whose
 * padded real / imag and flag are bitwise equal share a table), in the reference's f32 order of operations; the device's
 * sinf / cosf are the only difference from the host-built table of the shared call (the bound: DESIGN.md 3.1e).  Lengths may
 * differ between instances: the plan pads with zero coefficients to the node's longest set, which is exact for finite
 * coefficients (a padded term adds 0 cos + 0 sin = +0 to a sum that starts at +0).  waa_batch_rearm keeps the waves and their
 * tables, like everything but the audio. */
waa_status waa_oscillator_set_periodic_wave_instance(waa_batch* batch, uint32_t node, uint32_t instance, const float* real,
                                                     const float* imag, uint32_t n, int32_t disable_normalization);
waa_status waa_oscillator_set_wavetable_instance(waa_batch* batch, uint32_t node, uint32_t instance, const float* table, uint32_t n);

/* The 8192-point table `instance` renders with, into out[n] (n = 8192): after the plan, for a node in per-instance mode, the
 * instance's row of the device's tables (downloaded); otherwise the table built on the host — the shared wave's, the instance's
 * finished table, or its coefficients through the host's generator.  InvalidStateError if the instance has no wave at all. */
waa_status waa_oscillator_get_wavetable(waa_batch* batch, uint32_t node, uint32_t instance, float* out, uint32_t n);

/* WaveShaperNode::set_curve of ONE context of the batch (src/node/waveshaper.rs:203-217): in the reference every context sets
 * the curve of its own WaveShaperNode.  Replaces one batch, one plan and one launch sequence per distinct curve: a sweep over
 * drive amounts, a thousand clips each through its own saturator, sound matching over distortion shapes.
 *
 * Refused once the batch is planned (InvalidStateError), for an instance >= n_instances, for a node of another kind and for a
 * curve without points (WAA_ERR_INVALID_ARGUMENT); a second curve for the same instance is "InvalidStateError - cannot assign
 * curve twice", as for the shared call.  instance = WAA_ALL_INSTANCES is waa_waveshaper_set_curve.  The first call with a real
 * instance puts the node into per-instance mode; an instance without a curve of its own uses the shared one, and an instance
 * that has neither renders as the reference renders a node without a curve: its input passes through.  That is no error.
 *
 * Lengths may differ between instances and nothing is padded: every instance keeps its own length, because the lookup's scale
 * is (n - 1) / 2.  Instances with bitwise equal curves share one copy on the device.  Such a node ends its chain: its input is
 * a materialised signal (or a source read in place) and one launch of its own renders it; what it computes
 * per sample is the expression the shared curve is rendered with, bit for bit.  Out of scope (status 4, naming the node): the
 * node inside a feedback loop, in a graph that needs exact per-quantum channel counts, and with oversample 2x / 4x.
 * waa_batch_rearm keeps the curves, like everything but the audio. */
waa_status waa_waveshaper_set_curve_instance(waa_batch* batch, uint32_t node, uint32_t instance, const float* curve, uint32_t n);

/* BiquadFilterNode::set_type of ONE context of the batch (src/node/biquad_filter.rs:28-373 for what a type computes, the type
 * message at :901-906): in the reference every context builds its own BiquadFilterNode with its own type.  Replaces one batch,
 * one plan and one launch sequence per filter type (up to eight): a random-equaliser augmentation where every clip goes through
 * its own lowpass / peaking / shelf with its own frequency, Q and gain, a sweep over filter designs, serving requests that
 * differ in their filter type.  The node's four AudioParams were per instance already.
 *
 * type: 0 .. 7 as in waa_node_desc.i[0] of a BIQUAD node; anything else is "bad biquad type" (WAA_ERR_INVALID_ARGUMENT), the
 * refusal of waa_batch_create.  Refused once the batch is planned (InvalidStateError), for an instance >= n_instances and for a
 * node of another kind (WAA_ERR_INVALID_ARGUMENT).  instance = WAA_ALL_INSTANCES sets the node's shared type (i[0]) and leaves
 * the types given to single instances alone; an instance without a type of its own uses the shared one.  As set_type in the
 * reference, the call may be repeated: a later call for the same instance replaces the earlier one.
 *
 * A node whose instances all end up with the same type plans and renders exactly as a shared node of that type.  Where the types
 * differ, constant and k-rate coefficient rows are built per instance from the instance's type (they were per instance already);
 * an a-rate node gets one table row per instance even under one shared automation (40 B per frame and instance, DESIGN.md 3.1
 * "Per-context types"), written by biquad_coef_inst_kernel with the arithmetic of the shared kernel; and a Biquad in front of a
 * ConvolverNode is not folded into the impulse response — the exact-order filter stage renders it.  Called at a suspend point it
 * applies to the whole render, like the shared option.  waa_batch_rearm keeps the types, like everything
 * but the audio. */
waa_status waa_biquad_set_type_instance(waa_batch* batch, uint32_t node, uint32_t instance, int32_t type);

/* OscillatorNode::set_type of ONE context of the batch (src/node/oscillator.rs:305-330): in the reference every context owns its
 * OscillatorNode and sets its type.  Replaces one batch, one plan and one launch sequence per waveform (up to five): a data set
 * of synthetic notes, each with a random waveform, pitch, detune and envelope.  Frequency, detune, start / stop and the
 * PeriodicWave were per instance already.
 *
 * type: WAA_OSC_SINE .. WAA_OSC_TRIANGLE.  WAA_OSC_CUSTOM is "InvalidStateError: Custom type cannot be set manually", as in the
 * reference; anything else is "bad oscillator type" (WAA_ERR_INVALID_ARGUMENT).  Refused once the batch is planned
 * (InvalidStateError), for an instance >= n_instances and for a node of another kind (WAA_ERR_INVALID_ARGUMENT).
 * instance = WAA_ALL_INSTANCES sets the node's shared type (i[0]).  A later call for the same instance replaces the earlier one.
 *
 * The type instance i renders with is resolved when the batch is planned, in this order:
 *   1. i has a PeriodicWave of its own (waa_oscillator_set_periodic_wave_instance / _set_wavetable_instance): custom, with that
 *      wave; a type set for i is ignored, as the reference ignores set_type on a node that has a wave (:321-324);
 *   2. i has a type of its own: that type, EVEN WHERE A SHARED WAVE EXISTS.  Everywhere in this interface the values given for
 *      WAA_ALL_INSTANCES are defaults for the contexts without a setting of their own; this is the one place where a batch is
 *      therefore not literally "every context made the ALL call" (such a context would be custom);
 *   3. a shared wave exists: custom, with it;
 *   4. the node has per-instance waves but no shared one, and i has neither a wave nor a type: the plan fails,
 *      "InvalidStateError - OscillatorNode N has no PeriodicWave for instance k";
 *   5. otherwise the node's shared type (i[0]).
 * waa_oscillator_get_wavetable of an instance that resolves to a built-in type is InvalidStateError ("has no PeriodicWave").
 *
 * A node whose instances all resolve to the same type plans and renders exactly as today (the same kernels, uploads and plan
 * text).  Where they differ, the plan uploads a type byte per instance, the 2048-point sine table and table rows for the custom
 * instances alone, and the one Osc step is rendered by the kernels of waa_osc_types.hip, which read the type per instance and
 * otherwise are the single-type kernels (one launch for the time-parallel form, two passes for the prefix-sum form): every
 * instance gets the bits a batch of its type alone gives it.  The post-gain, LFO and two-operator FM folds carry the types.
 * Called at a suspend point it applies to the whole render, like the shared option.  waa_batch_rearm
 * keeps the types, like everything but the audio. */
waa_status waa_oscillator_set_type_instance(waa_batch* batch, uint32_t node, uint32_t instance, int32_t type);

/* PannerNode::new(PannerOptions{distance_model, ref_distance, max_distance, rolloff_factor, cone_*}) of ONE context of the batch
 * (src/node/panner.rs:146-166, the setters at :545-641): in the reference every context builds its own PannerNode with its own
 * options.  Replaces one batch, one plan and one launch sequence per distinct option set: a spatial augmentation that places a
 * thousand clips, each at its own position with its own distance law, rolloff and directivity cone.  The fifteen position,
 * orientation and listener AudioParams were per instance already.
 *
 * A call carries a COMPLETE set (there is no all-zero-means-defaults shorthand here); a later call for the same instance
 * replaces the earlier one.  distance_model: as waa_node_desc.i[1] of a PANNER node, anything else is "bad distance model"
 * (WAA_ERR_INVALID_ARGUMENT).  The values are checked like waa_batch_create checks d[0..5], with the reference's messages:
 * "RangeError - refDistance cannot be negative", "RangeError - maxDistance must be strictly positive", "RangeError - rolloffFactor
 * cannot be negative" (WAA_ERR_INVALID_ARGUMENT) and "InvalidStateError - coneOuterGain must be in the range [0, 1]"
 * (WAA_ERR_INVALID_STATE).  Refused with WAA_ERR_INVALID_ARGUMENT: a NULL `options`, a non-zero `reserved`, an instance
 * >= n_instances and a node of another kind; refused once the batch is planned (InvalidStateError).  instance =
 * WAA_ALL_INSTANCES replaces the node's shared set (i[1], d[0..5]) and leaves the sets given to single instances alone; an
 * instance without a set of its own uses the shared one.  The panning model (i[0]) is not part of the set: it decides the plan's
 * shape and stays one per node.
 *
 * A node whose instances all resolve to one set plans and renders exactly as a shared node of that set (the same launches, table
 * rows and plan text).  Where the sets differ, the host geometry of a single-valued listener and the HRTF geometry table take
 * every instance's gains from its own set (the HRTF table then has one row per instance), and the per-frame geometry of an
 * audio-rate listener is written by panner_geom_inst_kernel — panner_geom_kernel with the set read from a table of one 40-byte
 * row per instance — into one table row per instance, even under one listener automation shared by the batch (7 tables x 4 B
 * per frame and instance).  No consumer kernel differs.  Called at a suspend point it applies to the whole
 * render, like every payload.  waa_batch_rearm keeps the sets, like everything but the audio. */
typedef struct waa_panner_options {
  int32_t distance_model;            /* as waa_node_desc.i[1] of a PANNER node */
  int32_t reserved;                  /* 0 */
  double ref_distance, max_distance, rolloff_factor;
  double cone_inner_angle, cone_outer_angle, cone_outer_gain;
} waa_panner_options;
waa_status waa_panner_set_options_instance(waa_batch* batch, uint32_t node, uint32_t instance, const waa_panner_options* options);

/* DynamicsCompressorNode::reduction (src/node/dynamics_compressor.rs:304-306): the gain reduction in dB that the render thread
 * stored when it finished a render quantum — `-detector_value + makeup_gain` of the quantum's last frame (:440, stored at :450;
 * 0 before anything is rendered, :249).  Replaces polling one context at a time while it renders: a batched offline render
 * keeps the WHOLE trace, the value the reference would return after every render quantum, for every context — a gain-reduction
 * curve per clip, for plots, labels of a data set, choosing a threshold per clip.
 *
 * The meter is opt-in per node: waa_node_desc.i[0] of a WAA_NODE_DYNAMICS_COMPRESSOR is 0 (off, the default) or 1 (keep the
 * trace); waa_batch_create refuses any other value (WAA_ERR_INVALID_ARGUMENT, naming the node and the value).  A node with the
 * meter off plans and renders exactly as before (the same three launches, the same plan text).  With the meter on the plan
 * allocates [n_instances][n_quanta] floats and the node's step ends with a fourth launch, compressor_meter_kernel: one f32
 * negation and one f32 add per value, in the reference's order, from the detector's values and the make-up gain of the
 * quantum's own block constants.  Every render writes the trace again; waa_batch_rearm keeps the buffer.
 *
 * waa_compressor_get_reduction: the value after the last rendered quantum, for one instance.
 * waa_compressor_get_reduction_series: dst[n_instances][n_quanta], row q = the value after quantum q; n_quanta must be the
 * batch's ceil(length / 128), anything else is WAA_ERR_INVALID_ARGUMENT (as are a NULL batch or destination, a node index and
 * an instance out of range).  Both are WAA_ERR_INVALID_STATE (InvalidStateError) for a node of another kind, for a compressor
 * whose meter is off (the message names i[0]), before the batch has rendered and while a ranged render (waa_render_range) is
 * still in front of its last range.  A pageable destination is filled through the batch's pinned staging block, like every
 * download.  A metered node that does not reach the destination is not rendered: its values are the initial 0.
 * Out of scope: the trace of a batch merged from single contexts, and waa_render_sharded. */
waa_status waa_compressor_get_reduction(waa_batch* batch, uint32_t node, uint32_t instance, float* value);
waa_status waa_compressor_get_reduction_series(waa_batch* batch, uint32_t node, float* dst, uint32_t n_quanta);

/* Levels of the rendered output, computed on the device where the audio lies (the reference hands back f32 planes and nothing
 * else: this is an extension, like waa_download_all_pcm16 and the reduction trace).  Answers, without the f32 download: did a
 * context go non-finite and where, how loud is it overall and over time, how many samples will waa_download_all_pcm16 saturate.
 *
 * A ROW is one (instance i, output channel c): what waa_download(b, i, c, ...) returns, L = length_frames samples in
 * n_q = ceil(L / 128) render quanta; a channel the destination's signal does not carry is a row of zeros.  Every value is defined
 * on the sample's 32 bits, a = bits & 0x7fffffff, e = a >> 23 (e == 255: non-finite; e == 0: zero or denormal), so that nothing
 * depends on what a convert or a compare does with a denormal, and it is exact: a model reproduces it bit for bit
 * (tests/levels_model.py).
 *
 *   p_q  per-quantum peak: the f32 whose bits are the unsigned maximum of `a` over the quantum's frames f < L with e != 255
 *        (a denormal counts with its own bits); 0 when there is none.
 *   e_q  per-quantum energy, f64: s_j = (double)x_j * (double)x_j (exact) for the frames f = 128 q + j < L with 1 <= e <= 254,
 *        +0.0 otherwise; summed by the adjacent-pairs tree in index order (t0[k] = s[2k] + s[2k+1], t1[k] = t0[2k] + t0[2k+1],
 *        ... seven levels), every add f64 round-to-nearest.
 *   peak             max of p_q.
 *   sum_sq           the quanta in blocks of 64 consecutive ones (a missing quantum is +0.0); b_m = the same tree over the block's
 *                    64 e_q (six levels); sum_sq = (...((0.0 + b_0) + b_1) + ...), ascending.
 *   n_nonfinite      frames < L with e == 255;  first_nonfinite: the smallest such frame, UINT64_MAX if none.
 *   n_clipped        frames < L with e != 255 whose f32 product v = x * 32768.f has v > 32767.f or v < -32768.f: the samples
 *                    the clamp of waa_download_all_pcm16 changes (1.0f counts; -1.0f and 32767/32768 do not; a finite x whose
 *                    product overflows to infinity counts).
 * Nothing depends on the grid, the batch size, a row's neighbours or the run; there are no floating-point atomics.
 *
 * waa_output_levels: out[n_instances][n_channels_out].  waa_output_level_series: p_q and e_q, [n_instances][n_channels_out]
 * [n_quanta] each; either pointer may be NULL, not both.  Both compute from the output as it lies on the device when they are
 * called (nothing is cached: after waa_batch_rearm and a new render they give the new render's values) and wait for the render
 * as waa_download_all does.  The workspace (12 bytes per row and quantum, plus 40 per row and 64-quantum block) is allocated on
 * the first call and freed with the batch; a failed allocation is the call's status.  length_frames == 0: WAA_OK, nothing written.
 *
 * waa_download_all_pcm16_gain: waa_download_all_pcm16 with v = x * gain[instance] (one f32 multiply, unfused) in front of the
 * packer's * 32768, clamp, NaN -> 0 and round to nearest even; gain[n_instances] in host memory.  gain[i] == 1 for every i gives
 * the bits of waa_download_all_pcm16.
 *
 * Refusals, in this order: a NULL batch or pointer (WAA_ERR_INVALID_ARGUMENT); a plan-only batch (WAA_ERR_DEVICE); nothing
 * rendered yet, and a ranged render (waa_render_range) in front of its last range (WAA_ERR_INVALID_STATE, InvalidStateError); a
 * non-finite gain[i] (WAA_ERR_INVALID_ARGUMENT, naming the instance).
 * Out of scope: levels of a node other than the destination, loudness weighting, batches merged from single
 * contexts and waa_render_sharded (a `pull` callback may call these functions on its sub-batch). */
typedef struct waa_level_stats {      /* 40 bytes, one per (instance, output channel) */
  double   sum_sq;
  uint64_t n_nonfinite, first_nonfinite, n_clipped;
  float    peak;
  uint32_t reserved;                  /* 0 */
} waa_level_stats;
waa_status waa_output_levels(waa_batch* batch, waa_level_stats* out);
waa_status waa_output_level_series(waa_batch* batch, float* peak, double* sum_sq);
waa_status waa_download_all_pcm16_gain(waa_batch* batch, int16_t* dst, const float* gain);

/* Integrated loudness (ITU-R BS.1770-4 / EBU R 128) of every context's rendered output, computed on the device where the audio
 * lies: an extension like the levels above, and what a data-set pipeline normalises to (-23 LUFS, -16, -14) in front of
 * waa_download_all_pcm16_gain.  The device computes the K-weighted energy of every 100 ms sub-block of every row; blocks, gates and
 * logarithms are host arithmetic on those few doubles, the same code for every source of them (waa_loudness_from_series).
 *
 * Sub-blocks.  A ROW is one (instance, output channel) of L = length_frames frames at sample rate sr.  h = floor(sr / 10 + 0.5)
 *   frames are one sub-block (waa_loudness_hop), n_sub = floor(L / h); frames past n_sub * h belong to no block and are not read.
 * Samples, decided on the bits as above: e == 255 (non-finite) and e == 0 (zero, denormal) enter as +0.0, every other sample as
 *   (double)x; a channel the destination's signal does not carry is a row of zeros.
 * K-weighting: two biquads in f64, coefficients computed on the host in f64 from sr.
 *   Stage 1, the shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / sr),
 *     Vh = 10^(G / 20), Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2;
 *     b0 = (Vh + Vb K / Q + K^2) / a0, b1 = 2 (K^2 - Vh) / a0, b2 = (Vh - Vb K / Q + K^2) / a0,
 *     a1 = 2 (K^2 - 1) / a0, a2 = (1 - K / Q + K^2) / a0.
 *   Stage 2, the high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773; b = (1, -2, 1), not divided by a0; a1, a2 as above.
 *   (At 48 kHz these are the tables of BS.1770-4 to 1e-15.)
 *   Each stage is transposed direct form II, unfused, in this order: v = b0 x + p1;  p1 = (b1 x - a1 v) + p2;  p2 = b2 x - a2 v.
 *   Stage 2 runs on v with its own state (q1, q2) and gives w.  The state is zero at frame 0.
 * Sub-block energy: z[j] = (...((0 + w_0^2) + w_1^2) + ...) over the sub-block's h frames, ascending, f64.
 *   The device computes z in three launches (a zero-state pass per sub-block, a chain over the sub-blocks' states, an exact pass
 *   from the handed-over state), so z is the serial recurrence's value up to the rounding of the hand-over — DESIGN.md 3.14 and
 *   tests/loudness_model.py derive the bound, below 1e-9 of z on ordinary signals — and the same bits whatever the batch, the grid and the run.
 *   A row of zeros gives exact zeros.
 * Channel weights G_c: weights[n_channels_out] if given (finite, >= 0); otherwise by the Web Audio layouts — six channels
 *   (1, 1, 1, 0, 1.41, 1.41), four channels (1, 1, 1.41, 1.41), anything else 1 per channel.
 * Blocks: block k covers sub-blocks k .. k + 3, k = 0 .. n_sub - 4;  P_k = sum_c G_c (z_c[k] + z_c[k+1] + z_c[k+2] + z_c[k+3])
 *   / (4 h);  l_k = -0.691 + 10 log10 P_k, -inf for P_k = 0.
 * integrated: A = the blocks with l_k > -70;  relative_threshold = -0.691 + 10 log10(mean_A P_k) - 10 (-inf when A is empty);
 *   B = the blocks of A with l_k > relative_threshold;  integrated = -0.691 + 10 log10(mean_B P_k), -inf when B is empty (a clip
 *   shorter than 400 ms is one such case).  Means are ascending f64 sums.
 * momentary_max = max l_k.  short_term_max: the same formula over windows of 30 sub-blocks, hop one sub-block, ungated; -inf when
 *   n_sub < 30.  n_blocks = max(n_sub - 3, 0), n_gated = |B|.
 *
 * waa_output_loudness: out[n_instances]; weights may be NULL.  waa_output_loudness_series: z[n_instances][n_channels_out][n_sub].
 * Both compute from the output as it lies on the device when they are called (nothing is cached) and wait for the render as
 * waa_download_all does.  The workspace (4 + 4 + 1 doubles per row and sub-block) is the batch's own, allocated on the first call
 * and freed with the batch; a failed allocation is the call's status.  length_frames < h: WAA_OK, every field -inf / 0, no z written.
 * waa_loudness_hop: h of a sample rate.
 * waa_loudness_from_series: the blocks, gates and maxima of ONE context from its z[n_channels][n_sub] in host memory — no batch, no
 * device; the code waa_output_loudness gates with.  For jobs that hold z from elsewhere: a `pull` callback of waa_render_sharded,
 * contexts rendered one by one.  A NULL z (with something to read) or out, hop == 0 and a bad weight are WAA_ERR_INVALID_ARGUMENT.
 *
 * Refusals of the two batch calls, in this order: those of waa_output_levels, in its order and wording; then a negative or
 * non-finite weight (WAA_ERR_INVALID_ARGUMENT, naming the channel).
 * Out of scope: true peak, loudness range, dual-mono, batches merged from single contexts and
 * waa_render_sharded (beyond what waa_loudness_from_series allows in a `pull` callback). */
typedef struct waa_loudness_stats {   /* 40 bytes, one per instance */
  double   integrated, momentary_max, short_term_max, relative_threshold;   /* LUFS */
  uint32_t n_blocks, n_gated;
} waa_loudness_stats;
waa_status waa_output_loudness(waa_batch* batch, const double* weights /* NULL: default */, waa_loudness_stats* out);
waa_status waa_output_loudness_series(waa_batch* batch, double* z);
uint32_t waa_loudness_hop(double sample_rate);
waa_status waa_loudness_from_series(const double* z, uint32_t n_channels, uint32_t n_sub, uint32_t hop, const double* weights,
                                    waa_loudness_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* WAA_HIP_DEVICE_H */
