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

#ifdef __cplusplus
}
#endif

#endif /* WAA_HIP_DEVICE_H */
