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

#ifdef __cplusplus
}
#endif

#endif /* WAA_HIP_DEVICE_H */
