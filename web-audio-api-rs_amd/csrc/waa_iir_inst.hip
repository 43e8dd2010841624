// waa_iir_inst.hip — the per-instance forms of the streaming IIR kernels (one coefficient set per instance of the batch,
// waa_iir_set_coefficients_instance): iir_stream_kernel<NS, true> and iir_lane_kernel<NS, true> for NS = 1..19, iir_row_kernel<M, true>, instantiated from
// waa_iir_stream.hip into a code object of their own (see the note above its launchers).
#define WAA_IIR_PER_INST_TU
#include "waa_iir_stream.hip"
