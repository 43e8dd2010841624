// waa_output_calls.hpp — what the calls that read the rendered output where it lies share (waa_levels_host.cpp,
// waa_loudness_host.cpp): their refusals, their wait for the render and their launches.
#pragma once
#include "waa_host.hpp"

namespace waa {
namespace host {

// the checks these calls share, in the order and wording of waa_download_all_pcm16 and waa_download
inline int check_rendered(waa_batch* b) {
  if (b->dry) return fail(WAA_ERR_DEVICE, "plan-only batch has no device");
  if (!b->planned || !b->rendered) return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - nothing rendered yet");
  if (b->ranged && b->ctl_q < b->n_quanta)
    return fail(WAA_ERR_INVALID_STATE, "InvalidStateError - a ranged render is in progress (suspended in front of quantum %u): the output is complete "
                                       "once the last range is rendered", b->ctl_q);
  return 0;
}
// a launch made at call time, like an analyser pull: it gets its profile slot when it is first made on a profiled batch, so the
// profile of a batch that never asks for its levels or its loudness lists what it always listed
template <typename L>
int call_launch(waa_batch* b, const char* name, L&& launch) {
  return timed(b, b->profiling ? slot_for(b, name) : -1, launch);
}
inline int wait_for_render(waa_batch* b) {
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return settle_loops(b);
}

}  // namespace host
}  // namespace waa
