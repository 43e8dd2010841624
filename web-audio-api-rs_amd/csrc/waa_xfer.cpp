// waa_xfer.cpp — transfers between CALLER memory and the device, and the deferred fills of whole-batch source buffers.
// Pinned caller memory (hipHostMalloc / hipHostRegister: what a host that cares about the link hands over — bench.py, the sharded
// path) is copied directly.  PAGEABLE caller memory (a numpy array, a Rust Vec) goes through a pinned block of the batch: the runtime
// would otherwise lock the caller's pages on the fly and let its copy kernels read / write them in place — and a destination that
// has just been mapped and never touched (numpy's np.empty, a fresh Vec) is exactly what the round-6 campaigns saw go wrong under
// several processes (one download that never arrived: a render "of zeros"; "Memory access fault by GPU ... Write access to a
// read-only page").  Through the staging block the GPU only ever touches memory this library pinned.
#include "waa_host.hpp"

namespace waa {
namespace host {

namespace {
constexpr size_t STAGE_BYTES = 8u << 20;
bool caller_memory_is_pinned(const void* p) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost;
}
int stage_of(waa_batch* b, char** out) {
  if (!b->stage) HIP_TRY(hipHostMalloc(&b->stage, STAGE_BYTES, hipHostMallocDefault));
  *out = static_cast<char*>(b->stage);
  return 0;
}
}  // namespace
int xfer_h2d(waa_batch* b, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height) {
  if (!width || !height) return 0;
  if (caller_memory_is_pinned(src)) {
    if (dpitch == width && spitch == width)
      HIP_TRY(hipMemcpyAsync(dst, src, width * height, hipMemcpyHostToDevice, b->stream));
    else
      HIP_TRY(copy2d_async(b->device, dst, dpitch, src, spitch, width, height, hipMemcpyHostToDevice, b->stream));
    return 0;
  }
  char* st = nullptr;
  if (int e = stage_of(b, &st)) return e;
  for (size_t r = 0; r < height;) {
    if (width > STAGE_BYTES) {  // a row longer than the block: in pieces
      for (size_t o = 0; o < width; o += STAGE_BYTES) {
        const size_t n = std::min(STAGE_BYTES, width - o);
        std::memcpy(st, static_cast<const char*>(src) + r * spitch + o, n);
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(dst) + r * dpitch + o, st, n, hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
      }
      r++;
      continue;
    }
    const size_t rows = std::min(height - r, STAGE_BYTES / width);
    for (size_t k = 0; k < rows; k++) std::memcpy(st + k * width, static_cast<const char*>(src) + (r + k) * spitch, width);
    if (dpitch == width)
      HIP_TRY(hipMemcpyAsync(static_cast<char*>(dst) + r * dpitch, st, rows * width, hipMemcpyHostToDevice, b->stream));
    else
      HIP_TRY(copy2d_async(b->device, static_cast<char*>(dst) + r * dpitch, dpitch, st, width, width, rows, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    r += rows;
  }
  return 0;
}
int xfer_d2h(waa_batch* b, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height) {
  if (!width || !height) return 0;
  if (caller_memory_is_pinned(dst)) {
    if (dpitch == width && spitch == width)
      HIP_TRY(hipMemcpyAsync(dst, src, width * height, hipMemcpyDeviceToHost, b->stream));
    else
      HIP_TRY(copy2d_async(b->device, dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost, b->stream));
    return 0;
  }
  char* st = nullptr;
  if (int e = stage_of(b, &st)) return e;
  for (size_t r = 0; r < height;) {
    if (width > STAGE_BYTES) {
      for (size_t o = 0; o < width; o += STAGE_BYTES) {
        const size_t n = std::min(STAGE_BYTES, width - o);
        HIP_TRY(hipMemcpyAsync(st, static_cast<const char*>(src) + r * spitch + o, n, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        std::memcpy(static_cast<char*>(dst) + r * dpitch + o, st, n);
      }
      r++;
      continue;
    }
    const size_t rows = std::min(height - r, STAGE_BYTES / width);
    if (spitch == width)
      HIP_TRY(hipMemcpyAsync(st, static_cast<const char*>(src) + r * spitch, rows * width, hipMemcpyDeviceToHost, b->stream));
    else
      HIP_TRY(copy2d_async(b->device, st, width, static_cast<const char*>(src) + r * spitch, spitch, width, rows, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (size_t k = 0; k < rows; k++) std::memcpy(static_cast<char*>(dst) + (r + k) * dpitch, st + k * width, width);
    r += rows;
  }
  return 0;
}

// The data movement of a batch-wide source buffer (waa_source_set_buffer_batch / _pcm16_batch), apart from its allocation:
// waa_render_sharded registers the buffers first, plans, and fills them when the sub-batch has its turn on the link.
int fill_upload(waa_batch* b, const waa_batch::PendingFill& f) {
  if (f.kind == 0) {
    // on the batch's own stream (and waited for: the caller may free `data` on return): blocking copies on the null
    // stream of several host threads serialise, and the upload of one sub-batch could not overlap the download of
    // another (PCIe is full duplex) — SURVEY 8(e)
    // (contiguous on both sides -> a plain 1-D copy: those go through the DMA engines, one per direction; pitched 2-D
    // copies run as a copy kernel and did not overlap with a download on another stream)
    if (int e = xfer_h2d(b, f.planes, f.stride * sizeof(float), f.host, f.frames * sizeof(float), f.frames * sizeof(float), (size_t)f.n_items * f.n_ch))
      return e;
    HIP_TRY(hipStreamSynchronize(b->stream));
    return 0;
  }
  const size_t bytes = (size_t)f.n_items * f.frames * f.n_ch * sizeof(int16_t);
  if (int e = xfer_h2d(b, f.staging, bytes, f.host, bytes, bytes, 1)) return e;
  hipError_t he = hipSuccess;
  {
    const bool same = std::fabs(f.src_sr - b->sr) <= 0.1f;
    waa::DecodeDesc dd{};
    dd.pcm = f.staging;
    dd.out = f.planes;
    dd.frames = f.frames;
    dd.target_frames = f.target;
    dd.out_item_stride = (uint64_t)f.n_ch * f.stride;
    dd.out_ch_stride = f.stride;
    dd.nch = f.n_ch;
    dd.n_items = f.n_items;
    dd.resample = same ? 0 : 1;
    dd.scale = 1.f;
    waa::launch_pcm16_resample(dd, b->stream);
    he = hipGetLastError();
  }
  if (he == hipSuccess) he = hipStreamSynchronize(b->stream);
  if (he != hipSuccess) return fail(WAA_ERR_DEVICE, "HIP error %s in the PCM decode path", hipGetErrorString(he));
  return 0;
}
int fill_pending_uploads(waa_batch* b) {
  HIP_TRY(hipSetDevice(b->device));
  for (const auto& f : b->pending_fills)
    if (int e = fill_upload(b, f)) return e;
  b->pending_fills.clear();
  return 0;
}

}  // namespace host
}  // namespace waa
