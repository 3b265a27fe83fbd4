// What the host side of every image stage does the same way: the HIP error check, the synchronise-and-check tail, the two-event timer behind
// vdo_xx_last_timing, the staging of a row-strided image and the refusals whose text differs only in a noun.  Plain functions and one small struct:
// a handle stays the plain struct it is and holds a StageTimer by value.  Nothing here queues anything a caller does not ask for by name.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"
#include "frame_images.hpp"

namespace vdo {

constexpr int64_t kMaxPixels = int64_t(1) << 26;
constexpr int kMaxImageSide = 1 << 24;                                     // (float)(W - 1) and (float)x are exact

inline int check_hip(const char* who, hipError_t e) { return e == hipSuccess ? VDO_OK : set_error(VDO_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e)); }

// the end of an entry point: wait for the stream, then what a launch may have left behind
inline int sync_check(const char* who, hipStream_t s) {
  hipError_t e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipGetLastError();
  return check_hip(who, e);
}

inline bool is_finite(float v) { return std::fabs(v) <= FLT_MAX; }         // the host twin of dn_finite: false for NaN and the infinities

using StageClock = std::chrono::steady_clock;

inline double elapsed_ms(hipEvent_t from, hipEvent_t to) {
  float ms = 0.f;
  hipEventElapsedTime(&ms, from, to);
  return ms;
}

// ms[0]: the host's wall time of the last call from its begin(); ms[1]: the device time between the two events
struct StageTimer {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double ms[2] = {0, 0};
  bool create() { return hipEventCreate(&ev0) == hipSuccess && hipEventCreate(&ev1) == hipSuccess; }
  void destroy() {
    if (ev0) hipEventDestroy(ev0);
    if (ev1) hipEventDestroy(ev1);
  }
  StageClock::time_point begin(hipStream_t s) {
    const auto t0 = StageClock::now();
    hipEventRecord(ev0, s);
    return t0;
  }
  void mark_end(hipStream_t s) { hipEventRecord(ev1, s); }
  void finish(StageClock::time_point t0, double dev_ms) {
    ms[0] = std::chrono::duration<double, std::milli>(StageClock::now() - t0).count();
    ms[1] = dev_ms;
  }
  void finish(StageClock::time_point t0) { finish(t0, elapsed_ms(ev0, ev1)); }     // after the stream was waited for
};

// the body of every vdo_xx_last_timing; t is null when the handle is
inline int last_timing(const char* who, const StageTimer* t, double ms[2]) {
  if (!t || !ms) return set_error(VDO_ERR_INVALID, "%s: %s is null", who, !t ? "handle" : "ms");
  ms[0] = t->ms[0]; ms[1] = t->ms[1];
  return VDO_OK;
}

// Where a kernel reads an image of H rows of `row` elements that the caller gave with `stride` elements from row to row: a packed device image
// (at a multiple of `align` bytes) is read where it lies, anything else is copied on the stream to `packed` first.
template <class T>
inline const T* stage_rows(hipStream_t s, T* packed, const T* src, int64_t stride, int row, int H, int src_is_device, size_t align = 1) {
  if (src_is_device && stride == row && ((uintptr_t)src & (align - 1)) == 0) return src;
  hipMemcpy2DAsync(packed, row * sizeof(T), src, (size_t)stride * sizeof(T), row * sizeof(T), H, src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s);
  return packed;
}

// name: "K" or "Km"
inline int check_intrinsics(const char* who, const char* name, const float K[4]) {
  for (int k = 0; k < 4; ++k) if (!is_finite(K[k])) return set_error(VDO_ERR_INVALID, "%s: %s[%d] is not finite", who, name, k);
  if (!(K[0] > 0.f) || !(K[1] > 0.f)) return set_error(VDO_ERR_INVALID, "%s: %s: fx %g, fy %g must be positive", who, name, (double)K[0], (double)K[1]);
  return VDO_OK;
}

inline int check_depth_range(const char* who, float min_depth, float max_depth) {
  if (!is_finite(min_depth) || !(min_depth >= 0.f)) return set_error(VDO_ERR_INVALID, "%s: min_depth %g must be finite and >= 0", who, (double)min_depth);
  if (!is_finite(max_depth) || !(max_depth > min_depth)) return set_error(VDO_ERR_INVALID, "%s: max_depth %g must be finite and above min_depth %g", who, (double)max_depth, (double)min_depth);
  return VDO_OK;
}

// what: "width x height =" or "the model of"
inline int check_image_size(const char* who, const char* what, int W, int H) {
  if ((int64_t)W * H > kMaxPixels || W > kMaxImageSide || H > kMaxImageSide)
    return set_error(VDO_ERR_UNSUPPORTED, "%s: %s %d x %d exceeds 2^26 pixels or 2^24 on a side", who, what, W, H);
  return VDO_OK;
}

// a call's depth and mask images of width W, before anything is queued; a mask that is not required may be null
inline int check_depth_mask(const char* who, int W, const float* depth, int64_t ds, const int32_t* mask, int64_t ms, bool mask_required) {
  if (!depth) return set_error(VDO_ERR_INVALID, "%s: depth is null", who);
  if (mask_required && !mask) return set_error(VDO_ERR_INVALID, "%s: mask is null", who);
  if (ds < W) return set_error(VDO_ERR_INVALID, "%s: depth_stride_floats %lld smaller than the width %d", who, (long long)ds, W);
  if (mask && ms < W) return set_error(VDO_ERR_INVALID, "%s: mask_stride_ints %lld smaller than the width %d", who, (long long)ms, W);
  return VDO_OK;
}

// whose: "the mapper's", "the stage's" or "the aligner's"
inline int check_frame(const char* who, const vdo_frame_images* f, int W, int H, const char* whose) {
  if (!f) return set_error(VDO_ERR_INVALID, "%s: frame is null", who);
  if (f->w != W || f->h != H) return set_error(VDO_ERR_INVALID, "%s: frame is %d x %d, %s images are %d x %d", who, f->w, f->h, whose, W, H);
  return VDO_OK;
}

}  // namespace vdo
