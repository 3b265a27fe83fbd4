// Stereo rectifier: the raw 8-bit images of one or two cameras become the rectified grey images the stereo and flow matchers take.  The reference's
// stereo example does this with cv::initUndistortRectifyMap + cv::remap before its System sees an image; the semantics here are this library's own,
// stated in include/vdo_slam_hip.h (vdo_rectify_plan, vdo_rectify_compute) and restated in NumPy by tests/rectify_ref.py.  The map is planned on the
// host in fp64 (rectify_plan.hpp); everything below is integer arithmetic, and no result depends on workgroup shape or order.
//
//   k_rect_remap   up to 4 jobs in one launch (blockIdx.z = job).  One thread makes 4 consecutive destination pixels: two 16-byte loads of the
//                  map (the device map's rows are padded to a multiple of 4 entries, the pad holding the invalid sentinel, so the loads are aligned
//                  and never conditional), four gathered taps per pixel - neighbouring lanes gather neighbouring source bytes - the grey conversion
//                  of a colour tap fused in, one 32-bit store when the destination address is 4-aligned and the row has 4 pixels left, else bytes.
//                  Validity is re-derived here from (qx, qy) and the source size in the job's mode: no map can make it read outside the source.
//   k_rect_gate    image = 0.0f where the validity image is 0; counts the values it changed by wave ballot and one integer atomic per wave.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"
#include "rectify_plan.hpp"
#include "stage.hpp"

namespace vdo {

constexpr int kRectMaxJobs = 4, kRectMaxCams = 2;
constexpr int kRectBX = 64, kRectBY = 4;                  // 256 threads: 64 x 4 threads = 256 x 4 destination pixels

struct RectJobDev {
  const uint8_t* src; int64_t src_stride;
  uint8_t* dst; int64_t dst_stride;
  const int32_t* map;                                     // [H][Wp][2]
  int32_t ws, hs, channels, rgb_order, nearest;
};
struct RectLaunch { RectJobDev job[kRectMaxJobs]; };

}  // namespace vdo

struct vdo_rectify {
  vdo_ctx* ctx = nullptr;
  int W = 0, H = 0, Wp = 0, n_cams = 0;
  int ws[vdo::kRectMaxCams] = {0, 0}, hs[vdo::kRectMaxCams] = {0, 0};
  size_t stage_bytes = 0;
  int32_t* d_map[vdo::kRectMaxCams] = {nullptr, nullptr};           // [H][Wp][2], Wp = W rounded up to 4
  uint8_t* d_valid[vdo::kRectMaxCams] = {nullptr, nullptr};         // [H][W]
  uint8_t* d_src[vdo::kRectMaxJobs] = {nullptr, nullptr, nullptr, nullptr};
  uint8_t* d_dst[vdo::kRectMaxJobs] = {nullptr, nullptr, nullptr, nullptr};
  float* d_gate = nullptr;                                          // [H][W] staging of a host image of the gate
  int32_t* d_count = nullptr;
  int32_t* h_count = nullptr;                                       // pinned
  std::vector<int32_t> map[vdo::kRectMaxCams];                      // host copies [H][W][2]
  std::vector<uint8_t> valid[vdo::kRectMaxCams];
  int32_t n_valid[vdo::kRectMaxCams] = {0, 0};
  vdo::StageTimer tm;
};

namespace vdo {

// K2's arithmetic (k_rgb2gray, orb.hip) on one tap
__device__ __forceinline__ int rect_tap(const uint8_t* __restrict__ row, int x, int ch, int rgb_order) {
  if (ch == 1) return row[x];
  const uint8_t* p = row + (int64_t)x * ch;
  const int r = rgb_order ? p[0] : p[2], g = p[1], b = rgb_order ? p[2] : p[0];
  return (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14;
}

// One destination pixel.  Every read below is guarded by the test in front of it: 0 <= ix, ix + (ax > 0) <= ws - 1 and the same in y.
__device__ __forceinline__ int rect_pixel(const RectJobDev& j, int qx, int qy, int border) {
  if (j.nearest) {
    const int x = (int)(((int64_t)qx + 16) >> 5), y = (int)(((int64_t)qy + 16) >> 5);
    if (x < 0 || y < 0 || x >= j.ws || y >= j.hs) return border;
    return j.src[(int64_t)y * j.src_stride + x];
  }
  const int ix = qx >> 5, ax = qx & 31, iy = qy >> 5, ay = qy & 31;
  if (ix < 0 || iy < 0 || ix + (ax > 0) > j.ws - 1 || iy + (ay > 0) > j.hs - 1) return border;
  const uint8_t* r0 = j.src + (int64_t)iy * j.src_stride;
  int acc = (32 - ax) * (32 - ay) * rect_tap(r0, ix, j.channels, j.rgb_order) + 512;
  if (ax) acc += ax * (32 - ay) * rect_tap(r0, ix + 1, j.channels, j.rgb_order);
  if (ay) {
    const uint8_t* r1 = r0 + j.src_stride;
    acc += (32 - ax) * ay * rect_tap(r1, ix, j.channels, j.rgb_order);
    if (ax) acc += ax * ay * rect_tap(r1, ix + 1, j.channels, j.rgb_order);
  }
  return acc >> 10;
}

__global__ __launch_bounds__(kRectBX* kRectBY) void k_rect_remap(const RectLaunch L, int W, int H, int Wp, int border) {
  const RectJobDev& j = L.job[blockIdx.z];
  const int x0 = 4 * (blockIdx.x * kRectBX + threadIdx.x), y = blockIdx.y * kRectBY + threadIdx.y;
  if (x0 >= W || y >= H) return;
  const int4* m = reinterpret_cast<const int4*>(j.map + ((int64_t)y * Wp + x0) * 2);       // 32-byte aligned: Wp and x0 are multiples of 4
  const int4 a = m[0], b = m[1];
  uint8_t* d = j.dst + (int64_t)y * j.dst_stride + x0;
  const int n = min(4, W - x0);
  int v[4];
  v[0] = rect_pixel(j, a.x, a.y, border);
  v[1] = n > 1 ? rect_pixel(j, a.z, a.w, border) : 0;
  v[2] = n > 2 ? rect_pixel(j, b.x, b.y, border) : 0;
  v[3] = n > 3 ? rect_pixel(j, b.z, b.w, border) : 0;
  if (n == 4 && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
    *reinterpret_cast<uint32_t*>(d) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
  } else {
    for (int k = 0; k < n; ++k) d[k] = (uint8_t)v[k];
  }
}

__global__ __launch_bounds__(256) void k_rect_gate(const uint8_t* __restrict__ valid, int W, int H, float* __restrict__ img, int64_t stride, int32_t* __restrict__ count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool changed = false;
  if (i < W * H && !valid[i]) {
    const int y = i / W, x = i - y * W;
    float* p = img + (int64_t)y * stride + x;
    changed = __float_as_uint(*p) != 0u;
    *p = 0.0f;
  }
  const unsigned long long b = __ballot(changed);
  if ((threadIdx.x & (warpSize - 1)) == 0 && b) atomicAdd(count, (int32_t)__popcll(b));
}

static void rect_free(vdo_rectify* h) {
  for (int c = 0; c < kRectMaxCams; ++c) { hipFree(h->d_map[c]); hipFree(h->d_valid[c]); }
  for (int k = 0; k < kRectMaxJobs; ++k) { hipFree(h->d_src[k]); hipFree(h->d_dst[k]); }
  hipFree(h->d_gate); hipFree(h->d_count);
  if (h->h_count) hipHostFree(h->h_count);
  h->tm.destroy();
  delete h;
}

static int rect_check_sizes(const char* who, int W, int H, int n_cams, const int* ws, const int* hs) {
  if ((int64_t)W * H > kRectMaxPixels) return set_error(VDO_ERR_UNSUPPORTED, "%s: width x height = %d x %d exceeds 2^26 pixels", who, W, H);
  for (int c = 0; c < n_cams; ++c)
    if ((int64_t)ws[c] * hs[c] > kRectMaxPixels) return set_error(VDO_ERR_UNSUPPORTED, "%s: source %d of %d x %d exceeds 2^26 pixels", who, c, ws[c], hs[c]);
  return VDO_OK;
}

// the handle from host maps [H][W][2] already in h->map, validity in h->valid: every device allocation and the uploads
static int rect_build(const char* who, vdo_ctx* ctx, vdo_rectify* h, vdo_rectify** out) {
  int rc = ctx_bind(ctx);
  if (rc != VDO_OK) { delete h; return rc; }
  h->ctx = ctx;
  const int W = h->W, H = h->H, Wp = (W + 3) & ~3;
  h->Wp = Wp;
  const size_t n = (size_t)W * H;
  size_t src_px = 0;
  for (int c = 0; c < h->n_cams; ++c) src_px = std::max(src_px, (size_t)h->ws[c] * h->hs[c]);
  h->stage_bytes = src_px * 4;
  bool ok = true;
  for (int c = 0; c < h->n_cams && ok; ++c)
    ok = hipMalloc((void**)&h->d_map[c], (size_t)H * Wp * 2 * sizeof(int32_t)) == hipSuccess && hipMalloc((void**)&h->d_valid[c], n) == hipSuccess;
  for (int k = 0; k < kRectMaxJobs && ok; ++k) ok = hipMalloc((void**)&h->d_src[k], h->stage_bytes) == hipSuccess && hipMalloc((void**)&h->d_dst[k], n) == hipSuccess;
  ok = ok && hipMalloc((void**)&h->d_gate, n * sizeof(float)) == hipSuccess && hipMalloc((void**)&h->d_count, sizeof(int32_t)) == hipSuccess &&
       hipHostMalloc((void**)&h->h_count, sizeof(int32_t), hipHostMallocDefault) == hipSuccess && h->tm.create();
  if (!ok) {
    (void)hipGetLastError();
    rect_free(h);
    return set_error(VDO_ERR_OOM, "%s: device allocation failed for %d x %d", who, W, H);
  }
  hipStream_t s = ctx->stream;
  std::vector<int32_t> padded((size_t)H * Wp * 2, kRectInvalid);
  hipError_t e = hipSuccess;
  for (int c = 0; c < h->n_cams && e == hipSuccess; ++c) {
    for (int y = 0; y < H; ++y) std::memcpy(padded.data() + (size_t)y * Wp * 2, h->map[c].data() + (size_t)y * W * 2, (size_t)W * 2 * sizeof(int32_t));
    e = hipMemcpyAsync(h->d_map[c], padded.data(), padded.size() * sizeof(int32_t), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h->d_valid[c], h->valid[c].data(), n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);       // `padded` is reused by the next camera
  }
  if (e != hipSuccess) { rect_free(h); return check_hip(who, e); }
  *out = h;
  return VDO_OK;
}

}  // namespace vdo

using namespace vdo;

extern "C" int vdo_rectify_plan(const vdo_rectify_params* p, int cam, int32_t* map, uint8_t* valid, int32_t* n_valid) {
  static const char* who = "vdo_rectify_plan";
  char msg[160];
  if (rect_check_params(p, cam == -1 ? -2 : cam, msg, sizeof msg)) return set_error(VDO_ERR_INVALID, "%s: %s", who, msg);
  if (!map) return set_error(VDO_ERR_INVALID, "%s: map is null", who);
  const int ws[2] = {p->cam[0].src_width, p->cam[1].src_width}, hs[2] = {p->cam[0].src_height, p->cam[1].src_height};
  const int rc = rect_check_sizes(who, p->width, p->height, p->n_cams, ws, hs);
  if (rc != VDO_OK) return rc;
  rect_plan_map(p, cam, map, valid, n_valid);
  return VDO_OK;
}

extern "C" int vdo_rectify_create(vdo_ctx* ctx, const vdo_rectify_params* p, vdo_rectify** out) {
  static const char* who = "vdo_rectify_create";
  if (!ctx) return set_error(VDO_ERR_INVALID, "%s: ctx is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  char msg[160];
  if (rect_check_params(p, -1, msg, sizeof msg)) return set_error(VDO_ERR_INVALID, "%s: %s", who, msg);
  const int ws[2] = {p->cam[0].src_width, p->cam[1].src_width}, hs[2] = {p->cam[0].src_height, p->cam[1].src_height};
  const int rc = rect_check_sizes(who, p->width, p->height, p->n_cams, ws, hs);
  if (rc != VDO_OK) return rc;
  vdo_rectify* h = new vdo_rectify;
  h->W = p->width; h->H = p->height; h->n_cams = p->n_cams;
  const size_t n = (size_t)h->W * h->H;
  for (int c = 0; c < p->n_cams; ++c) {
    h->ws[c] = ws[c]; h->hs[c] = hs[c];
    h->map[c].resize(2 * n); h->valid[c].resize(n);
    rect_plan_map(p, c, h->map[c].data(), h->valid[c].data(), &h->n_valid[c]);
  }
  return rect_build(who, ctx, h, out);
}

extern "C" int vdo_rectify_create_from_maps(vdo_ctx* ctx, int width, int height, int n_cams, const int32_t* const* maps, const int32_t* src_width,
                                            const int32_t* src_height, vdo_rectify** out) {
  static const char* who = "vdo_rectify_create_from_maps";
  if (!ctx) return set_error(VDO_ERR_INVALID, "%s: ctx is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (width < 1) return set_error(VDO_ERR_INVALID, "%s: width %d < 1", who, width);
  if (height < 1) return set_error(VDO_ERR_INVALID, "%s: height %d < 1", who, height);
  if (n_cams < 1 || n_cams > kRectMaxCams) return set_error(VDO_ERR_INVALID, "%s: n_cams %d outside 1..2", who, n_cams);
  if (!maps || !src_width || !src_height) return set_error(VDO_ERR_INVALID, "%s: %s is null", who, !maps ? "maps" : !src_width ? "src_width" : "src_height");
  for (int c = 0; c < n_cams; ++c) {
    if (!maps[c]) return set_error(VDO_ERR_INVALID, "%s: maps[%d] is null", who, c);
    if (src_width[c] < 1) return set_error(VDO_ERR_INVALID, "%s: src_width[%d] %d < 1", who, c, src_width[c]);
    if (src_height[c] < 1) return set_error(VDO_ERR_INVALID, "%s: src_height[%d] %d < 1", who, c, src_height[c]);
  }
  const int rc = rect_check_sizes(who, width, height, n_cams, src_width, src_height);
  if (rc != VDO_OK) return rc;
  vdo_rectify* h = new vdo_rectify;
  h->W = width; h->H = height; h->n_cams = n_cams;
  const size_t n = (size_t)width * height;
  for (int c = 0; c < n_cams; ++c) {
    h->ws[c] = src_width[c]; h->hs[c] = src_height[c];
    h->map[c].assign(maps[c], maps[c] + 2 * n);
    h->valid[c].resize(n);
    int32_t count = 0;
    for (size_t i = 0; i < n; ++i) { const bool v = rect_map_valid(maps[c][2 * i], maps[c][2 * i + 1], h->ws[c], h->hs[c]); h->valid[c][i] = v; count += v; }
    h->n_valid[c] = count;
  }
  return rect_build(who, ctx, h, out);
}

extern "C" int vdo_rectify_destroy(vdo_rectify* h) {
  if (!h) return VDO_OK;
  if (ctx_bind(h->ctx) == VDO_OK) hipStreamSynchronize(h->ctx->stream);
  rect_free(h);
  return VDO_OK;
}

extern "C" int vdo_rectify_compute(vdo_rectify* h, const vdo_rectify_job* jobs, int n_jobs, int src_is_device, int dst_is_device, int border) {
  static const char* who = "vdo_rectify_compute";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!jobs) return set_error(VDO_ERR_INVALID, "%s: jobs is null", who);
  if (n_jobs < 1 || n_jobs > kRectMaxJobs) return set_error(VDO_ERR_INVALID, "%s: n_jobs %d outside 1..4", who, n_jobs);
  if (border < 0 || border > 255) return set_error(VDO_ERR_INVALID, "%s: border %d outside 0..255", who, border);
  for (int k = 0; k < n_jobs; ++k) {
    const vdo_rectify_job& j = jobs[k];
    if (!j.src) return set_error(VDO_ERR_INVALID, "%s: jobs[%d].src is null", who, k);
    if (!j.dst) return set_error(VDO_ERR_INVALID, "%s: jobs[%d].dst is null", who, k);
    if (j.cam < 0 || j.cam >= h->n_cams) return set_error(VDO_ERR_INVALID, "%s: jobs[%d].cam %d outside 0..%d", who, k, j.cam, h->n_cams - 1);
    if (j.channels != 1 && j.channels != 3 && j.channels != 4) return set_error(VDO_ERR_INVALID, "%s: jobs[%d].channels %d is not 1, 3 or 4", who, k, j.channels);
    if (j.nearest && j.channels != 1) return set_error(VDO_ERR_INVALID, "%s: jobs[%d].nearest with %d channels (one channel only)", who, k, j.channels);
    if (j.src_stride < (int64_t)h->ws[j.cam] * j.channels)
      return set_error(VDO_ERR_INVALID, "%s: jobs[%d].src_stride %lld smaller than the row of %d x %d bytes", who, k, (long long)j.src_stride, h->ws[j.cam], j.channels);
    if (j.dst_stride < h->W) return set_error(VDO_ERR_INVALID, "%s: jobs[%d].dst_stride %lld smaller than the width %d", who, k, (long long)j.dst_stride, h->W);
  }
  int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const int W = h->W, H = h->H;
  const auto t0 = h->tm.begin(s);
  RectLaunch L{};
  for (int k = 0; k < n_jobs; ++k) {
    const vdo_rectify_job& j = jobs[k];
    RectJobDev& d = L.job[k];
    const int ws = h->ws[j.cam], hs = h->hs[j.cam];
    d.map = h->d_map[j.cam]; d.ws = ws; d.hs = hs; d.channels = j.channels; d.rgb_order = j.rgb_order != 0; d.nearest = j.nearest != 0;
    if (src_is_device) { d.src = j.src; d.src_stride = j.src_stride; }
    else {
      const size_t row = (size_t)ws * j.channels;                                      // row * hs <= stage_bytes: channels <= 4
      hipMemcpy2DAsync(h->d_src[k], row, j.src, (size_t)j.src_stride, row, hs, hipMemcpyHostToDevice, s);
      d.src = h->d_src[k]; d.src_stride = (int64_t)row;
    }
    if (dst_is_device) { d.dst = j.dst; d.dst_stride = j.dst_stride; }
    else { d.dst = h->d_dst[k]; d.dst_stride = W; }
  }
  const dim3 grid(((W + 3) / 4 + kRectBX - 1) / kRectBX, (H + kRectBY - 1) / kRectBY, n_jobs);
  hipLaunchKernelGGL(k_rect_remap, grid, dim3(kRectBX, kRectBY), 0, s, L, W, H, h->Wp, border);
  h->tm.mark_end(s);
  if (!dst_is_device)
    for (int k = 0; k < n_jobs; ++k) hipMemcpy2DAsync(jobs[k].dst, (size_t)jobs[k].dst_stride, h->d_dst[k], W, W, H, hipMemcpyDeviceToHost, s);
  rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  h->tm.finish(t0);
  return VDO_OK;
}

extern "C" int vdo_rectify_gate(vdo_rectify* h, int cam, float* image, int64_t stride_floats, int is_device, int32_t* n_cleared) {
  static const char* who = "vdo_rectify_gate";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (cam < 0 || cam >= h->n_cams) return set_error(VDO_ERR_INVALID, "%s: cam %d outside 0..%d", who, cam, h->n_cams - 1);
  if (!image) return set_error(VDO_ERR_INVALID, "%s: image is null", who);
  if (stride_floats < h->W) return set_error(VDO_ERR_INVALID, "%s: stride_floats %lld smaller than the width %d", who, (long long)stride_floats, h->W);
  if (!n_cleared) return set_error(VDO_ERR_INVALID, "%s: n_cleared is null", who);
  int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const int W = h->W, H = h->H, n = W * H;
  const size_t rowb = (size_t)W * sizeof(float);
  const auto t0 = h->tm.begin(s);
  hipMemsetAsync(h->d_count, 0, sizeof(int32_t), s);
  float* d = image; int64_t stride = stride_floats;
  if (!is_device) { hipMemcpy2DAsync(h->d_gate, rowb, image, (size_t)stride_floats * sizeof(float), rowb, H, hipMemcpyHostToDevice, s); d = h->d_gate; stride = W; }
  hipLaunchKernelGGL(k_rect_gate, dim3((n + 255) / 256), dim3(256), 0, s, (const uint8_t*)h->d_valid[cam], W, H, d, stride, h->d_count);
  h->tm.mark_end(s);
  if (!is_device) hipMemcpy2DAsync(image, (size_t)stride_floats * sizeof(float), h->d_gate, rowb, rowb, H, hipMemcpyDeviceToHost, s);
  hipMemcpyAsync(h->h_count, h->d_count, sizeof(int32_t), hipMemcpyDeviceToHost, s);
  rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  h->tm.finish(t0);
  *n_cleared = *h->h_count;
  return VDO_OK;
}

extern "C" int vdo_rectify_get_map(vdo_rectify* h, int cam, int32_t* map) {
  static const char* who = "vdo_rectify_get_map";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (cam < 0 || cam >= h->n_cams) return set_error(VDO_ERR_INVALID, "%s: cam %d outside 0..%d", who, cam, h->n_cams - 1);
  if (!map) return set_error(VDO_ERR_INVALID, "%s: map is null", who);
  std::memcpy(map, h->map[cam].data(), h->map[cam].size() * sizeof(int32_t));
  return VDO_OK;
}

extern "C" int vdo_rectify_get_valid(vdo_rectify* h, int cam, uint8_t* valid, int32_t* n_valid) {
  static const char* who = "vdo_rectify_get_valid";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (cam < 0 || cam >= h->n_cams) return set_error(VDO_ERR_INVALID, "%s: cam %d outside 0..%d", who, cam, h->n_cams - 1);
  if (valid) std::memcpy(valid, h->valid[cam].data(), h->valid[cam].size());
  if (n_valid) *n_valid = h->n_valid[cam];
  return VDO_OK;
}

extern "C" int vdo_rectify_last_timing(vdo_rectify* h, double ms[2]) {
  return last_timing("vdo_rectify_last_timing", h ? &h->tm : nullptr, ms);
}

extern "C" int vdo_rectify_device_images(vdo_rectify* h, int k, uint8_t** src, uint8_t** dst) {
  if (!h) return set_error(VDO_ERR_INVALID, "vdo_rectify_device_images: handle is null");
  if (k < 0 || k >= kRectMaxJobs) return set_error(VDO_ERR_INVALID, "vdo_rectify_device_images: k %d outside 0..3", k);
  if (src) *src = h->d_src[k];
  if (dst) *dst = h->d_dst[k];
  return VDO_OK;
}

extern "C" int vdo_rectify_download_image(vdo_rectify* h, const uint8_t* image_dev, int64_t stride, uint8_t* out) {
  static const char* who = "vdo_rectify_download_image";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!image_dev || !out) return set_error(VDO_ERR_INVALID, "%s: %s is null", who, !image_dev ? "image_dev" : "out");
  if (stride < h->W) return set_error(VDO_ERR_INVALID, "%s: stride %lld smaller than the width %d", who, (long long)stride, h->W);
  const int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipMemcpy2DAsync(out, h->W, image_dev, (size_t)stride, h->W, h->H, hipMemcpyDeviceToHost, h->ctx->stream);
  return check_hip(who, hipStreamSynchronize(h->ctx->stream));
}
