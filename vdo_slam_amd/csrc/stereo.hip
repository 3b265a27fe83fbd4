// Stereo matcher: 9 x 7 census, Hamming cost volume, semi-global aggregation over 4 / 8 paths and a fused selection, from a rectified 8-bit
// pair to disparity x 256 - the `depth_raw` format K1 (vdo_frame_images_ingest_device) and FramePipeline::Step take.  The reference consumes such
// maps (src/Tracking.cc:180-204) but its authors computed them offline; the semantics are this library's own, stated in include/vdo_slam_hip.h
// (vdo_stereo_compute) and restated in NumPy by tests/stereo_ref.py.  Integer arithmetic end to end: the only fp32 operations are the conversion
// of the result and the optional output scale.
//
//   k_stereo_census     32 x 8 pixels per workgroup from an LDS tile with a 4 / 3 pixel halo (40 x 14 bytes, borders clamped); one uint64 per pixel,
//                       both images in one launch (the tile itself is census.hpp's, shared with optflow.hip).
//   k_stereo_cost       one thread per pixel and 16 disparities: 16 XOR + popcounts, one 16-byte store into cost[y][x][d] (uint8, d fastest).
//   k_stereo_aggregate  one wave per scan line, ALL directions in one launch (blockIdx.y): the disparities sit on the lanes, K = 2 (D <= 128) or 4
//                       consecutive ones per lane; d - 1 / d + 1 come from the neighbouring lanes by shuffles, min_k L_r by a wave reduction - no LDS
//                       memory and no barrier in the step; the cost bytes are loaded one pixel ahead.  L_r is added into ONE uint16 volume sum[y][x][d] with 32-bit integer atomics on pairs of
//                       entries (S <= 8 * (62 + P2) < 2^16: no carry crosses a pair), so the directions run concurrently and the sum does not
//                       depend on their order.  Per-direction volumes would take 8 x 2 bytes per entry instead of 2.
//   k_stereo_select     one thread per pixel: argmin with the lowest d on ties (packed (S << 8) | d key), second minimum outside d* +- 1, the right
//                       image's disparity at x - d* read along the volume's diagonal, left-right check, sub-pixel parabola, output, and the count
//                       of valid pixels (wave ballot, one integer atomic per wave).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "../../include/vdo_slam_hip.h"
#include "census.hpp"
#include "ctx.hpp"
#include "stage.hpp"

struct vdo_stereo {
  vdo_ctx* ctx = nullptr;
  int W = 0, H = 0;
  vdo_stereo_params p{};
  float scale = 1.f;
  uint8_t *d_left = nullptr, *d_right = nullptr;        // packed W x H; host inputs are staged here
  uint64_t* d_census = nullptr;                         // [2][H][W]
  uint8_t* d_cost = nullptr;                            // [H][W][D]
  uint16_t* d_sum = nullptr;                            // [H][W][D]
  float* d_disp = nullptr;                              // [H][W]
  int* d_count = nullptr;
  int* h_count = nullptr;                               // pinned
  float* d_flow = nullptr; int32_t* d_mask = nullptr;   // vdo_stereo_stage_frame, made on first use
  vdo::StageTimer tm;
  bool computed = false;
};

namespace vdo {

constexpr int kNoCost = 62;                             // C(x, y, d) where x - d < 0
constexpr int kAggInf = 1 << 20;                        // "takes no part" in the recurrence: above every L_r + P2
constexpr int64_t kStereoMaxVolume = int64_t(1) << 28;

__global__ __launch_bounds__(256) void k_stereo_census(const uint8_t* __restrict__ left, int64_t left_stride, const uint8_t* __restrict__ right, int64_t right_stride,
                                                       int W, int H, int tiles_x, int tiles_per_image, uint64_t* __restrict__ out) {
  const int which = blockIdx.x / tiles_per_image, t = blockIdx.x % tiles_per_image;
  census_tile(which ? right : left, which ? right_stride : left_stride, W, H, (t % tiles_x) * kCensusTX, (t / tiles_x) * kCensusTY, out + (size_t)which * W * H);
}

__global__ __launch_bounds__(256) void k_stereo_cost(const uint64_t* __restrict__ cl, const uint64_t* __restrict__ cr, int W, int64_t n_pix, int D,
                                                     uint8_t* __restrict__ cost) {
  const int G = D / 16;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pix * G) return;
  const int64_t pix = i / G;
  const int g = (int)(i % G), x = (int)(pix % W);
  const uint64_t c = cl[pix];
  uint32_t w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int d = g * 16 + q * 4 + b;
      const uint32_t e = x - d >= 0 ? (uint32_t)__popcll(c ^ cr[pix - d]) : (uint32_t)kNoCost;
      v |= e << (8 * b);
    }
    w[q] = v;
  }
  *(uint4*)(cost + pix * D + g * 16) = make_uint4(w[0], w[1], w[2], w[3]);      // 16-byte aligned: D is a multiple of 16
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

__constant__ int kStereoDx[8] = {1, -1, 0, 0, 1, -1, 1, -1};
__constant__ int kStereoDy[8] = {0, 0, 1, -1, 1, 1, -1, -1};

// K consecutive disparities per lane (d = K * lane + j); 4 waves = 4 lines per workgroup, blockIdx.y = direction
template <int K>
__global__ __launch_bounds__(256) void k_stereo_aggregate(const uint8_t* __restrict__ cost, uint32_t* __restrict__ sum2, int W, int H, int D, int P1, int P2) {
  const int lane = threadIdx.x & 63;
  const int dx = kStereoDx[blockIdx.y], dy = kStereoDy[blockIdx.y];
  const int n_lines = dy == 0 ? H : dx == 0 ? W : W + H - 1;
  const int64_t line64 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (line64 >= n_lines) return;                                   // (wave-uniform)
  const int line = (int)line64;
  // the line's first pixel: the one whose predecessor p - r is outside
  int x, y;
  if (dy == 0) { x = dx > 0 ? 0 : W - 1; y = line; }
  else if (dx == 0 || line < W) { x = line; y = dy > 0 ? 0 : H - 1; }
  else { const int j = line - W + 1; x = dx > 0 ? 0 : W - 1; y = dy > 0 ? j : H - 1 - j; }
  const bool act = K * lane < D;                                   // (D is a multiple of 16: a lane is entirely in or out)
  const bool last = K * (lane + 1) >= D;
  using Packed = typename std::conditional<K == 2, uint16_t, uint32_t>::type;
  auto load = [&](int px, int py) -> Packed {                      // the K cost bytes of this lane, packed as they lie
    return act ? *(const Packed*)(cost + ((size_t)py * W + px) * D + K * lane) : (Packed)0;
  };
  auto inside = [&](int px, int py) { return px >= 0 && px < W && py >= 0 && py < H; };
  int L[K];
  {
    const Packed v = load(x, y);
#pragma unroll
    for (int j = 0; j < K; ++j) L[j] = act ? (int)((v >> (8 * j)) & 255) : kAggInf;
  }
  // the cost of a pixel is loaded one step before the step that uses it: the load's latency runs beside the exchanges of the step in between
  int nx = x + dx, ny = y + dy;
  bool more = inside(nx, ny);
  Packed vn = more ? load(nx, ny) : (Packed)0;
  for (;;) {
    if (act) {
      uint32_t* o = sum2 + (((size_t)y * W + x) * D + K * lane) / 2;
#pragma unroll
      for (int j = 0; j < K; j += 2) atomicAdd(o + j / 2, (uint32_t)L[j] | ((uint32_t)L[j + 1] << 16));
    }
    if (!more) break;
    x = nx; y = ny;
    const Packed v = vn;
    nx += dx; ny += dy;
    more = inside(nx, ny);
    if (more) vn = load(nx, ny);
    int m = L[0];
#pragma unroll
    for (int j = 1; j < K; ++j) m = min(m, L[j]);
    m = wave_min(m);
    int up = __shfl_up(L[K - 1], 1, 64), dn = __shfl_down(L[0], 1, 64);
    if (lane == 0) up = kAggInf;                                   // d - 1 < 0 and d + 1 >= D take no part
    if (last) dn = kAggInf;
    int N[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int lo = j ? L[j - 1] : up, hi = j < K - 1 ? L[j + 1] : dn;
      N[j] = (int)((v >> (8 * j)) & 255) + min(min(L[j], m + P2), min(lo, hi) + P1) - m;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) L[j] = act ? N[j] : kAggInf;
  }
}

__global__ __launch_bounds__(256) void k_stereo_select(const uint16_t* __restrict__ S, int W, int64_t n_pix, int D, int uniqueness, int lr_max_diff, int subpixel,
                                                       float scale, float* __restrict__ out, int* __restrict__ n_valid) {
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool ok = false;
  if (pix < n_pix) {
    const int x = (int)(pix % W);
    const uint16_t* s = S + pix * D;
    uint32_t best = ~0u;
    for (int d0 = 0; d0 < D; d0 += 8) {
      const uint4 v = *(const uint4*)(s + d0);                     // 16-byte aligned: D is a multiple of 16
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        best = min(best, ((w[q] & 0xffffu) << 8) | (uint32_t)(d0 + 2 * q));       // (S << 8) | d: the lowest d wins a tie
        best = min(best, ((w[q] >> 16) << 8) | (uint32_t)(d0 + 2 * q + 1));
      }
    }
    const int ds = (int)(best & 255u), s0 = (int)(best >> 8);
    ok = ds >= 1 && x - ds >= 0;
    if (ok && uniqueness > 0) {
      int s2 = INT_MAX;
      for (int d0 = 0; d0 < D; d0 += 8) {
        const uint4 v = *(const uint4*)(s + d0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int d = d0 + 2 * q;
          if (d < ds - 1 || d > ds + 1) s2 = min(s2, (int)(w[q] & 0xffffu));
          if (d + 1 < ds - 1 || d + 1 > ds + 1) s2 = min(s2, (int)(w[q] >> 16));
        }
      }
      if (s2 != INT_MAX) ok = 100 * s0 < (100 - uniqueness) * s2;
    }
    if (ok && lr_max_diff >= 0) {                                  // dR(x - d*, y): the minimum along the diagonal S(x' + d, y, d), x' + d < W
      const int xr = x - ds;
      const uint16_t* row = S + (pix - x) * D;
      const int nd = min(D, W - xr);
      uint32_t rbest = ~0u;
      for (int d = 0; d < nd; ++d) rbest = min(rbest, ((uint32_t)row[(size_t)(xr + d) * D + d] << 8) | (uint32_t)d);
      const int dr = (int)(rbest & 255u);
      ok = abs(dr - ds) <= lr_max_diff;
    }
    int off = 0;
    if (ok && subpixel && ds <= D - 2) {
      const int sm = s[ds - 1], sp = s[ds + 1];
      const int den = sm + sp - 2 * s0;
      if (den > 0) {
        const int num = 128 * (sm - sp);
        const int mag = (2 * abs(num) + den) / (2 * den);
        off = num < 0 ? -mag : mag;
      }
    }
    out[pix] = ok ? (float)(256 * ds + off) * scale : 0.f;
  }
  const unsigned long long m = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_valid, (int)__popcll(m));
}

static void stereo_free(vdo_stereo* h) {
  hipFree(h->d_left); hipFree(h->d_right); hipFree(h->d_census); hipFree(h->d_cost); hipFree(h->d_sum); hipFree(h->d_disp); hipFree(h->d_count);
  hipFree(h->d_flow); hipFree(h->d_mask);
  if (h->h_count) hipHostFree(h->h_count);
  h->tm.destroy();
  delete h;
}

}  // namespace vdo

using namespace vdo;

extern "C" int vdo_stereo_create(vdo_ctx* ctx, int width, int height, const vdo_stereo_params* p, vdo_stereo** out) {
  static const char* who = "vdo_stereo_create";
  if (!ctx) return set_error(VDO_ERR_INVALID, "%s: ctx is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (!p) return set_error(VDO_ERR_INVALID, "%s: params is null", who);
  if (width < 1) return set_error(VDO_ERR_INVALID, "%s: width %d < 1", who, width);
  if (height < 1) return set_error(VDO_ERR_INVALID, "%s: height %d < 1", who, height);
  if (p->max_disparity < 16 || p->max_disparity > 256 || p->max_disparity % 16) return set_error(VDO_ERR_INVALID, "%s: max_disparity %d is not a multiple of 16 in 16..256", who, p->max_disparity);
  if (p->paths != 4 && p->paths != 8) return set_error(VDO_ERR_INVALID, "%s: paths %d is neither 4 nor 8", who, p->paths);
  if (p->p1 < 1 || p->p1 > p->p2) return set_error(VDO_ERR_INVALID, "%s: p1 %d outside 1..p2 (%d)", who, p->p1, p->p2);
  if (p->p2 > 1000) return set_error(VDO_ERR_INVALID, "%s: p2 %d above 1000", who, p->p2);
  if (p->uniqueness < 0 || p->uniqueness > 99) return set_error(VDO_ERR_INVALID, "%s: uniqueness %d outside 0..99", who, p->uniqueness);
  if (p->lr_max_diff < -1) return set_error(VDO_ERR_INVALID, "%s: lr_max_diff %d below -1", who, p->lr_max_diff);
  const int64_t n_pix = (int64_t)width * height;
  if (n_pix * p->max_disparity > kStereoMaxVolume)
    return set_error(VDO_ERR_UNSUPPORTED, "%s: width x height x max_disparity = %d x %d x %d exceeds 2^28 volume entries", who, width, height, p->max_disparity);
  int rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  vdo_stereo* h = new vdo_stereo;
  h->ctx = ctx; h->W = width; h->H = height; h->p = *p;
  const size_t n = (size_t)n_pix, vol = n * p->max_disparity;
  const bool ok = hipMalloc((void**)&h->d_left, n) == hipSuccess && hipMalloc((void**)&h->d_right, n) == hipSuccess &&
                  hipMalloc((void**)&h->d_census, 2 * n * sizeof(uint64_t)) == hipSuccess && hipMalloc((void**)&h->d_cost, vol) == hipSuccess &&
                  hipMalloc((void**)&h->d_sum, vol * sizeof(uint16_t)) == hipSuccess && hipMalloc((void**)&h->d_disp, n * sizeof(float)) == hipSuccess &&
                  hipMalloc((void**)&h->d_count, sizeof(int)) == hipSuccess && hipHostMalloc((void**)&h->h_count, sizeof(int), hipHostMallocDefault) == hipSuccess &&
                  h->tm.create();
  if (!ok) {
    (void)hipGetLastError();
    stereo_free(h);
    return set_error(VDO_ERR_OOM, "%s: device allocation failed for %d x %d x %d", who, width, height, p->max_disparity);
  }
  *out = h;
  return VDO_OK;
}

extern "C" int vdo_stereo_destroy(vdo_stereo* h) {
  if (!h) return VDO_OK;
  if (ctx_bind(h->ctx) == VDO_OK) hipStreamSynchronize(h->ctx->stream);
  stereo_free(h);
  return VDO_OK;
}

extern "C" int vdo_stereo_set_output_scale(vdo_stereo* h, float scale) {
  static const char* who = "vdo_stereo_set_output_scale";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!(scale > 0.f) || scale > 65536.f) return set_error(VDO_ERR_INVALID, "%s: scale %g outside (0, 65536]", who, (double)scale);
  h->scale = scale;
  return VDO_OK;
}

extern "C" int vdo_stereo_compute(vdo_stereo* h, const uint8_t* left, int64_t left_stride, const uint8_t* right, int64_t right_stride, int src_is_device,
                                  float* disparity256, int out_is_device, int32_t* n_valid) {
  static const char* who = "vdo_stereo_compute";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!left) return set_error(VDO_ERR_INVALID, "%s: left is null", who);
  if (!right) return set_error(VDO_ERR_INVALID, "%s: right is null", who);
  if (left_stride < h->W) return set_error(VDO_ERR_INVALID, "%s: left_stride %lld smaller than the width %d", who, (long long)left_stride, h->W);
  if (right_stride < h->W) return set_error(VDO_ERR_INVALID, "%s: right_stride %lld smaller than the width %d", who, (long long)right_stride, h->W);
  if (!disparity256) return set_error(VDO_ERR_INVALID, "%s: disparity256 is null", who);
  if (!n_valid) return set_error(VDO_ERR_INVALID, "%s: n_valid is null", who);
  int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const int W = h->W, H = h->H, D = h->p.max_disparity;
  const int64_t n_pix = (int64_t)W * H;
  const auto t0 = h->tm.begin(s);
  if (!src_is_device) {                                            // staged packed; a device pair is read where it is, with its strides
    left = stage_rows(s, h->d_left, left, left_stride, W, H, 0);
    right = stage_rows(s, h->d_right, right, right_stride, W, H, 0);
    left_stride = right_stride = W;
  }
  const int tiles_x = (W + kCensusTX - 1) / kCensusTX, tiles = tiles_x * ((H + kCensusTY - 1) / kCensusTY);
  hipLaunchKernelGGL(k_stereo_census, dim3(2 * tiles), dim3(256), 0, s, left, left_stride, right, right_stride, W, H, tiles_x, tiles, h->d_census);
  hipLaunchKernelGGL(k_stereo_cost, dim3((unsigned)((n_pix * (D / 16) + 255) / 256)), dim3(256), 0, s, (const uint64_t*)h->d_census,
                     (const uint64_t*)h->d_census + n_pix, W, n_pix, D, h->d_cost);
  hipMemsetAsync(h->d_sum, 0, (size_t)n_pix * D * sizeof(uint16_t), s);
  hipMemsetAsync(h->d_count, 0, sizeof(int), s);
  const int max_lines = h->p.paths == 8 ? W + H - 1 : (W > H ? W : H);
  const dim3 ga((max_lines + 3) / 4, h->p.paths);
  if (D <= 128) hipLaunchKernelGGL(k_stereo_aggregate<2>, ga, dim3(256), 0, s, (const uint8_t*)h->d_cost, (uint32_t*)h->d_sum, W, H, D, h->p.p1, h->p.p2);
  else hipLaunchKernelGGL(k_stereo_aggregate<4>, ga, dim3(256), 0, s, (const uint8_t*)h->d_cost, (uint32_t*)h->d_sum, W, H, D, h->p.p1, h->p.p2);
  float* d_out = out_is_device ? disparity256 : h->d_disp;
  hipLaunchKernelGGL(k_stereo_select, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, s, (const uint16_t*)h->d_sum, W, n_pix, D, h->p.uniqueness, h->p.lr_max_diff,
                     h->p.subpixel, h->scale, d_out, h->d_count);
  h->tm.mark_end(s);
  hipMemcpyAsync(h->h_count, h->d_count, sizeof(int), hipMemcpyDeviceToHost, s);
  if (!out_is_device) hipMemcpyAsync(disparity256, h->d_disp, (size_t)n_pix * sizeof(float), hipMemcpyDeviceToHost, s);
  rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  *n_valid = *h->h_count;
  h->tm.finish(t0);
  h->computed = true;
  return VDO_OK;
}

static int stereo_fetch(const char* who, vdo_stereo* h, const void* dev, void* out, size_t bytes) {
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (!h->computed) return set_error(VDO_ERR_INVALID, "%s: no vdo_stereo_compute on this handle yet", who);
  const int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, h->ctx->stream);
  return check_hip(who, hipStreamSynchronize(h->ctx->stream));
}

extern "C" int vdo_stereo_get_census(vdo_stereo* h, int which, uint64_t* out) {
  if (h && which != 0 && which != 1) return set_error(VDO_ERR_INVALID, "vdo_stereo_get_census: which %d is neither 0 (left) nor 1 (right)", which);
  const size_t n = h ? (size_t)h->W * h->H : 0;
  return stereo_fetch("vdo_stereo_get_census", h, h ? h->d_census + (size_t)which * n : nullptr, out, n * sizeof(uint64_t));
}

extern "C" int vdo_stereo_get_cost(vdo_stereo* h, uint8_t* out) {
  return stereo_fetch("vdo_stereo_get_cost", h, h ? h->d_cost : nullptr, out, h ? (size_t)h->W * h->H * h->p.max_disparity : 0);
}

extern "C" int vdo_stereo_get_aggregated(vdo_stereo* h, uint16_t* out) {
  return stereo_fetch("vdo_stereo_get_aggregated", h, h ? h->d_sum : nullptr, out, h ? (size_t)h->W * h->H * h->p.max_disparity * sizeof(uint16_t) : 0);
}

extern "C" int vdo_stereo_last_timing(vdo_stereo* h, double ms[2]) {
  return last_timing("vdo_stereo_last_timing", h ? &h->tm : nullptr, ms);
}

extern "C" int vdo_stereo_device_images(vdo_stereo* h, uint8_t** left, uint8_t** right, float** disparity256) {
  if (!h) return set_error(VDO_ERR_INVALID, "vdo_stereo_device_images: handle is null");
  if (left) *left = h->d_left;
  if (right) *right = h->d_right;
  if (disparity256) *disparity256 = h->d_disp;
  return VDO_OK;
}

extern "C" int vdo_stereo_stage_frame(vdo_stereo* h, const float* flow, const int32_t* mask, float** flow_dev, int32_t** mask_dev) {
  static const char* who = "vdo_stereo_stage_frame";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!flow || !mask || !flow_dev || !mask_dev)
    return set_error(VDO_ERR_INVALID, "%s: %s is null", who, !flow ? "flow" : !mask ? "mask" : !flow_dev ? "flow_dev" : "mask_dev");
  const int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  const size_t n = (size_t)h->W * h->H;
  if (!h->d_flow && hipMalloc((void**)&h->d_flow, 2 * n * sizeof(float)) != hipSuccess) { h->d_flow = nullptr; return set_error(VDO_ERR_OOM, "%s: device allocation failed", who); }
  if (!h->d_mask && hipMalloc((void**)&h->d_mask, n * sizeof(int32_t)) != hipSuccess) { h->d_mask = nullptr; return set_error(VDO_ERR_OOM, "%s: device allocation failed", who); }
  hipStream_t s = h->ctx->stream;
  hipMemcpyAsync(h->d_flow, flow, 2 * n * sizeof(float), hipMemcpyHostToDevice, s);
  hipMemcpyAsync(h->d_mask, mask, n * sizeof(int32_t), hipMemcpyHostToDevice, s);
  const int rs = check_hip(who, hipStreamSynchronize(s));
  if (rs != VDO_OK) return rs;
  *flow_dev = h->d_flow; *mask_dev = h->d_mask;
  return VDO_OK;
}
