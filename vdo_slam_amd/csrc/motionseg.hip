// Motion segmenter: which pixels move against the scene, from the disparity of frame t, the disparity of frame t + 1, the flow between them and the
// camera motion - the class image the instance labeller takes, made on the device.  The reference takes its masks from an offline segmentation
// network; the semantics are this library's own, stated in include/vdo_slam_hip.h (vdo_motionseg_compute) and restated in NumPy by
// tests/motionseg_ref.py.  Stage 1 is fp32 with one rounded operation per step (the library is built with -ffp-contract=off; / and floorf are
// correctly rounded), stage 2 is integer: no result depends on workgroup shape or order.
//
//   k_ms_residual   one thread per pixel: coalesced disp0 and float2 flow loads, one gathered disp1, the state byte and the residual; the numbers of
//                   state-0 and state-2 pixels by wave ballot, one integer atomic per wave.  T and the parameters are kernel arguments.
//   k_ms_vote       one workgroup per 64 x 16 tile: the states with an r-pixel halo in LDS, the packed (m, s) pair summed along x, then along y, the
//                   class byte; the number of moving pixels by ballot.
//   k_ms_samples    the grid positions of the ego-motion, kept under stage 1's tests on the source pixel: count per workgroup, k_ms_scan (one workgroup),
//                   then the same kernel writes X and uv in raster order (the ordered compaction of frame.hip's K10 and labels.hip).
//
// NO OUT-OF-RANGE READS: the one gathered address comes from float compares against 0 and W - 1 / H - 1 made before any conversion to int; a NaN
// fails them.  Every loop has a bound fixed by the launch (the tile, the radius <= 7, the grid).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>
#include <cstring>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"
#include "scan.hpp"
#include "stage.hpp"

namespace vdo {

constexpr int kMsTW = 64, kMsTH = 16, kMsRMax = 7;                         // vote tile: 256 threads, 4 pixels each
constexpr int kMsPitch = 80, kMsHH = kMsTH + 2 * kMsRMax;                  // LDS: 30 x 80 state bytes + 30 x 64 packed sums = 10080 bytes
enum { kMsMoving = 0, kMsStatic, kMsUnknown, kMsCounters = 4 };

// what the kernels take by value: the camera, the weights, the thresholds and the first three rows of T
struct MsArgs {
  float fx, fy, cx, cy, bf, unit, wf, wd, chi2, min_d;
  float T[12];
};

}  // namespace vdo

struct vdo_motionseg {
  vdo_ctx* ctx = nullptr;
  int W = 0, H = 0;
  vdo_motionseg_params p{};
  vdo::MsArgs a{};
  uint8_t* d_state = nullptr;                             // [H][W] 0 static, 1 moving, 2 unknown
  float* d_res = nullptr;                                 // [H][W] e, or -1 where unknown
  uint8_t* d_cls = nullptr;                               // [H][W]
  float* d_disp1 = nullptr;                               // [H][W]: the next pair's disparity (a matcher writes it; a host or padded disp1 is staged here)
  uint8_t* d_right = nullptr;                             // [H][W]: room for the next-right picture of a rectified frame
  float* d_disp0 = nullptr;                               // [H][W] staging
  float* d_flow = nullptr;                                // [H][W][2] staging
  uint8_t* d_valid = nullptr;                             // [H][W] staging
  char* d_smp = nullptr;                                  // 8 bytes (n), then X [cap][3] and uv [cap][2] doubles, cap = the call's grid size <= W * H
  char* h_smp = nullptr;                                  // pinned mirror
  int32_t* d_blk = nullptr;                               // per 256 grid positions: kept, then their exclusive scan
  int32_t* d_cnt = nullptr;                               // [kMsCounters]
  int32_t* h_cnt = nullptr;                               // pinned
  vdo::StageTimer tm;
  bool computed = false;
  int smp_cap = -1;                                       // the grid size of the last ego-motion, -1 before the first
};

namespace vdo {

__device__ __forceinline__ bool ms_finite(float v) { return fabsf(v) <= FLT_MAX; }       // false for NaN and the infinities

// Stage 1's tests on the source pixel (x, y): d0, the flow, its validity flag and the target inside the image.  True: *d0, *uo, *vo and the
// target's raster index *j are set.
__device__ __forceinline__ bool ms_source(const MsArgs& a, int x, int y, int W, int H, float disp0, float2 f, bool flagged, float* d0, float* uo, float* vo, int* j) {
  *d0 = disp0 / a.unit;
  *uo = (float)x + f.x;
  *vo = (float)y + f.y;
  const float xq = floorf(*uo + 0.5f), yq = floorf(*vo + 0.5f);
  const bool ok = ms_finite(*d0) && *d0 >= a.min_d && ms_finite(*uo) && ms_finite(*vo) && xq >= 0.f && xq <= (float)(W - 1) && yq >= 0.f && yq <= (float)(H - 1) && flagged;
  *j = ok ? (int)yq * W + (int)xq : 0;
  return ok;
}

__device__ __forceinline__ void ms_backproject(const MsArgs& a, int x, int y, float d0, float* X, float* Y, float* Z) {
  *Z = a.bf / d0;
  *X = ((float)x - a.cx) * *Z / a.fx;
  *Y = ((float)y - a.cy) * *Z / a.fy;
}

__global__ __launch_bounds__(256) void k_ms_residual(MsArgs a, const float* __restrict__ disp0, const float* __restrict__ disp1, const float2* __restrict__ flow,
                                                     const uint8_t* __restrict__ valid, int W, int H, uint8_t* __restrict__ state, float* __restrict__ res,
                                                     int32_t* __restrict__ cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool in = i < W * H;
  int st = 2;
  float e = -1.f;
  if (in) {
    const int y = i / W, x = i - y * W;
    float d0, uo, vo;
    int j;
    if (ms_source(a, x, y, W, H, disp0[i], flow[i], !valid || valid[i] != 0, &d0, &uo, &vo, &j)) {
      const float d1 = disp1[j] / a.unit;
      if (ms_finite(d1) && d1 > 0.f) {
        float X, Y, Z;
        ms_backproject(a, x, y, d0, &X, &Y, &Z);
        const float Xp = (a.T[0] * X + a.T[1] * Y) + (a.T[2] * Z + a.T[3]);
        const float Yp = (a.T[4] * X + a.T[5] * Y) + (a.T[6] * Z + a.T[7]);
        const float Zp = (a.T[8] * X + a.T[9] * Y) + (a.T[10] * Z + a.T[11]);
        const float up = a.fx * Xp / Zp + a.cx, vp = a.fy * Yp / Zp + a.cy, dp = a.bf / Zp;
        const float du = uo - up, dv = vo - vp, dd = d1 - dp;
        const float ee = (du * du + dv * dv) * a.wf + (dd * dd) * a.wd;
        if (Zp > 0.f && ms_finite(ee)) { e = ee; st = ee > a.chi2 ? 1 : 0; }
      }
    }
    state[i] = (uint8_t)st;
    res[i] = e;
  }
  const int n0 = (int)__popcll(__ballot(in && st == 0)), n2 = (int)__popcll(__ballot(in && st == 2));
  if ((threadIdx.x & 63) == 0) {
    if (n0) atomicAdd(cnt + kMsStatic, n0);
    if (n2) atomicAdd(cnt + kMsUnknown, n2);
  }
}

__global__ __launch_bounds__(256) void k_ms_vote(const uint8_t* __restrict__ state, int W, int H, int tiles_x, int r, int vote_num, int vote_den, int min_known, int class_value,
                                                 uint8_t* __restrict__ cls, int32_t* __restrict__ cnt) {
  __shared__ uint8_t st[kMsHH * kMsPitch];
  __shared__ uint32_t hs[kMsHH * kMsTW];
  const int x0 = (blockIdx.x % tiles_x) * kMsTW, y0 = (blockIdx.x / tiles_x) * kMsTH;
  const int hw = kMsTW + 2 * r, hh = kMsTH + 2 * r;                          // r <= kMsRMax: hw <= 78 <= kMsPitch, hh <= kMsHH
  for (int k = threadIdx.x; k < hw * hh; k += 256) {
    const int ly = k / hw, lx = k - ly * hw, gx = x0 - r + lx, gy = y0 - r + ly;
    st[ly * kMsPitch + lx] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? state[gy * W + gx] : (uint8_t)2;       // outside the image: in neither count
  }
  __syncthreads();
  for (int k = threadIdx.x; k < hh * kMsTW; k += 256) {
    const int ly = k / kMsTW, lx = k % kMsTW;
    uint32_t acc = 0;
    for (int i = 0; i <= 2 * r; ++i) { const int s = st[ly * kMsPitch + lx + i]; acc += (s == 1 ? 1u : 0u) + (s == 0 ? 0x10000u : 0u); }
    hs[k] = acc;                                                             // m in the low half, s in the high half, each <= 15
  }
  __syncthreads();
  const int lx = threadIdx.x & 63;
  int moved = 0;
#pragma unroll
  for (int q = 0; q < kMsTH / 4; ++q) {
    const int ly = (threadIdx.x >> 6) + 4 * q;
    uint32_t acc = 0;
    for (int j = 0; j <= 2 * r; ++j) acc += hs[(ly + j) * kMsTW + lx];       // each half <= 225
    const int m = (int)(acc & 0xffffu), known = m + (int)(acc >> 16);
    const int x = x0 + lx, y = y0 + ly;
    const bool in = x < W && y < H;
    const bool mv = in && known >= min_known && m * vote_den > vote_num * known;
    if (in) cls[y * W + x] = mv ? (uint8_t)class_value : (uint8_t)0;
    moved += (int)__popcll(__ballot(mv));
  }
  if (lx == 0 && moved) atomicAdd(cnt + kMsMoving, moved);
}

// grid position g -> pixel; the kept ones are numbered in raster order
template <bool WRITE>
__global__ __launch_bounds__(256) void k_ms_samples(MsArgs a, const float* __restrict__ disp0, const float2* __restrict__ flow, const uint8_t* __restrict__ valid, int W, int H,
                                                    int step, int nx, int ngrid, int32_t* __restrict__ blk, double* __restrict__ X3, double* __restrict__ uv2) {
  __shared__ int lds[17];
  const int g = blockIdx.x * 256 + threadIdx.x;
  int keep = 0;
  float d0 = 0.f, uo = 0.f, vo = 0.f;
  int x = 0, y = 0;
  if (g < ngrid) {
    const int gy = g / nx, gx = g - gy * nx;
    x = step / 2 + gx * step; y = step / 2 + gy * step;                      // < W, < H by the choice of nx and ngrid
    const int i = y * W + x;
    int j;
    keep = ms_source(a, x, y, W, H, disp0[i], flow[i], !valid || valid[i] != 0, &d0, &uo, &vo, &j) ? 1 : 0;
  }
  int total;
  const int ex = block_excl_scan(keep, lds, &total);
  if (!WRITE) {
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
  } else if (keep) {
    const int pos = blk[blockIdx.x] + ex;
    float X, Y, Z;
    ms_backproject(a, x, y, d0, &X, &Y, &Z);
    X3[3 * pos] = (double)X; X3[3 * pos + 1] = (double)Y; X3[3 * pos + 2] = (double)Z;
    uv2[2 * pos] = (double)uo; uv2[2 * pos + 1] = (double)vo;
  }
}

// exclusive scan of the workgroup counts (single workgroup), as labels.hip's k_lab_scan; the total goes to the head of the sample block
__global__ __launch_bounds__(1024) void k_ms_scan(int32_t* __restrict__ blk, int nblk, int32_t* __restrict__ n_out) {
  __shared__ int lds[17];
  int carry = 0;
  for (int base = 0; base < nblk; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < nblk ? blk[i] : 0;
    int total;
    const int ex = block_excl_scan(v, lds, &total);
    if (i < nblk) blk[i] = carry + ex;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) { n_out[0] = carry; n_out[1] = 0; }
}

static void ms_free(vdo_motionseg* h) {
  hipFree(h->d_state); hipFree(h->d_res); hipFree(h->d_cls); hipFree(h->d_disp1); hipFree(h->d_right); hipFree(h->d_disp0); hipFree(h->d_flow); hipFree(h->d_valid);
  hipFree(h->d_smp); hipFree(h->d_blk); hipFree(h->d_cnt);
  if (h->h_smp) hipHostFree(h->h_smp);
  if (h->h_cnt) hipHostFree(h->h_cnt);
  h->tm.destroy();
  delete h;
}

// the images every entry reads, brought to where a kernel can read them: a packed (and, for the flow, 8-byte aligned) device image is read where
// it lies, anything else goes to the handle's staging image
struct MsSources { const float* disp0; const float2* flow; const uint8_t* valid; };
static MsSources ms_stage(vdo_motionseg* h, hipStream_t s, const float* disp0, int64_t disp0_stride, const float* flow, int64_t flow_stride, const uint8_t* valid, int64_t valid_stride,
                          int src_is_device) {
  const int W = h->W, H = h->H;
  return MsSources{stage_rows(s, h->d_disp0, disp0, disp0_stride, W, H, src_is_device), (const float2*)stage_rows(s, h->d_flow, flow, flow_stride, 2 * W, H, src_is_device, 8),
                   valid ? stage_rows(s, h->d_valid, valid, valid_stride, W, H, src_is_device) : nullptr};
}

// the refusals the two entries share; 0 when the sources are in order
static int ms_check_sources(const char* who, const vdo_motionseg* h, const float* disp0, int64_t disp0_stride, const float* flow, int64_t flow_stride, const uint8_t* valid,
                            int64_t valid_stride) {
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!disp0) return set_error(VDO_ERR_INVALID, "%s: disp0 is null", who);
  if (disp0_stride < h->W) return set_error(VDO_ERR_INVALID, "%s: disp0_stride_floats %lld smaller than the width %d", who, (long long)disp0_stride, h->W);
  if (!flow) return set_error(VDO_ERR_INVALID, "%s: flow is null", who);
  if (flow_stride < 2 * (int64_t)h->W) return set_error(VDO_ERR_INVALID, "%s: flow_stride_floats %lld smaller than twice the width %d", who, (long long)flow_stride, h->W);
  if (valid && valid_stride < h->W) return set_error(VDO_ERR_INVALID, "%s: flow_valid_stride %lld smaller than the width %d", who, (long long)valid_stride, h->W);
  return VDO_OK;
}

}  // namespace vdo

using namespace vdo;

extern "C" int vdo_motionseg_create(vdo_ctx* ctx, int width, int height, const vdo_motionseg_params* p, vdo_motionseg** out) {
  static const char* who = "vdo_motionseg_create";
  if (!ctx) return set_error(VDO_ERR_INVALID, "%s: ctx is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (!p) return set_error(VDO_ERR_INVALID, "%s: params is null", who);
  if (width < 1) return set_error(VDO_ERR_INVALID, "%s: width %d < 1", who, width);
  if (height < 1) return set_error(VDO_ERR_INVALID, "%s: height %d < 1", who, height);
  int rc = check_intrinsics(who, "K", p->K);
  if (rc != VDO_OK) return rc;
  if (!is_finite(p->bf) || !(p->bf > 0.f)) return set_error(VDO_ERR_INVALID, "%s: bf %g must be positive and finite", who, (double)p->bf);
  if (!is_finite(p->disp_unit) || !(p->disp_unit > 0.f)) return set_error(VDO_ERR_INVALID, "%s: disp_unit %g must be positive and finite", who, (double)p->disp_unit);
  if (!is_finite(p->sigma_flow) || !(p->sigma_flow > 0.f)) return set_error(VDO_ERR_INVALID, "%s: sigma_flow %g must be positive and finite", who, (double)p->sigma_flow);
  if (!is_finite(p->sigma_disp) || !(p->sigma_disp > 0.f)) return set_error(VDO_ERR_INVALID, "%s: sigma_disp %g must be positive and finite", who, (double)p->sigma_disp);
  if (!is_finite(p->chi2) || !(p->chi2 >= 0.f)) return set_error(VDO_ERR_INVALID, "%s: chi2 %g must be finite and >= 0", who, (double)p->chi2);
  if (!is_finite(p->min_disparity) || !(p->min_disparity >= 0.f)) return set_error(VDO_ERR_INVALID, "%s: min_disparity %g must be finite and >= 0", who, (double)p->min_disparity);
  if (p->vote_radius < 0 || p->vote_radius > kMsRMax) return set_error(VDO_ERR_INVALID, "%s: vote_radius %d outside 0..%d", who, p->vote_radius, kMsRMax);
  if (p->vote_den < 1 || p->vote_den > 65535) return set_error(VDO_ERR_INVALID, "%s: vote_den %d outside 1..65535", who, p->vote_den);
  if (p->vote_num < 0 || p->vote_num >= p->vote_den) return set_error(VDO_ERR_INVALID, "%s: vote_num %d outside 0..vote_den-1 = %d", who, p->vote_num, p->vote_den - 1);
  if (p->min_known < 1) return set_error(VDO_ERR_INVALID, "%s: min_known %d < 1", who, p->min_known);
  if (p->class_value < 1 || p->class_value > 255) return set_error(VDO_ERR_INVALID, "%s: class_value %d outside 1..255", who, p->class_value);
  rc = check_image_size(who, "width x height =", width, height);
  if (rc == VDO_OK) rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  vdo_motionseg* h = new vdo_motionseg;
  h->ctx = ctx; h->W = width; h->H = height; h->p = *p;
  MsArgs& a = h->a;
  a.fx = p->K[0]; a.fy = p->K[1]; a.cx = p->K[2]; a.cy = p->K[3]; a.bf = p->bf; a.unit = p->disp_unit;
  a.wf = 1.0f / (p->sigma_flow * p->sigma_flow); a.wd = 1.0f / (p->sigma_disp * p->sigma_disp);
  a.chi2 = p->chi2; a.min_d = p->min_disparity > FLT_MIN ? p->min_disparity : FLT_MIN;
  const size_t n = (size_t)width * height, nblk = (n + 255) / 256, smp = 8 + n * 5 * sizeof(double);
  const bool ok = hipMalloc((void**)&h->d_state, n) == hipSuccess && hipMalloc((void**)&h->d_res, n * sizeof(float)) == hipSuccess && hipMalloc((void**)&h->d_cls, n) == hipSuccess &&
                  hipMalloc((void**)&h->d_disp1, n * sizeof(float)) == hipSuccess && hipMalloc((void**)&h->d_right, n) == hipSuccess &&
                  hipMalloc((void**)&h->d_disp0, n * sizeof(float)) == hipSuccess && hipMalloc((void**)&h->d_flow, 2 * n * sizeof(float)) == hipSuccess &&
                  hipMalloc((void**)&h->d_valid, n) == hipSuccess && hipMalloc((void**)&h->d_smp, smp) == hipSuccess && hipMalloc((void**)&h->d_blk, nblk * sizeof(int32_t)) == hipSuccess &&
                  hipMalloc((void**)&h->d_cnt, kMsCounters * sizeof(int32_t)) == hipSuccess && hipHostMalloc((void**)&h->h_smp, smp, hipHostMallocDefault) == hipSuccess &&
                  hipHostMalloc((void**)&h->h_cnt, kMsCounters * sizeof(int32_t), hipHostMallocDefault) == hipSuccess && h->tm.create();
  if (!ok) {
    (void)hipGetLastError();
    ms_free(h);
    return set_error(VDO_ERR_OOM, "%s: device allocation failed for %d x %d", who, width, height);
  }
  *out = h;
  return VDO_OK;
}

extern "C" int vdo_motionseg_destroy(vdo_motionseg* h) {
  if (!h) return VDO_OK;
  if (ctx_bind(h->ctx) == VDO_OK) hipStreamSynchronize(h->ctx->stream);
  ms_free(h);
  return VDO_OK;
}

extern "C" int vdo_motionseg_egomotion(vdo_motionseg* h, const float* disp0, int64_t disp0_stride_floats, const float* flow, int64_t flow_stride_floats, const uint8_t* flow_valid,
                                       int64_t flow_valid_stride, int src_is_device, int step, int max_iterations, double reproj_threshold, double confidence, int min_inliers,
                                       float T[16], int32_t out[3]) {
  static const char* who = "vdo_motionseg_egomotion";
  int rc = ms_check_sources(who, h, disp0, disp0_stride_floats, flow, flow_stride_floats, flow_valid, flow_valid_stride);
  if (rc != VDO_OK) return rc;
  if (step < 1) return set_error(VDO_ERR_INVALID, "%s: step %d < 1", who, step);
  if (max_iterations < 0) return set_error(VDO_ERR_INVALID, "%s: max_iterations %d < 0", who, max_iterations);
  if (!(reproj_threshold > 0.0) || !(reproj_threshold <= DBL_MAX)) return set_error(VDO_ERR_INVALID, "%s: reproj_threshold %g must be positive and finite", who, reproj_threshold);
  if (!(confidence > 0.0) || !(confidence < 1.0)) return set_error(VDO_ERR_INVALID, "%s: confidence %g outside (0, 1)", who, confidence);
  if (min_inliers < 0) return set_error(VDO_ERR_INVALID, "%s: min_inliers %d < 0", who, min_inliers);
  if (!T) return set_error(VDO_ERR_INVALID, "%s: T is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const int W = h->W, H = h->H;
  const int nx = step / 2 < W ? (W - 1 - step / 2) / step + 1 : 0, ny = step / 2 < H ? (H - 1 - step / 2) / step + 1 : 0;
  const int ngrid = nx * ny, nblk = (ngrid + 255) / 256;
  double* dX = (double*)(h->d_smp + 8);
  double* dUV = dX + 3 * (size_t)ngrid;
  int32_t n = 0;
  const auto t0 = h->tm.begin(s);
  if (ngrid > 0) {
    const MsSources src = ms_stage(h, s, disp0, disp0_stride_floats, flow, flow_stride_floats, flow_valid, flow_valid_stride, src_is_device);
    hipLaunchKernelGGL(k_ms_samples<false>, dim3(nblk), dim3(256), 0, s, h->a, src.disp0, src.flow, src.valid, W, H, step, nx, ngrid, h->d_blk, dX, dUV);
    hipLaunchKernelGGL(k_ms_scan, dim3(1), dim3(1024), 0, s, h->d_blk, nblk, (int32_t*)h->d_smp);
    hipLaunchKernelGGL(k_ms_samples<true>, dim3(nblk), dim3(256), 0, s, h->a, src.disp0, src.flow, src.valid, W, H, step, nx, ngrid, h->d_blk, dX, dUV);
    h->tm.mark_end(s);
    // one download: the count and both lists at the grid's capacity
    hipMemcpyAsync(h->h_smp, h->d_smp, 8 + (size_t)ngrid * 5 * sizeof(double), hipMemcpyDeviceToHost, s);
  } else {
    h->tm.mark_end(s);
  }
  rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  if (ngrid > 0) std::memcpy(&n, h->h_smp, sizeof n);
  else std::memset(h->h_smp, 0, 8);
  h->smp_cap = ngrid;
  vdo_pnp_problem pr{};
  pr.n = n; pr.X = (const double*)(h->h_smp + 8); pr.uv = pr.X + 3 * (size_t)ngrid;
  pr.K[0] = h->p.K[0]; pr.K[1] = h->p.K[1]; pr.K[2] = h->p.K[2]; pr.K[3] = h->p.K[3];
  pr.max_iterations = max_iterations; pr.reproj_threshold = reproj_threshold; pr.confidence = confidence; pr.refit = 1;
  vdo_pnp_result r{};
  rc = vdo_pnp_ransac(h->ctx, &pr, &r, nullptr);
  if (rc != VDO_OK) return rc;
  const bool found = r.n_inliers >= min_inliers && r.best_iteration >= 0;
  for (int k = 0; k < 16; ++k) T[k] = found ? (float)r.T[k] : (k % 5 == 0 ? 1.f : 0.f);
  out[0] = n; out[1] = r.n_inliers; out[2] = r.iterations_run;
  h->tm.finish(t0);
  return VDO_OK;
}

extern "C" int vdo_motionseg_compute(vdo_motionseg* h, const float* disp0, int64_t disp0_stride_floats, const float* disp1, int64_t disp1_stride_floats, const float* flow,
                                     int64_t flow_stride_floats, const uint8_t* flow_valid, int64_t flow_valid_stride, int src_is_device, const float T[16], uint8_t* cls,
                                     int out_is_device, int32_t out[3]) {
  static const char* who = "vdo_motionseg_compute";
  int rc = ms_check_sources(who, h, disp0, disp0_stride_floats, flow, flow_stride_floats, flow_valid, flow_valid_stride);
  if (rc != VDO_OK) return rc;
  if (!disp1) return set_error(VDO_ERR_INVALID, "%s: disp1 is null", who);
  if (disp1_stride_floats < h->W) return set_error(VDO_ERR_INVALID, "%s: disp1_stride_floats %lld smaller than the width %d", who, (long long)disp1_stride_floats, h->W);
  if (!T) return set_error(VDO_ERR_INVALID, "%s: T is null", who);
  if (!cls) return set_error(VDO_ERR_INVALID, "%s: cls is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const int W = h->W, H = h->H, n = W * H, nblk = (n + 255) / 256;
  const int tiles_x = (W + kMsTW - 1) / kMsTW, tiles_y = (H + kMsTH - 1) / kMsTH;
  MsArgs a = h->a;
  for (int k = 0; k < 12; ++k) a.T[k] = T[k];
  const auto t0 = h->tm.begin(s);
  const MsSources src = ms_stage(h, s, disp0, disp0_stride_floats, flow, flow_stride_floats, flow_valid, flow_valid_stride, src_is_device);
  const float* d_disp1 = stage_rows(s, h->d_disp1, disp1, disp1_stride_floats, W, H, src_is_device);
  uint8_t* d_cls = out_is_device ? cls : h->d_cls;
  hipMemsetAsync(h->d_cnt, 0, kMsCounters * sizeof(int32_t), s);
  hipLaunchKernelGGL(k_ms_residual, dim3(nblk), dim3(256), 0, s, a, src.disp0, d_disp1, src.flow, src.valid, W, H, h->d_state, h->d_res, h->d_cnt);
  const vdo_motionseg_params& p = h->p;
  hipLaunchKernelGGL(k_ms_vote, dim3(tiles_x * tiles_y), dim3(256), 0, s, (const uint8_t*)h->d_state, W, H, tiles_x, p.vote_radius, p.vote_num, p.vote_den, p.min_known, p.class_value,
                     d_cls, h->d_cnt);
  h->tm.mark_end(s);
  if (!out_is_device) hipMemcpyAsync(cls, h->d_cls, (size_t)n, hipMemcpyDeviceToHost, s);
  hipMemcpyAsync(h->h_cnt, h->d_cnt, kMsCounters * sizeof(int32_t), hipMemcpyDeviceToHost, s);
  rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  out[0] = h->h_cnt[kMsMoving]; out[1] = h->h_cnt[kMsStatic]; out[2] = h->h_cnt[kMsUnknown];
  h->tm.finish(t0);
  h->computed = true;
  return VDO_OK;
}

static int ms_fetch(const char* who, vdo_motionseg* h, const void* dev, size_t bytes, void* out) {
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (!h->computed) return set_error(VDO_ERR_INVALID, "%s: no vdo_motionseg_compute on this handle yet", who);
  const int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, h->ctx->stream);
  return check_hip(who, hipStreamSynchronize(h->ctx->stream));
}

extern "C" int vdo_motionseg_get_state(vdo_motionseg* h, uint8_t* out) { return ms_fetch("vdo_motionseg_get_state", h, h ? h->d_state : nullptr, h ? (size_t)h->W * h->H : 0, out); }

extern "C" int vdo_motionseg_get_residual(vdo_motionseg* h, float* out) {
  return ms_fetch("vdo_motionseg_get_residual", h, h ? h->d_res : nullptr, h ? (size_t)h->W * h->H * sizeof(float) : 0, out);
}

extern "C" int vdo_motionseg_get_samples(vdo_motionseg* h, double* X, double* uv, int32_t* n) {
  static const char* who = "vdo_motionseg_get_samples";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!n) return set_error(VDO_ERR_INVALID, "%s: n is null", who);
  if (h->smp_cap < 0) return set_error(VDO_ERR_INVALID, "%s: no vdo_motionseg_egomotion on this handle yet", who);
  int32_t cnt = 0;
  std::memcpy(&cnt, h->h_smp, sizeof cnt);
  const double* hX = (const double*)(h->h_smp + 8);
  if (X && cnt) std::memcpy(X, hX, (size_t)cnt * 3 * sizeof(double));
  if (uv && cnt) std::memcpy(uv, hX + 3 * (size_t)h->smp_cap, (size_t)cnt * 2 * sizeof(double));
  *n = cnt;
  return VDO_OK;
}

extern "C" int vdo_motionseg_last_timing(vdo_motionseg* h, double ms[2]) {
  return last_timing("vdo_motionseg_last_timing", h ? &h->tm : nullptr, ms);
}

extern "C" int vdo_motionseg_device_images(vdo_motionseg* h, float** disp1, uint8_t** next_right, uint8_t** cls) {
  if (!h) return set_error(VDO_ERR_INVALID, "vdo_motionseg_device_images: handle is null");
  if (disp1) *disp1 = h->d_disp1;
  if (next_right) *next_right = h->d_right;
  if (cls) *cls = h->d_cls;
  return VDO_OK;
}
