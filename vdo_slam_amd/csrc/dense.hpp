// What the dense mapper (dense.hip) and the views onto its volume (raycast.hip) share: the handle, the kernel arguments and the index helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"
#include "stage.hpp"

namespace vdo {

constexpr int kDnMaxSide = 1 << 12;
constexpr int64_t kDnMaxVoxels = int64_t(1) << 31;
constexpr int kDnMaxOrigin = 1 << 22;                                      // every |g| in use stays below it: (float)g + 0.5f is exact
constexpr int kDnZ = 4;                                                    // z slots per workgroup of k_dn_integrate
enum { kDnUpdated = 0, kDnMasked, kDnOccluded, kDnCounters = 4 };
constexpr int kDnSlots = 1024;                                             // the counters of k_dn_integrate are kept kDnSlots times, 32 bytes apart; the host adds them up
constexpr int kDnTotal = kDnSlots * kDnCounters;                           // then the point count of k_counts_scan

// what the kernels take by value
struct DnArgs {
  float fx, fy, cx, cy, trunc, min_z, min_d, max_d, voxel;
  int max_w;
  float T[12];
  int n[3], o[3], om[3];                                                   // size, origin, origin mod size (non-negative)
};

}  // namespace vdo

struct vdo_dense {
  vdo_ctx* ctx = nullptr;
  int W = 0, H = 0;
  vdo_dense_params p{};
  vdo::DnArgs a{};
  int vpt = 4;
  int64_t nvox = 0, stage_points = 0;
  uint32_t* d_vol = nullptr;                              // [nz][ny][nx] words in slot order
  float* d_depth = nullptr;                               // [H][W] staging
  int32_t* d_mask = nullptr;                              // [H][W] staging
  long long* d_blk = nullptr;                             // per 256 voxels of a box: its points, then their exclusive scan
  unsigned long long* d_cnt = nullptr;                    // [kDnSlots][kDnCounters], then the point count of the last extraction
  unsigned long long* h_cnt = nullptr;                    // pinned
  float* d_xyz = nullptr; int32_t* d_grad = nullptr; int32_t* d_wgt = nullptr;      // [stage_points] staging of host outputs
  vdo::StageTimer tm;
};

namespace vdo {

__device__ __forceinline__ bool dn_finite(float v) { return fabsf(v) <= FLT_MAX; }       // false for NaN and the infinities

__device__ __forceinline__ int dn_floor_div(int a, int d) { return a >= 0 ? a / d : -((-a + d - 1) / d); }      // d > 0

// slot -> global voxel on one axis: the one g in [o, o + n) with g mod n == s
__device__ __forceinline__ int dn_global(int s, int o, int om, int n) { return o + (s - om) + (s < om ? n : 0); }

// The per-voxel arithmetic of the fusion, shared by k_dn_integrate (dense.hip) and k_ob_integrate (objects.hip) so that both produce the same bits.
// The pixel a camera-frame point falls on, as floats (exact integers); false unless Zc is finite and above min_z, u and v are finite and the rounded
// pixel lies in the image - compared as floats, so (int)xq, (int)yq are safe after a true.
__device__ __forceinline__ bool dn_pixel(const DnArgs& a, float Xc, float Yc, float Zc, int W, int H, float* xq, float* yq) {
  if (!(dn_finite(Zc) && Zc > a.min_z)) return false;
  const float u = (a.fx * Xc) / Zc + a.cx, v = (a.fy * Yc) / Zc + a.cy;
  *xq = floorf(u + 0.5f); *yq = floorf(v + 0.5f);
  return dn_finite(u) && dn_finite(v) && *xq >= 0.f && *xq <= (float)(W - 1) && *yq >= 0.f && *yq <= (float)(H - 1);
}

__device__ __forceinline__ bool dn_depth_ok(const DnArgs& a, float d) { return dn_finite(d) && d > a.min_d && d <= a.max_d; }

// One usable depth d seen from a voxel at camera depth Zc: false when the voxel is occluded (s < -trunc), else *nw is the word after the running mean.
__device__ __forceinline__ bool dn_fuse(const DnArgs& a, float d, float Zc, uint32_t word, uint32_t* nw) {
  float s = d - Zc;
  if (s < -a.trunc) return false;
  s = fminf(s, a.trunc);
  const int q = (int)floorf((s / a.trunc) * 32767.0f + 0.5f);
  const int t = (int)(int16_t)(word & 0xffffu), w = (int)(word >> 16);
  const int t1 = dn_floor_div(2 * (t * w + q) + (w + 1), 2 * (w + 1));      // |t|, |q| <= 32767, w <= 255: below 2^25
  const int w1 = w + 1 < a.max_w ? w + 1 : a.max_w;
  *nw = ((uint32_t)w1 << 16) | ((uint32_t)t1 & 0xffffu);
  return true;
}

// The camera centre of T (4 x 4 row-major, world -> camera) as the raycaster states it: c_a = -((T0a*T03 + T1a*T13) + T2a*T23).  Host, once per call.
inline void dn_centre(const float T[16], float c[3]) {
  for (int a = 0; a < 3; ++a) c[a] = -((T[a] * T[3] + T[4 + a] * T[7]) + T[8 + a] * T[11]);
}

// The world-frame ray of pixel (x, y), camera-z component 1: r_a = (T0a*dx + T1a*dy) + T2a with R[3 * i + a] = T(i, a).  A view's kernel and the
// aligner's model point (c_a + depth * r_a) share it, so that both name the same point bit for bit.
__device__ __forceinline__ void dn_ray(float x, float y, float fx, float fy, float cx, float cy, const float R[9], float r[3]) {
  const float dx = (x - cx) / fx, dy = (y - cy) / fy;
#pragma unroll
  for (int a = 0; a < 3; ++a) r[a] = (R[a] * dx + R[3 + a] * dy) + R[6 + a];
}

// What another handle needs of a view (raycast.hip): its image size, its intrinsics (fx, fy, cx, cy) and the context of its map
void rc_view_info(const vdo_raycast* view, int* W, int* H, float K[4], vdo_ctx** ctx);

}  // namespace vdo
