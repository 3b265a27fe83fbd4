// What the dense mapper (dense.hip) and the views onto its volume (raycast.hip) share: the handle, the kernel arguments and the index helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"

namespace vdo {

constexpr int kDnMaxSide = 1 << 12;
constexpr int64_t kDnMaxVoxels = int64_t(1) << 31;
constexpr int kDnMaxOrigin = 1 << 22;                                      // every |g| in use stays below it: (float)g + 0.5f is exact
constexpr int64_t kDnMaxPixels = int64_t(1) << 26;
constexpr int kDnMaxImageSide = 1 << 24;                                   // (float)(W - 1) is exact
constexpr int kDnZ = 4;                                                    // z slots per workgroup of k_dn_integrate
enum { kDnUpdated = 0, kDnMasked, kDnOccluded, kDnCounters = 4 };
constexpr int kDnSlots = 1024;                                             // the counters of k_dn_integrate are kept kDnSlots times, 32 bytes apart; the host adds them up
constexpr int kDnTotal = kDnSlots * kDnCounters;                           // then the point count of k_dn_scan

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
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double ms[2] = {0, 0};
};

namespace vdo {

__device__ __forceinline__ bool dn_finite(float v) { return fabsf(v) <= FLT_MAX; }       // false for NaN and the infinities

__device__ __forceinline__ int dn_floor_div(int a, int d) { return a >= 0 ? a / d : -((-a + d - 1) / d); }      // d > 0

// slot -> global voxel on one axis: the one g in [o, o + n) with g mod n == s
__device__ __forceinline__ int dn_global(int s, int o, int om, int n) { return o + (s - om) + (s < om ? n : 0); }

}  // namespace vdo
