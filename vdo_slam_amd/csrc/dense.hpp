// The contract of the TSDF volume (vdo_dense), written once for everything that reads or writes one: the mapper (dense.hip), the raycaster
// (raycast.hip), the object mapper (objects.hip), the mesher (mesh.hip), the colourer (colour.hip) and the distance field (distance.hip); the aligner
// (align.hip) takes dn_finite, dn_ray and dn_centre.  Device: slot addressing, the word's halves, the guard before a float becomes a voxel index,
// the fusion arithmetic.  Host: the size refusals, the clipped box and the move (dense_plan.hpp), the queue of a move, the sharded counters.
// LEFT ALONE ON PURPOSE: (1) the windowed host-staging loops of vdo_dense_extract, vdo_mesh_extract (two), vdo_colour_sample, vdo_colour_render and
// vdo_distance_sample look alike but differ in what is copied in and out: a helper general enough for all six is more machinery than the loops;
// (2) the traversal and the workgroup counts of k_dn_integrate, k_cl_integrate and k_ob_integrate: every shared spelling that was tried costs the
// mapper an instruction or moves a register count (profiles/volume_header.txt), so the three keep their own text over dn_pixel / dn_depth_ok / dn_fuse.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"
#include "stage.hpp"
#include "dense_plan.hpp"

namespace vdo {

typedef unsigned long long u64;
constexpr int kDnMaxSide = 1 << 12;
constexpr int64_t kDnMaxVoxels = int64_t(1) << 31;
constexpr int kDnMaxOrigin = 1 << 22;                                      // every |g| in use stays below it: (float)g + 0.5f is exact
constexpr int kDnZ = 4;                                                    // z slots per workgroup of the integrate kernels
enum { kDnUpdated = 0, kDnMasked, kDnOccluded, kDnCounters = 4 };
constexpr int kDnSlots = 1024;                                             // the counters of k_dn_integrate and of the colourer are kept kDnSlots times, 32 bytes apart

// what the kernels take by value
struct DnArgs {
  float fx, fy, cx, cy, trunc, min_z, min_d, max_d, voxel;
  int max_w;
  float T[12];
  int n[3], o[3], om[3];                                                   // size, origin, origin mod size (non-negative)
};

// Counters that a kernel adds to on one of `slots` copies, `counters` words (32 bytes for 4) apart, so that its atomics do not queue on one address;
// the host adds the copies up.  One spare word follows the copies for a total a handle keeps beside them (vdo_dense_extract): zero() and download()
// leave it alone.
struct SlotCounts {
  unsigned long long *d = nullptr, *h = nullptr;                           // on the device; pinned
  int slots = 0, counters = 0;
  size_t words() const { return (size_t)slots * counters; }
  bool create(int slots_, int counters_) {
    slots = slots_; counters = counters_;
    return hipMalloc((void**)&d, (words() + 1) * 8) == hipSuccess && hipHostMalloc((void**)&h, (words() + 1) * 8, hipHostMallocDefault) == hipSuccess;
  }
  void destroy() { hipFree(d); if (h) hipHostFree(h); }
  void zero(hipStream_t s) { hipMemsetAsync(d, 0, words() * 8, s); }
  void download(hipStream_t s) { hipMemcpyAsync(h, d, words() * 8, hipMemcpyDeviceToHost, s); }
  int64_t sum(int k) const { unsigned long long t = 0; for (int i = 0; i < slots; ++i) t += h[(size_t)i * counters + k]; return (int64_t)t; }      // after the download
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
  vdo::SlotCounts cnt;                                    // [kDnSlots][kDnCounters]; the spare word is the point count of the last extraction
  float* d_xyz = nullptr; int32_t* d_grad = nullptr; int32_t* d_wgt = nullptr;      // [stage_points] staging of host outputs
  vdo::StageTimer tm;
};

namespace vdo {

__device__ __forceinline__ bool dn_finite(float v) { return fabsf(v) <= FLT_MAX; }       // false for NaN and the infinities

__device__ __forceinline__ int dn_floor_div(int a, int d) { return a >= 0 ? a / d : -((-a + d - 1) / d); }      // d > 0

// THE SLOT RULE.  The global voxel g, o <= g < o + n, lives at slot (g mod n) of its axis: with l = g - o its local index and om = o mod n that is
// om + l, minus n when it passes n.  Nothing else in the library turns a voxel into an address.
__device__ __forceinline__ int dn_wrap(int s, int n) { return s >= n ? s - n : s; }      // 0 <= s < 2 n
__device__ __forceinline__ int dn_slot(int l, int om, int n) { return dn_wrap(om + l, n); }

__device__ __forceinline__ int dn_next(int s, int n) { return s + 1 == n ? 0 : s + 1; }      // the slot after s: the voxel one up on the axis

// slot -> global voxel on one axis: the one g in [o, o + n) with g mod n == s
__device__ __forceinline__ int dn_global(int s, int o, int om, int n) { return o + (s - om) + (s < om ? n : 0); }

// the word of the voxel at local (x, y, z), each inside [0, n)
__device__ __forceinline__ uint32_t dn_word(const uint32_t* __restrict__ vol, const int n[3], const int om[3], int x, int y, int z) {
  int sx = om[0] + x, sy = om[1] + y, sz = om[2] + z;                       // dn_slot per axis, the three sums first: the order the kernels were scheduled in
  sx = dn_wrap(sx, n[0]); sy = dn_wrap(sy, n[1]); sz = dn_wrap(sz, n[2]);
  return vol[((size_t)sz * n[1] + sy) * n[0] + sx];
}

// a word's two halves: the signed distance in units of trunc / 32767, the weight
__device__ __forceinline__ int dn_tsdf(uint32_t w) { return (int)(int16_t)(w & 0xffffu); }
__device__ __forceinline__ float dn_tsdf_f(uint32_t w) { return (float)dn_tsdf(w); }
__device__ __forceinline__ int dn_weight(uint32_t w) { return (int)(w >> 16); }

// true when the floor fl of a voxel coordinate computed from the finite p may become an int index: inside [-2^22, 2^22), where every volume lies
__device__ __forceinline__ bool dn_indexable(float p, float fl) { return dn_finite(p) && fl >= -(float)kDnMaxOrigin && fl <= (float)(kDnMaxOrigin - 1); }

// The per-voxel arithmetic that k_dn_integrate (dense.hip), k_ob_integrate (objects.hip) and k_cl_integrate (colour.hip) share bit for bit.
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
  const int t = dn_tsdf(word), w = dn_weight(word);
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

// The size refusals of every handle that holds a volume's worth of anything, in the two places a create call makes them among its other refusals
inline int dn_check_sides(const char* who, const int32_t n[3]) {
  for (int k = 0; k < 3; ++k) if (n[k] < 1) return set_error(VDO_ERR_INVALID, "%s: n[%d] = %d < 1", who, k, n[k]);
  return VDO_OK;
}
inline int dn_check_size(const char* who, const int32_t n[3], int64_t* nvox) {
  for (int k = 0; k < 3; ++k) if (n[k] > kDnMaxSide) return set_error(VDO_ERR_UNSUPPORTED, "%s: n[%d] = %d exceeds 2^12", who, k, n[k]);
  *nvox = (int64_t)n[0] * n[1] * n[2];
  if (*nvox > kDnMaxVoxels) return set_error(VDO_ERR_UNSUPPORTED, "%s: %d x %d x %d voxels exceed 2^31", who, n[0], n[1], n[2]);
  return VDO_OK;
}

inline DnClip dn_clip(const vdo_dense* map, const int32_t lo[3], const int32_t hi[3]) { return dn_clip(map->a.n, map->a.o, lo, hi); }

// dense.hip: queues what a move of the origin of `words` ([nz][ny][nx] in slot order) makes stale (dn_move): a memset, or a k_dn_clear per slab
void dn_queue_move(hipStream_t s, uint32_t* words, const int n[3], int64_t nvox, const int from[3], const int to[3]);

// What another handle needs of a view (raycast.hip): its image size, its intrinsics (fx, fy, cx, cy) and the context of its map
void rc_view_info(const vdo_raycast* view, int* W, int* H, float K[4], vdo_ctx** ctx);

// What the joint solve needs of an aligner (align.hip): its frame size, its min_pixels, whether a model is set, and its context
void al_info(const vdo_align* h, int* W, int* H, int* min_pixels, bool* has_model, vdo_ctx** ctx);

}  // namespace vdo
