// Object mapper, device stage: per-label statistics of a frame's mask (pixel count, pixel box, fixed-point sums of the back-projected points) and
// ONE label-selecting TSDF fusion launch over a batch of object volumes.  An object's volume is a plain vdo_dense (dense.hpp); this handle owns the
// tables, the counters and the image staging.  The semantics are stated in include/vdo_slam_hip.h (vdo_objects_*) and restated in NumPy by
// tests/objects_ref.py.  Everything accumulated is an integer: no result depends on workgroup shape, on the schedule or on the culling.
//
//   k_ob_stats_reset     one thread per row of the table: (0, W, H, -1, -1, 0, 0, 0).
//   k_ob_stats           one thread per pixel, a wave = 64 consecutive pixels of the packed image.  The lanes of a wave that carry the same label
//                        are combined in registers (a loop over the wave's distinct labels: ballot, xor-shuffle butterfly with the identity in the
//                        other lanes), then one lane issues the row's eight 64-bit atomics.  Background waves leave after one ballot.
//   k_ob_integrate<VPT>  k_dn_integrate's shape per object (x on the lanes, 4 z per workgroup, VPT y per thread), the object index on blockIdx.x /
//                        xblocks; the entry (the map's DnArgs with this call's T, the volume, the label, the label's box) is read from a device
//                        table at a workgroup-uniform address.  Workgroups outside an object's own volume return at once.  The per-voxel arithmetic
//                        is dense.hpp's dn_pixel / dn_depth_ok / dn_fuse.  Counts by wave ballot, LDS over the workgroup, one atomic per workgroup
//                        and counter on one of kObSlots copies per object.
//
// NO OUT-OF-RANGE ACCESS: dn_pixel compares floats against 0 and W - 1 / H - 1 before any conversion to int; every volume index is built from slot
// coordinates tested against the object's n; a stats row is addressed by a label tested against 1..max_labels.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"
#include "frame_images.hpp"
#include "stage.hpp"
#include "dense.hpp"

namespace vdo {

constexpr int kObSlots = 64;                                               // copies of an object's two counters; the host adds them up
constexpr int kObVpt = 4;
constexpr int kObRow = 8;

struct ObEntry {
  DnArgs a;
  uint32_t* vol;
  int label, slot;                                                         // slot: the object's place in the caller's batch (its counters)
  float bx0, by0, bx1, by1;                                                // the label's pixel box (the whole image when culling is off)
};

struct ObStatArgs { float fx, fy, cx, cy, min_d, max_d; int max_labels; };

__global__ __launch_bounds__(256) void k_ob_stats_reset(long long* __restrict__ tab, int rows, int W, int H) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  long long* t = tab + (size_t)r * kObRow;
  t[0] = 0; t[1] = W; t[2] = H; t[3] = -1; t[4] = -1; t[5] = 0; t[6] = 0; t[7] = 0;
}

__device__ __forceinline__ int ob_min_xor(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(v, m); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ int ob_max_xor(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(v, m); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ long long ob_sum_xor(long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__global__ __launch_bounds__(256) void k_ob_stats(const float* __restrict__ depth, const int32_t* __restrict__ mask, int W, int H, ObStatArgs s, long long* __restrict__ tab) {
  const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;   // W * H <= 2^26
  int l = 0, x = 0, y = 0;
  bool other = false;
  long long qx = 0, qy = 0, qz = 0;
  if (i < W * H) {
    const float d = depth[i];
    if (dn_finite(d) && d > s.min_d && d <= s.max_d) {
      const int m = mask[i];
      if (m >= 1 && m <= s.max_labels) {
        l = m; y = i / W; x = i - y * W;
        qx = (long long)floorf(((((float)x - s.cx) * d) / s.fx) * 1024.f + 0.5f);
        qy = (long long)floorf(((((float)y - s.cy) * d) / s.fy) * 1024.f + 0.5f);
        qz = (long long)floorf(d * 1024.f + 0.5f);
      } else if (m != 0) {
        other = true;
      }
    }
  }
  const unsigned long long bo = __ballot(other);
  if (bo && lane == __ffsll((long long)bo) - 1) __hip_atomic_fetch_add(tab, (long long)__popcll(bo), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  unsigned long long pending = __ballot(l != 0);
  while (pending) {                                                        // wave-uniform: one round per distinct label of the wave
    const int leader = __ffsll((long long)pending) - 1;
    const int cur = __shfl(l, leader);                                     // != 0
    const bool mine = l == cur;
    const unsigned long long bm = __ballot(mine);
    const int x0 = ob_min_xor(mine ? x : INT_MAX), y0 = ob_min_xor(mine ? y : INT_MAX), x1 = ob_max_xor(mine ? x : -1), y1 = ob_max_xor(mine ? y : -1);
    const long long sx = ob_sum_xor(mine ? qx : 0), sy = ob_sum_xor(mine ? qy : 0), sz = ob_sum_xor(mine ? qz : 0);
    if (lane == leader) {
      long long* t = tab + (size_t)cur * kObRow;                           // 1 <= cur <= max_labels
      __hip_atomic_fetch_add(t + 0, (long long)__popcll(bm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_min(t + 1, (long long)x0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_min(t + 2, (long long)y0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_max(t + 3, (long long)x1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_max(t + 4, (long long)y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(t + 5, sx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(t + 6, sy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(t + 7, sz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    pending &= ~bm;
  }
}

template <int VPT>
__global__ __launch_bounds__(256) void k_ob_integrate(const ObEntry* __restrict__ tab, int xblocks, const float* __restrict__ depth, const int32_t* __restrict__ mask, int W, int H,
                                                      unsigned long long* __restrict__ cnt) {
  const int ob = blockIdx.x / xblocks, bxi = blockIdx.x - ob * xblocks;    // ob < the table's length: the grid's x is its length * xblocks
  const ObEntry& e = tab[ob];
  const DnArgs& a = e.a;
  const int nx = a.n[0], ny = a.n[1], nz = a.n[2];
  const int sy0 = blockIdx.y * VPT;
  if (bxi * 64 >= nx || sy0 >= ny || (int)blockIdx.z * kDnZ >= nz) return; // the grid is sized for the largest volume of the batch
  const int sx = bxi * 64 + threadIdx.x, sz = blockIdx.z * kDnZ + threadIdx.z;
  const int label = e.label;
  uint32_t* __restrict__ vol = e.vol;
  const bool in_xz = sx < nx && sz < nz;
  float ax = 0.f, ay = 0.f, az = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
  if (in_xz) {
    const float px = ((float)dn_global(sx, a.o[0], a.om[0], nx) + 0.5f) * a.voxel, pz = ((float)dn_global(sz, a.o[2], a.om[2], nz) + 0.5f) * a.voxel;
    ax = a.T[0] * px; ay = a.T[4] * px; az = a.T[8] * px;
    bx = a.T[2] * pz + a.T[3]; by = a.T[6] * pz + a.T[7]; bz = a.T[10] * pz + a.T[11];
  }
  const size_t row0 = ((size_t)(in_xz ? sz : 0) * ny) * nx + (in_xz ? sx : 0);
  int n_upd = 0, n_occ = 0;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int sy = sy0 + k;
    bool upd = false, occ = false;
    if (in_xz && sy < ny) {
      const float py = ((float)dn_global(sy, a.o[1], a.om[1], ny) + 0.5f) * a.voxel;
      const float Xc = (ax + a.T[1] * py) + bx, Yc = (ay + a.T[5] * py) + by, Zc = (az + a.T[9] * py) + bz;
      float xq, yq;
      if (dn_pixel(a, Xc, Yc, Zc, W, H, &xq, &yq) && xq >= e.bx0 && xq <= e.bx1 && yq >= e.by0 && yq <= e.by1) {
        const int j = (int)yq * W + (int)xq;
        if (mask[j] == label) {                                            // most voxels of an object's volume see another label: its depth is not read
          const float d = depth[j];
          if (dn_depth_ok(a, d)) {
            const size_t at = row0 + (size_t)sy * nx;
            const uint32_t word = vol[at];
            uint32_t nw;
            if (!dn_fuse(a, d, Zc, word, &nw)) {
              occ = true;
            } else {
              if (nw != word) vol[at] = nw;
              upd = true;
            }
          }
        }
      }
    }
    n_upd += (int)__popcll(__ballot(upd)); n_occ += (int)__popcll(__ballot(occ));
  }
  __shared__ int red[kDnZ][2];
  if (threadIdx.x == 0) { red[threadIdx.z][0] = n_upd; red[threadIdx.z][1] = n_occ; }
  __syncthreads();
  if (threadIdx.x < 2 && threadIdx.z == 0) {
    int sum = 0;
    for (int z = 0; z < kDnZ; ++z) sum += red[z][threadIdx.x];
    const unsigned slot = (bxi + xblocks * (blockIdx.y + gridDim.y * blockIdx.z)) & (unsigned)(kObSlots - 1);
    if (sum) atomicAdd(cnt + ((size_t)e.slot * kObSlots + slot) * 2 + threadIdx.x, (unsigned long long)sum);
  }
}

}  // namespace vdo

struct vdo_objects {
  vdo_ctx* ctx = nullptr;
  int W = 0, H = 0;
  vdo_objects_params p{};
  vdo::ObStatArgs sa{};
  int rows = 0, cull = 0;
  bool have_stats = false;
  float* d_depth = nullptr;                               // [H][W] staging
  int32_t* d_mask = nullptr;                              // [H][W] staging
  long long* d_stats = nullptr;                           // [max_labels + 1][8]
  long long* h_stats = nullptr;                           // pinned
  vdo::ObEntry* d_tab = nullptr;                          // [max_batch]
  vdo::ObEntry* h_tab = nullptr;                          // pinned
  unsigned long long* d_cnt = nullptr;                    // [max_batch][kObSlots][2]
  unsigned long long* h_cnt = nullptr;                    // pinned
  vdo::StageTimer tm;
};

namespace vdo {

static void ob_free(vdo_objects* h) {
  hipFree(h->d_depth); hipFree(h->d_mask); hipFree(h->d_stats); hipFree(h->d_tab); hipFree(h->d_cnt);
  if (h->h_stats) hipHostFree(h->h_stats);
  if (h->h_tab) hipHostFree(h->h_tab);
  if (h->h_cnt) hipHostFree(h->h_cnt);
  h->tm.destroy();
  delete h;
}

static int ob_check_batch(const char* who, const vdo_objects* h, int n, vdo_dense* const* maps, const int32_t* labels, const float* T, const int64_t* out) {
  if (n < 0 || n > h->p.max_batch) return set_error(VDO_ERR_INVALID, "%s: n %d outside 0..max_batch %d", who, n, h->p.max_batch);
  if (n == 0) return VDO_OK;
  if (!maps) return set_error(VDO_ERR_INVALID, "%s: maps is null", who);
  if (!labels) return set_error(VDO_ERR_INVALID, "%s: labels is null", who);
  if (!T) return set_error(VDO_ERR_INVALID, "%s: T is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  for (int i = 0; i < n; ++i) {
    const vdo_dense* m = maps[i];
    if (!m) return set_error(VDO_ERR_INVALID, "%s: maps[%d] is null", who, i);
    for (int j = 0; j < i; ++j)
      if (maps[j] == m) return set_error(VDO_ERR_INVALID, "%s: maps[%d] is maps[%d]: a map may appear once in a batch", who, i, j);
    if (m->ctx != h->ctx) return set_error(VDO_ERR_INVALID, "%s: maps[%d] belongs to another context", who, i);
    if (m->W != h->W || m->H != h->H) return set_error(VDO_ERR_INVALID, "%s: maps[%d] takes %d x %d images, the stage's are %d x %d", who, i, m->W, m->H, h->W, h->H);
    if (m->p.min_depth < h->p.min_depth || m->p.max_depth > h->p.max_depth)
      return set_error(VDO_ERR_INVALID, "%s: maps[%d]: depth range (%g, %g] outside the stage's (%g, %g]", who, i, (double)m->p.min_depth, (double)m->p.max_depth,
                       (double)h->p.min_depth, (double)h->p.max_depth);
    if (labels[i] < 1 || labels[i] > h->p.max_labels) return set_error(VDO_ERR_INVALID, "%s: labels[%d] = %d outside 1..max_labels %d", who, i, labels[i], h->p.max_labels);
  }
  return VDO_OK;
}

// The stats pass and its download; the table is in h_stats afterwards
static int ob_stats(const char* who, vdo_objects* h, const float* d_depth, const int32_t* d_mask) {
  hipStream_t s = h->ctx->stream;
  const int npix = h->W * h->H;
  hipLaunchKernelGGL(k_ob_stats_reset, dim3((h->rows + 255) / 256), dim3(256), 0, s, h->d_stats, h->rows, h->W, h->H);
  hipLaunchKernelGGL(k_ob_stats, dim3((npix + 255) / 256), dim3(256), 0, s, d_depth, d_mask, h->W, h->H, h->sa, h->d_stats);
  h->tm.mark_end(s);
  hipMemcpyAsync(h->h_stats, h->d_stats, (size_t)h->rows * kObRow * sizeof(long long), hipMemcpyDeviceToHost, s);
  const int rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  h->have_stats = true;
  return VDO_OK;
}

static void ob_finish(vdo_objects* h, StageClock::time_point t0, int64_t* stats) {
  if (stats) std::memcpy(stats, h->h_stats, (size_t)h->rows * kObRow * sizeof(long long));
  h->tm.finish(t0);
}

// After the stats: the table of the objects that get work, one launch, the counts
static int ob_fuse(const char* who, vdo_objects* h, const float* d_depth, const int32_t* d_mask, int n, vdo_dense* const* maps, const int32_t* labels, const float* T, int64_t* out) {
  hipStream_t s = h->ctx->stream;
  int m = 0, big[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const long long* row = h->h_stats + (size_t)labels[i] * kObRow;
    out[3 * i + 0] = 0; out[3 * i + 1] = 0; out[3 * i + 2] = row[0];
    if (h->cull && row[0] == 0) continue;
    ObEntry& e = h->h_tab[m++];
    e.a = maps[i]->a;
    for (int k = 0; k < 12; ++k) e.a.T[k] = T[16 * i + k];
    e.vol = maps[i]->d_vol; e.label = labels[i]; e.slot = i;
    e.bx0 = h->cull ? (float)row[1] : 0.f; e.by0 = h->cull ? (float)row[2] : 0.f;
    e.bx1 = h->cull ? (float)row[3] : (float)(h->W - 1); e.by1 = h->cull ? (float)row[4] : (float)(h->H - 1);
    for (int k = 0; k < 3; ++k) big[k] = e.a.n[k] > big[k] ? e.a.n[k] : big[k];
  }
  if (m == 0) return VDO_OK;
  hipMemcpyAsync(h->d_tab, h->h_tab, (size_t)m * sizeof(ObEntry), hipMemcpyHostToDevice, s);
  hipMemsetAsync(h->d_cnt, 0, (size_t)n * kObSlots * 2 * sizeof(unsigned long long), s);
  const int xblocks = (big[0] + 63) / 64;                                  // <= 64, times m <= 64
  const dim3 grid((unsigned)(xblocks * m), (big[1] + kObVpt - 1) / kObVpt, (big[2] + kDnZ - 1) / kDnZ);
  hipLaunchKernelGGL(k_ob_integrate<kObVpt>, grid, dim3(64, 1, kDnZ), 0, s, (const ObEntry*)h->d_tab, xblocks, d_depth, d_mask, h->W, h->H, h->d_cnt);
  h->tm.mark_end(s);
  hipMemcpyAsync(h->h_cnt, h->d_cnt, (size_t)n * kObSlots * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
  const int rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 2; ++k) {
      unsigned long long sum = 0;
      for (int slot = 0; slot < kObSlots; ++slot) sum += h->h_cnt[((size_t)i * kObSlots + slot) * 2 + k];
      out[3 * i + k] = (int64_t)sum;
    }
  return VDO_OK;
}

}  // namespace vdo

using namespace vdo;

extern "C" int vdo_objects_create(vdo_ctx* ctx, int width, int height, const vdo_objects_params* p, vdo_objects** out) {
  static const char* who = "vdo_objects_create";
  if (!ctx) return set_error(VDO_ERR_INVALID, "%s: ctx is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (!p) return set_error(VDO_ERR_INVALID, "%s: params is null", who);
  if (width < 1) return set_error(VDO_ERR_INVALID, "%s: width %d < 1", who, width);
  if (height < 1) return set_error(VDO_ERR_INVALID, "%s: height %d < 1", who, height);
  int rc = check_intrinsics(who, "K", p->K);
  if (rc == VDO_OK) rc = check_depth_range(who, p->min_depth, p->max_depth);
  if (rc != VDO_OK) return rc;
  if (p->max_labels < 1 || p->max_labels > 1023) return set_error(VDO_ERR_INVALID, "%s: max_labels %d outside 1..1023", who, p->max_labels);
  if (p->max_batch < 1 || p->max_batch > 64) return set_error(VDO_ERR_INVALID, "%s: max_batch %d outside 1..64", who, p->max_batch);
  rc = check_image_size(who, "width x height =", width, height);
  if (rc != VDO_OK) return rc;
  {
    const double mx = (double)width + std::fabs((double)p->K[2]), my = (double)height + std::fabs((double)p->K[3]), m = mx > my ? mx : my;
    const double f = (double)(p->K[0] < p->K[1] ? p->K[0] : p->K[1]), r = m / f > 1.0 ? m / f : 1.0;
    const double term = r * (double)p->max_depth * 1024.0 + 1.0;
    if (!((double)width * (double)height * term <= 4611686018427387904.0))
      return set_error(VDO_ERR_UNSUPPORTED, "%s: width * height * (max((w + |cx|, h + |cy|) / min(fx, fy), 1) * max_depth * 1024 + 1) = %g exceeds 2^62: a sum could leave int64", who,
                       (double)width * (double)height * term);
  }
  rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  vdo_objects* h = new vdo_objects;
  h->ctx = ctx; h->W = width; h->H = height; h->p = *p; h->rows = p->max_labels + 1;
  h->sa = ObStatArgs{p->K[0], p->K[1], p->K[2], p->K[3], p->min_depth, p->max_depth, p->max_labels};
  const size_t npix = (size_t)width * height, sb = (size_t)h->rows * kObRow * sizeof(long long), tb = (size_t)p->max_batch * sizeof(ObEntry),
               cb = (size_t)p->max_batch * kObSlots * 2 * sizeof(unsigned long long);
  const bool ok = hipMalloc((void**)&h->d_depth, npix * sizeof(float)) == hipSuccess && hipMalloc((void**)&h->d_mask, npix * sizeof(int32_t)) == hipSuccess &&
                  hipMalloc((void**)&h->d_stats, sb) == hipSuccess && hipMalloc((void**)&h->d_tab, tb) == hipSuccess && hipMalloc((void**)&h->d_cnt, cb) == hipSuccess &&
                  hipHostMalloc((void**)&h->h_stats, sb, hipHostMallocDefault) == hipSuccess && hipHostMalloc((void**)&h->h_tab, tb, hipHostMallocDefault) == hipSuccess &&
                  hipHostMalloc((void**)&h->h_cnt, cb, hipHostMallocDefault) == hipSuccess && h->tm.create();
  if (!ok) {
    (void)hipGetLastError();
    ob_free(h);
    return set_error(VDO_ERR_OOM, "%s: device allocation failed for %d x %d images, %d labels and %d objects", who, width, height, p->max_labels, p->max_batch);
  }
  *out = h;
  return VDO_OK;
}

extern "C" int vdo_objects_destroy(vdo_objects* h) {
  if (!h) return VDO_OK;
  if (ctx_bind(h->ctx) == VDO_OK) hipStreamSynchronize(h->ctx->stream);
  ob_free(h);
  return VDO_OK;
}

extern "C" int vdo_objects_stats(vdo_objects* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device, int64_t* stats) {
  static const char* who = "vdo_objects_stats";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  int rc = check_depth_mask(who, h->W, depth, depth_stride_floats, mask, mask_stride_ints, true);
  if (rc != VDO_OK) return rc;
  rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const auto t0 = h->tm.begin(s);
  const float* d_depth = stage_rows(s, h->d_depth, depth, depth_stride_floats, h->W, h->H, src_is_device);
  const int32_t* d_mask = stage_rows(s, h->d_mask, mask, mask_stride_ints, h->W, h->H, src_is_device);
  rc = ob_stats(who, h, d_depth, d_mask);
  if (rc != VDO_OK) return rc;
  ob_finish(h, t0, stats);
  return VDO_OK;
}

extern "C" int vdo_objects_stats_frame(vdo_objects* h, const vdo_frame_images* f, int64_t* stats) {
  static const char* who = "vdo_objects_stats_frame";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  int rc = check_frame(who, f, h->W, h->H, "the stage's");
  if (rc != VDO_OK) return rc;
  rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  const auto t0 = h->tm.begin(h->ctx->stream);
  rc = ob_stats(who, h, f->d_depth, f->d_mask);
  if (rc != VDO_OK) return rc;
  ob_finish(h, t0, stats);
  return VDO_OK;
}

extern "C" int vdo_objects_integrate(vdo_objects* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device, int n,
                                     vdo_dense* const* maps, const int32_t* labels, const float* T, int64_t* out) {
  static const char* who = "vdo_objects_integrate";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  int rc = check_depth_mask(who, h->W, depth, depth_stride_floats, mask, mask_stride_ints, true);
  if (rc != VDO_OK) return rc;
  rc = ob_check_batch(who, h, n, maps, labels, T, out);
  if (rc != VDO_OK) return rc;
  rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const auto t0 = h->tm.begin(s);
  const float* d_depth = stage_rows(s, h->d_depth, depth, depth_stride_floats, h->W, h->H, src_is_device);
  const int32_t* d_mask = stage_rows(s, h->d_mask, mask, mask_stride_ints, h->W, h->H, src_is_device);
  rc = ob_stats(who, h, d_depth, d_mask);
  if (rc == VDO_OK) rc = ob_fuse(who, h, d_depth, d_mask, n, maps, labels, T, out);
  if (rc != VDO_OK) return rc;
  ob_finish(h, t0, nullptr);
  return VDO_OK;
}

extern "C" int vdo_objects_integrate_frame(vdo_objects* h, const vdo_frame_images* f, int n, vdo_dense* const* maps, const int32_t* labels, const float* T, int64_t* out) {
  static const char* who = "vdo_objects_integrate_frame";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  int rc = check_frame(who, f, h->W, h->H, "the stage's");
  if (rc != VDO_OK) return rc;
  rc = ob_check_batch(who, h, n, maps, labels, T, out);
  if (rc != VDO_OK) return rc;
  rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  const auto t0 = h->tm.begin(h->ctx->stream);
  rc = ob_stats(who, h, f->d_depth, f->d_mask);
  if (rc == VDO_OK) rc = ob_fuse(who, h, f->d_depth, f->d_mask, n, maps, labels, T, out);
  if (rc != VDO_OK) return rc;
  ob_finish(h, t0, nullptr);
  return VDO_OK;
}

extern "C" int vdo_objects_set_cull(vdo_objects* h, int on) {
  if (!h) return set_error(VDO_ERR_INVALID, "vdo_objects_set_cull: handle is null");
  if (on != 0 && on != 1) return set_error(VDO_ERR_INVALID, "vdo_objects_set_cull: on %d not 0 or 1", on);
  h->cull = on;
  return VDO_OK;
}

extern "C" int vdo_objects_last_stats(vdo_objects* h, int64_t* stats) {
  if (!h || !stats) return set_error(VDO_ERR_INVALID, "vdo_objects_last_stats: %s is null", !h ? "handle" : "stats");
  if (!h->have_stats) return set_error(VDO_ERR_INVALID, "vdo_objects_last_stats: no stats or integrate call was made yet");
  std::memcpy(stats, h->h_stats, (size_t)h->rows * vdo::kObRow * sizeof(long long));
  return VDO_OK;
}

extern "C" int vdo_objects_last_timing(vdo_objects* h, double ms[2]) {
  return last_timing("vdo_objects_last_timing", h ? &h->tm : nullptr, ms);
}
