// Dense mapper: a truncated-signed-distance (TSDF) voxel volume of the static scene on the device - world-aligned, cyclically addressed, following the
// camera - fused projectively from a frame's metric depth, its instance mask (non-zero pixels are left out) and its camera pose; surface points are
// extracted from it in a fixed order.  The reference keeps no dense map; the semantics are this library's own, stated in include/vdo_slam_hip.h
// (vdo_dense_integrate) and restated in NumPy by tests/dense_ref.py.  The geometry is fp32 with one rounded operation per step (the library is built
// with -ffp-contract=off; / and floorf are correctly rounded), the fusion and everything after it is integer: no result depends on workgroup shape,
// on the voxels a thread takes or on the schedule.
//
//   k_dn_integrate<VPT>  x on the lanes (one wave = 64 consecutive slots of a row: the 4-byte words are read and written coalesced), 4 z per workgroup,
//                        VPT consecutive y per thread: T0 * px, T2 * pz + T3, K and the thresholds stay in registers, the VPT words are loaded before
//                        the first is used.  Every voxel is computed from its own integer index.  A word is written only when it changed.  The three
//                        counts by wave ballot, summed over the workgroup in LDS, one 64-bit integer atomic per workgroup and counter on one of
//                        1024 copies of the counters, which the host adds up.
//   k_dn_clear           recenter: the slots of ONE leaving slab (a cyclic range on one axis, everything on the other two) are set to 0.
//   k_dn_extract<FILL>   one thread per voxel of the box (x fastest), up to three points each: count per workgroup, k_counts_scan of scan.hpp (one workgroup, 64-bit
//                        carry), then the same kernel writes the points of a window [base, base + cap) of the visiting order.
//
// NO OUT-OF-RANGE ACCESS: the one gathered address comes from float compares against 0 and W - 1 / H - 1 made before any conversion to int (a NaN
// fails them); every volume index is built from slot coordinates tested against n; an extracted point is written only inside its window.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>
#include <cstring>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"
#include "frame_images.hpp"
#include "stage.hpp"
#include "dense.hpp"
#include "scan.hpp"

namespace vdo {

template <int VPT>
__global__ __launch_bounds__(256) void k_dn_integrate(DnArgs a, const float* __restrict__ depth, const int32_t* __restrict__ mask, int W, int H, uint32_t* __restrict__ vol,
                                                      unsigned long long* __restrict__ cnt) {
  const int nx = a.n[0], ny = a.n[1], nz = a.n[2];
  const int sx = blockIdx.x * 64 + threadIdx.x, sz = blockIdx.z * kDnZ + threadIdx.z, sy0 = blockIdx.y * VPT;
  const bool in_xz = sx < nx && sz < nz;
  float ax = 0.f, ay = 0.f, az = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
  if (in_xz) {
    const float px = ((float)dn_global(sx, a.o[0], a.om[0], nx) + 0.5f) * a.voxel, pz = ((float)dn_global(sz, a.o[2], a.om[2], nz) + 0.5f) * a.voxel;
    ax = a.T[0] * px; ay = a.T[4] * px; az = a.T[8] * px;
    bx = a.T[2] * pz + a.T[3]; by = a.T[6] * pz + a.T[7]; bz = a.T[10] * pz + a.T[11];
  }
  const size_t row0 = ((size_t)(in_xz ? sz : 0) * ny) * nx + (in_xz ? sx : 0);
  uint32_t word[VPT];
#pragma unroll
  for (int k = 0; k < VPT; ++k) word[k] = (in_xz && sy0 + k < ny) ? vol[row0 + (size_t)(sy0 + k) * nx] : 0u;
  int n_upd = 0, n_msk = 0, n_occ = 0;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int sy = sy0 + k;
    bool upd = false, msk = false, occ = false;
    if (in_xz && sy < ny) {
      const float py = ((float)dn_global(sy, a.o[1], a.om[1], ny) + 0.5f) * a.voxel;
      const float Xc = (ax + a.T[1] * py) + bx, Yc = (ay + a.T[5] * py) + by, Zc = (az + a.T[9] * py) + bz;
      float xq, yq;
      if (dn_pixel(a, Xc, Yc, Zc, W, H, &xq, &yq)) {
        const int j = (int)yq * W + (int)xq;
        const float d = depth[j];
        if (dn_depth_ok(a, d)) {
          uint32_t nw;
          if (mask && mask[j] != 0) {
            msk = true;
          } else if (!dn_fuse(a, d, Zc, word[k], &nw)) {
            occ = true;
          } else {
            if (nw != word[k]) vol[row0 + (size_t)sy * nx] = nw;
            upd = true;
          }
        }
      }
    }
    n_upd += (int)__popcll(__ballot(upd)); n_msk += (int)__popcll(__ballot(msk)); n_occ += (int)__popcll(__ballot(occ));
  }
  // the four waves' counts through LDS (blockDim.x == 64: one wave per threadIdx.z), then at most three atomics per workgroup, on one of kDnSlots
  // copies of the counters: with one copy and one atomic per wave the kernel took the time of its atomics, not of its voxels
  __shared__ int red[kDnZ][3];
  if (threadIdx.x == 0) { red[threadIdx.z][0] = n_upd; red[threadIdx.z][1] = n_msk; red[threadIdx.z][2] = n_occ; }
  __syncthreads();
  if (threadIdx.x < 3 && threadIdx.z == 0) {
    int sum = 0;
    for (int z = 0; z < kDnZ; ++z) sum += red[z][threadIdx.x];
    const unsigned slot = (blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) & (unsigned)(kDnSlots - 1);
    if (sum) atomicAdd(cnt + slot * kDnCounters + threadIdx.x, (unsigned long long)sum);
  }
}

// the slab of `len` slots from slot s0 on (cyclic) on `axis`, whole on the other two axes
__global__ __launch_bounds__(256) void k_dn_clear(uint32_t* __restrict__ vol, int nx, int ny, int nz, int axis, int s0, int len) {
  const int lx = axis == 0 ? len : nx, ly = axis == 1 ? len : ny, lz = axis == 2 ? len : nz;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)lx * ly * lz) return;
  int x = (int)(i % lx), y = (int)((i / lx) % ly), z = (int)(i / ((long long)lx * ly));
  if (axis == 0) x = dn_slot(x, s0, nx);
  if (axis == 1) y = dn_slot(y, s0, ny);
  if (axis == 2) z = dn_slot(z, s0, nz);
  vol[((size_t)z * ny + y) * nx + x] = 0u;
}

// Voxel i of the box in the visiting order (x fastest): its points on axes 0, 1, 2.  !FILL: the workgroup's number of points.  FILL: the points
// whose place in the visiting order lies in [base, base + cap) are written at place - base.
template <bool FILL>
__global__ __launch_bounds__(256) void k_dn_extract(DnArgs a, DnBox bx, long long nbox, int min_w, const uint32_t* __restrict__ vol, long long* __restrict__ blk, long long base,
                                                    long long cap, float* __restrict__ xyz, int32_t* __restrict__ grad, int32_t* __restrict__ wgt) {
  __shared__ int lds[17];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  int cross = 0, g[3] = {0, 0, 0}, ta = 0, wa = 0, tb[3] = {0, 0, 0}, wb[3] = {0, 0, 0};
  bool all_in = false;
  if (i < nbox) {
    g[0] = bx.lo[0] + (int)(i % bx.b[0]); g[1] = bx.lo[1] + (int)((i / bx.b[0]) % bx.b[1]); g[2] = bx.lo[2] + (int)(i / ((long long)bx.b[0] * bx.b[1]));
    int s[3];
    for (int k = 0; k < 3; ++k) { s[k] = g[k] % a.n[k]; if (s[k] < 0) s[k] += a.n[k]; }
    const uint32_t w0 = vol[((size_t)s[2] * a.n[1] + s[1]) * a.n[0] + s[0]];
    ta = (int)(int16_t)(w0 & 0xffffu); wa = dn_weight(w0);                   // dn_tsdf, spelled out here and for tb: the call changes the kernel's instructions
    all_in = true;
    for (int k = 0; k < 3; ++k) {
      const bool inside = g[k] + 1 < a.o[k] + a.n[k];
      if (inside) {
        int t[3] = {s[0], s[1], s[2]};
        t[k] = dn_next(s[k], a.n[k]);
        const uint32_t w1 = vol[((size_t)t[2] * a.n[1] + t[1]) * a.n[0] + t[0]];
        tb[k] = (int)(int16_t)(w1 & 0xffffu); wb[k] = dn_weight(w1);
      }
      const bool usable = inside && wb[k] >= min_w;
      all_in = all_in && usable;
      if (usable && wa >= min_w && ((ta < 0) != (tb[k] < 0))) cross |= 1 << k;
    }
  }
  int total;
  const int ex = block_excl_scan(__popc(cross), lds, &total);
  if (!FILL) {
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
    return;
  }
  long long pos = blk[blockIdx.x] + ex;
  for (int k = 0; k < 3; ++k) {
    if (!(cross >> k & 1)) continue;
    if (pos >= base && pos < base + cap) {
      const long long r = pos - base;
      const float frac = (float)ta / (float)(ta - tb[k]);
      for (int c = 0; c < 3; ++c) {
        const float centre = (float)g[c] + 0.5f;
        xyz[3 * r + c] = (c == k ? centre + frac : centre) * a.voxel;
        grad[3 * r + c] = all_in ? tb[c] - ta : 0;
      }
      wgt[r] = wa < wb[k] ? wa : wb[k];
    }
    ++pos;
  }
}

static void dn_free(vdo_dense* h) {
  hipFree(h->d_vol); hipFree(h->d_depth); hipFree(h->d_mask); hipFree(h->d_blk); hipFree(h->d_xyz); hipFree(h->d_grad); hipFree(h->d_wgt);
  h->cnt.destroy();
  h->tm.destroy();
  delete h;
}

void dn_queue_move(hipStream_t s, uint32_t* words, const int n[3], int64_t nvox, const int from[3], const int to[3]) {
  const DnMove m = dn_move(n, from, to);
  if (m.all) hipMemsetAsync(words, 0, (size_t)nvox * sizeof(uint32_t), s);
  for (int i = 0; i < m.slabs; ++i) {
    const long long cells = (long long)m.slab[i].len * (nvox / n[m.slab[i].axis]);
    hipLaunchKernelGGL(k_dn_clear, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, words, n[0], n[1], n[2], m.slab[i].axis, m.slab[i].s0, m.slab[i].len);
  }
}

// an origin whose volume stays inside (-2^22, 2^22) on every axis; 0 when it does
static int dn_check_origin(const char* who, const char* name, const int32_t o[3], const int32_t n[3]) {
  for (int k = 0; k < 3; ++k)
    if (o[k] <= -kDnMaxOrigin || (int64_t)o[k] + n[k] > kDnMaxOrigin)
      return set_error(VDO_ERR_INVALID, "%s: %s[%d] = %d: the volume must stay inside (-2^22, 2^22) voxels", who, name, k, o[k]);
  return VDO_OK;
}

static void dn_set_origin(vdo_dense* h, const int32_t o[3]) {
  for (int k = 0; k < 3; ++k) { h->p.origin[k] = o[k]; h->a.o[k] = o[k]; h->a.om[k] = dn_mod(o[k], h->a.n[k]); }
}

template <int VPT>
static void dn_launch_integrate(vdo_dense* h, hipStream_t s, const DnArgs& a, const float* depth, const int32_t* mask) {
  const dim3 grid((a.n[0] + 63) / 64, (a.n[1] + VPT - 1) / VPT, (a.n[2] + kDnZ - 1) / kDnZ);
  hipLaunchKernelGGL(k_dn_integrate<VPT>, grid, dim3(64, 1, kDnZ), 0, s, a, depth, mask, h->W, h->H, h->d_vol, h->cnt.d);
}

// the launch, the download of the counts and the timing the two integrate entries share; depth and mask are packed device images
static int dn_integrate(const char* who, vdo_dense* h, const float* d_depth, const int32_t* d_mask, const float T[16], int64_t out[3], StageClock::time_point t0) {
  hipStream_t s = h->ctx->stream;
  DnArgs a = h->a;
  for (int k = 0; k < 12; ++k) a.T[k] = T[k];
  h->cnt.zero(s);
  switch (h->vpt) {
    case 1: dn_launch_integrate<1>(h, s, a, d_depth, d_mask); break;
    case 2: dn_launch_integrate<2>(h, s, a, d_depth, d_mask); break;
    case 8: dn_launch_integrate<8>(h, s, a, d_depth, d_mask); break;
    default: dn_launch_integrate<4>(h, s, a, d_depth, d_mask); break;
  }
  h->tm.mark_end(s);
  h->cnt.download(s);
  const int rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  for (int k = 0; k < 3; ++k) out[k] = h->cnt.sum(k);
  h->tm.finish(t0);
  return VDO_OK;
}

}  // namespace vdo

using namespace vdo;

extern "C" int vdo_dense_create(vdo_ctx* ctx, int width, int height, const vdo_dense_params* p, vdo_dense** out) {
  static const char* who = "vdo_dense_create";
  if (!ctx) return set_error(VDO_ERR_INVALID, "%s: ctx is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (!p) return set_error(VDO_ERR_INVALID, "%s: params is null", who);
  if (width < 1) return set_error(VDO_ERR_INVALID, "%s: width %d < 1", who, width);
  if (height < 1) return set_error(VDO_ERR_INVALID, "%s: height %d < 1", who, height);
  int rc = dn_check_sides(who, p->n);
  if (rc != VDO_OK) return rc;
  if (!is_finite(p->voxel) || !(p->voxel > 0.f)) return set_error(VDO_ERR_INVALID, "%s: voxel %g must be positive and finite", who, (double)p->voxel);
  rc = check_intrinsics(who, "K", p->K);
  if (rc != VDO_OK) return rc;
  if (!is_finite(p->trunc) || !(p->trunc > 0.f)) return set_error(VDO_ERR_INVALID, "%s: trunc %g must be positive and finite", who, (double)p->trunc);
  rc = check_depth_range(who, p->min_depth, p->max_depth);
  if (rc != VDO_OK) return rc;
  if (p->max_weight < 1 || p->max_weight > 255) return set_error(VDO_ERR_INVALID, "%s: max_weight %d outside 1..255", who, p->max_weight);
  if (p->stage_points < 1) return set_error(VDO_ERR_INVALID, "%s: stage_points %d < 1", who, p->stage_points);
  int64_t nvox;
  rc = dn_check_size(who, p->n, &nvox);
  if (rc == VDO_OK) rc = check_image_size(who, "width x height =", width, height);
  if (rc != VDO_OK) return rc;
  rc = dn_check_origin(who, "origin", p->origin, p->n);
  if (rc != VDO_OK) return rc;
  rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  vdo_dense* h = new vdo_dense;
  h->ctx = ctx; h->W = width; h->H = height; h->p = *p; h->nvox = nvox; h->stage_points = p->stage_points;
  DnArgs& a = h->a;
  a.fx = p->K[0]; a.fy = p->K[1]; a.cx = p->K[2]; a.cy = p->K[3]; a.trunc = p->trunc; a.min_d = p->min_depth; a.max_d = p->max_depth; a.voxel = p->voxel;
  a.min_z = p->min_depth > FLT_MIN ? p->min_depth : FLT_MIN;
  a.max_w = p->max_weight;
  for (int k = 0; k < 3; ++k) a.n[k] = p->n[k];
  dn_set_origin(h, p->origin);
  const size_t npix = (size_t)width * height, nblk = (size_t)((nvox + 255) / 256), sp = (size_t)p->stage_points;
  const bool ok = hipMalloc((void**)&h->d_vol, (size_t)nvox * sizeof(uint32_t)) == hipSuccess && hipMalloc((void**)&h->d_depth, npix * sizeof(float)) == hipSuccess &&
                  hipMalloc((void**)&h->d_mask, npix * sizeof(int32_t)) == hipSuccess && hipMalloc((void**)&h->d_blk, nblk * sizeof(long long)) == hipSuccess &&
                  h->cnt.create(kDnSlots, kDnCounters) && hipMalloc((void**)&h->d_xyz, sp * 3 * sizeof(float)) == hipSuccess &&
                  hipMalloc((void**)&h->d_grad, sp * 3 * sizeof(int32_t)) == hipSuccess && hipMalloc((void**)&h->d_wgt, sp * sizeof(int32_t)) == hipSuccess && h->tm.create() &&
                  hipMemsetAsync(h->d_vol, 0, (size_t)nvox * sizeof(uint32_t), ctx->stream) == hipSuccess &&
                  hipStreamSynchronize(ctx->stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    dn_free(h);
    return set_error(VDO_ERR_OOM, "%s: device allocation failed for %d x %d x %d voxels and %d x %d images", who, p->n[0], p->n[1], p->n[2], width, height);
  }
  *out = h;
  return VDO_OK;
}

extern "C" int vdo_dense_destroy(vdo_dense* h) {
  if (!h) return VDO_OK;
  if (ctx_bind(h->ctx) == VDO_OK) hipStreamSynchronize(h->ctx->stream);
  dn_free(h);
  return VDO_OK;
}

extern "C" int vdo_dense_set_voxels_per_thread(vdo_dense* h, int voxels) {
  if (!h) return set_error(VDO_ERR_INVALID, "vdo_dense_set_voxels_per_thread: handle is null");
  if (voxels != 1 && voxels != 2 && voxels != 4 && voxels != 8) return set_error(VDO_ERR_INVALID, "vdo_dense_set_voxels_per_thread: voxels %d not 1, 2, 4 or 8", voxels);
  h->vpt = voxels;
  return VDO_OK;
}

extern "C" int vdo_dense_integrate(vdo_dense* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device, const float T[16],
                                   int64_t out[3]) {
  static const char* who = "vdo_dense_integrate";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  int rc = check_depth_mask(who, h->W, depth, depth_stride_floats, mask, mask_stride_ints, false);
  if (rc != VDO_OK) return rc;
  if (!T) return set_error(VDO_ERR_INVALID, "%s: T is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const auto t0 = h->tm.begin(s);
  const float* d_depth = stage_rows(s, h->d_depth, depth, depth_stride_floats, h->W, h->H, src_is_device);
  const int32_t* d_mask = mask ? stage_rows(s, h->d_mask, mask, mask_stride_ints, h->W, h->H, src_is_device) : nullptr;
  return dn_integrate(who, h, d_depth, d_mask, T, out, t0);
}

extern "C" int vdo_dense_integrate_frame(vdo_dense* h, const vdo_frame_images* f, const float T[16], int64_t out[3]) {
  static const char* who = "vdo_dense_integrate_frame";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  int rc = check_frame(who, f, h->W, h->H, "the mapper's");
  if (rc != VDO_OK) return rc;
  if (!T) return set_error(VDO_ERR_INVALID, "%s: T is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  const auto t0 = h->tm.begin(h->ctx->stream);
  return dn_integrate(who, h, f->d_depth, f->d_mask, T, out, t0);
}

extern "C" int vdo_dense_recenter(vdo_dense* h, const int32_t new_origin[3]) {
  static const char* who = "vdo_dense_recenter";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!new_origin) return set_error(VDO_ERR_INVALID, "%s: new_origin is null", who);
  int rc = dn_check_origin(who, "new_origin", new_origin, h->p.n);
  if (rc != VDO_OK) return rc;
  rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const auto t0 = h->tm.begin(s);
  dn_queue_move(s, h->d_vol, h->a.n, h->nvox, h->a.o, new_origin);
  h->tm.mark_end(s);
  rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  dn_set_origin(h, new_origin);
  h->tm.finish(t0);
  return VDO_OK;
}

extern "C" int vdo_dense_extract(vdo_dense* h, const int32_t lo[3], const int32_t hi[3], int min_weight, int64_t capacity, float* xyz, int32_t* grad, int32_t* weight, int out_is_device,
                                 int64_t* count) {
  static const char* who = "vdo_dense_extract";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!lo) return set_error(VDO_ERR_INVALID, "%s: lo is null", who);
  if (!hi) return set_error(VDO_ERR_INVALID, "%s: hi is null", who);
  if (min_weight < 1) return set_error(VDO_ERR_INVALID, "%s: min_weight %d < 1", who, min_weight);
  if (capacity < 0) return set_error(VDO_ERR_INVALID, "%s: capacity %lld < 0", who, (long long)capacity);
  if (capacity > 0 && !xyz) return set_error(VDO_ERR_INVALID, "%s: xyz is null", who);
  if (capacity > 0 && !grad) return set_error(VDO_ERR_INVALID, "%s: grad is null", who);
  if (capacity > 0 && !weight) return set_error(VDO_ERR_INVALID, "%s: weight is null", who);
  if (!count) return set_error(VDO_ERR_INVALID, "%s: count is null", who);
  int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const DnClip clip = dn_clip(h, lo, hi);
  const DnBox& bx = clip.box;
  const long long nbox = clip.voxels();
  unsigned long long* d_total = h->cnt.d + h->cnt.words();                    // the spare word
  const auto t0 = h->tm.begin(s);
  long long total = 0;
  if (nbox > 0) {
    const long long nblk = (nbox + 255) / 256;
    hipLaunchKernelGGL(k_dn_extract<false>, dim3((unsigned)nblk), dim3(256), 0, s, h->a, bx, nbox, min_weight, (const uint32_t*)h->d_vol, h->d_blk, 0LL, 0LL, (float*)nullptr,
                       (int32_t*)nullptr, (int32_t*)nullptr);
    hipLaunchKernelGGL(k_counts_scan<1024>, dim3(1), dim3(1024), 0, s, h->d_blk, nblk, d_total);
    hipMemcpyAsync(h->cnt.h + h->cnt.words(), d_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
    rc = sync_check(who, s);
    if (rc != VDO_OK) return rc;
    total = (long long)h->cnt.h[h->cnt.words()];
    const long long want = total < capacity ? total : capacity;
    // a device output is one window; a host output goes through the staging lists, stage_points at a time
    for (long long base = 0; base < want; base += out_is_device ? want : h->stage_points) {
      const long long cap = out_is_device ? want : (want - base < h->stage_points ? want - base : h->stage_points);
      float* o_xyz = out_is_device ? xyz : h->d_xyz; int32_t* o_grad = out_is_device ? grad : h->d_grad; int32_t* o_wgt = out_is_device ? weight : h->d_wgt;
      hipLaunchKernelGGL(k_dn_extract<true>, dim3((unsigned)nblk), dim3(256), 0, s, h->a, bx, nbox, min_weight, (const uint32_t*)h->d_vol, h->d_blk, base, cap, o_xyz, o_grad, o_wgt);
      if (!out_is_device) {
        hipMemcpyAsync(xyz + 3 * base, h->d_xyz, (size_t)cap * 3 * sizeof(float), hipMemcpyDeviceToHost, s);
        hipMemcpyAsync(grad + 3 * base, h->d_grad, (size_t)cap * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s);
        hipMemcpyAsync(weight + base, h->d_wgt, (size_t)cap * sizeof(int32_t), hipMemcpyDeviceToHost, s);
        rc = check_hip(who, hipStreamSynchronize(s));                        // the staging lists are free for the next window
        if (rc != VDO_OK) return rc;
      }
    }
  }
  h->tm.mark_end(s);
  rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  *count = total;
  h->tm.finish(t0);
  return VDO_OK;
}

extern "C" int vdo_dense_get_volume(vdo_dense* h, uint32_t* words, int32_t origin[3]) {
  static const char* who = "vdo_dense_get_volume";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!words && !origin) return set_error(VDO_ERR_INVALID, "%s: words and origin are both null", who);
  if (words) {
    const int rc = ctx_bind(h->ctx);
    if (rc != VDO_OK) return rc;
    hipMemcpyAsync(words, h->d_vol, (size_t)h->nvox * sizeof(uint32_t), hipMemcpyDeviceToHost, h->ctx->stream);
    const int rs = check_hip(who, hipStreamSynchronize(h->ctx->stream));
    if (rs != VDO_OK) return rs;
  }
  if (origin) for (int k = 0; k < 3; ++k) origin[k] = h->a.o[k];
  return VDO_OK;
}

extern "C" int vdo_dense_set_volume(vdo_dense* h, const uint32_t* words) {
  static const char* who = "vdo_dense_set_volume";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!words) return set_error(VDO_ERR_INVALID, "%s: words is null", who);
  const int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipMemcpyAsync(h->d_vol, words, (size_t)h->nvox * sizeof(uint32_t), hipMemcpyHostToDevice, h->ctx->stream);
  return check_hip(who, hipStreamSynchronize(h->ctx->stream));
}

extern "C" int vdo_dense_clear(vdo_dense* h) {
  static const char* who = "vdo_dense_clear";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  const int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipMemsetAsync(h->d_vol, 0, (size_t)h->nvox * sizeof(uint32_t), h->ctx->stream);
  return check_hip(who, hipStreamSynchronize(h->ctx->stream));
}

extern "C" int vdo_dense_last_timing(vdo_dense* h, double ms[2]) {
  return last_timing("vdo_dense_last_timing", h ? &h->tm : nullptr, ms);
}

extern "C" int vdo_dense_device_volume(vdo_dense* h, uint32_t** words) {
  if (!h || !words) return set_error(VDO_ERR_INVALID, "vdo_dense_device_volume: %s is null", !h ? "handle" : "words");
  *words = h->d_vol;
  return VDO_OK;
}
