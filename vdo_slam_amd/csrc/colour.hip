// Colourer: a colour per voxel beside a dense mapper's TSDF volume (dense.hip) - fused per frame from the image the frame's depth belongs to, read
// back at world points and along a depth image.  The semantics are this library's own, stated in include/vdo_slam_hip.h ("Colourer") and restated in
// NumPy by tests/colour_ref.py.  The geometry is fp32 with one rounded operation per step (the library is built with -ffp-contract=off; / and floorf
// are correctly rounded), everything after it is integer: no result depends on workgroup shape, on the voxels a thread takes or on the schedule.
//
//   k_cl_pack            one thread per pixel: 1, 3 or 4 bytes -> one word R | G << 8 | B << 16, so that the fusion reads one word per tap.
//   k_cl_integrate<VPT>  the launch shape and the projection of k_dn_integrate (x on the lanes: the words of a row are coalesced; 4 z per workgroup; VPT
//                        consecutive y per thread; dn_pixel and dn_depth_ok, so that the pixel is the same bit for bit).  Few voxels pass the band
//                        test - a shell of 2 * band around the surfaces against the whole frustum -, so the colour word is NOT loaded up front as
//                        k_dn_integrate loads its TSDF word: only a voxel that reaches the running mean reads it, and writes it only when it changed.
//                        The three counts as there: wave ballots, LDS, one 64-bit integer atomic per workgroup and counter on one of 1024 copies.
//   (follow)             dense.hip's dn_queue_move on the colour words: the mapper's own rule and its k_dn_clear.
//   k_cl_sample          one thread per point: up to eight gathered words, integer trilinear weights.
//   k_cl_render          one thread per pixel of a window of a depth image: the raycaster's point, then the same sample.
//
// NO OUT-OF-RANGE ACCESS: the gathered pixel comes from float compares against 0 and W - 1 / H - 1 made before any conversion to int (a NaN fails
// them); a sample's base cell is converted to int only after dn_indexable, and a corner is turned into slots only after its integer
// tests against o and o + n; a point or pixel is read and written only inside its window.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"
#include "frame_images.hpp"
#include "stage.hpp"
#include "dense.hpp"

namespace vdo {

enum { kClUpdated = 0, kClLabel, kClBand };                                // the counters of k_cl_integrate, kept as k_dn_integrate keeps its own
constexpr long long kClMaxWindow = 1LL << 30;                              // points per launch of k_cl_sample on a device output

struct ClFuse { float band; int max_w, label; };

// what a sample needs of the map
struct ClVol { float voxel; int n[3], o[3], om[3]; };

// the render's view: intrinsics, the camera centre, R[3 * i + a] = T(i, a), the image width
struct ClView { float fx, fy, cx, cy, c[3], R[9]; int W; };

__global__ __launch_bounds__(256) void k_cl_pack(const uint8_t* __restrict__ src, long long stride, int channels, int bgr, int W, int H, uint32_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W * H) return;
  const int x = i % W, y = i / W;
  const uint8_t* p = src + (size_t)y * (size_t)stride + (size_t)x * channels;
  uint32_t r, g, b;
  if (channels == 1) {
    r = g = b = p[0];
  } else {
    r = p[bgr ? 2 : 0]; g = p[1]; b = p[bgr ? 0 : 2];
  }
  out[i] = r | (g << 8) | (b << 16);
}

// the word after one more observation q (packed R, G, B) of a voxel
__device__ __forceinline__ uint32_t cl_mean(uint32_t word, uint32_t q, int max_w) {
  const int cw = (int)(word >> 24), w1 = cw + 1 < max_w ? cw + 1 : max_w;
  uint32_t nw = (uint32_t)w1 << 24;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int old = (int)((word >> (8 * c)) & 0xffu), obs = (int)((q >> (8 * c)) & 0xffu);
    nw |= (uint32_t)((2 * (old * cw + obs) + (cw + 1)) / (2 * (cw + 1))) << (8 * c);      // at most 255: the rounded mean of values <= 255
  }
  return nw;
}

template <int VPT>
__global__ __launch_bounds__(256) void k_cl_integrate(DnArgs a, ClFuse cf, const float* __restrict__ depth, const int32_t* __restrict__ mask, const uint32_t* __restrict__ img, int W,
                                                      int H, uint32_t* __restrict__ col, unsigned long long* __restrict__ cnt) {
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
  int n_upd = 0, n_lab = 0, n_band = 0;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int sy = sy0 + k;
    bool upd = false, lab = false, out_band = false;
    if (in_xz && sy < ny) {
      const float py = ((float)dn_global(sy, a.o[1], a.om[1], ny) + 0.5f) * a.voxel;
      const float Xc = (ax + a.T[1] * py) + bx, Yc = (ay + a.T[5] * py) + by, Zc = (az + a.T[9] * py) + bz;
      float xq, yq;
      if (dn_pixel(a, Xc, Yc, Zc, W, H, &xq, &yq)) {
        const int j = (int)yq * W + (int)xq;
        const float d = depth[j];
        if (dn_depth_ok(a, d)) {
          const int m = (mask && cf.label >= 0) ? mask[j] : 0;
          const float s = d - Zc;
          if (cf.label == 0 ? m != 0 : (cf.label > 0 && m != cf.label)) {
            lab = true;
          } else if (!(fabsf(s) <= cf.band)) {
            out_band = true;
          } else {
            uint32_t* p = col + row0 + (size_t)sy * nx;
            const uint32_t word = *p, nw = cl_mean(word, img[j], cf.max_w);
            if (nw != word) *p = nw;
            upd = true;
          }
        }
      }
    }
    n_upd += (int)__popcll(__ballot(upd)); n_lab += (int)__popcll(__ballot(lab)); n_band += (int)__popcll(__ballot(out_band));
  }
  // as k_dn_integrate: the four waves' counts through LDS (blockDim.x == 64: one wave per threadIdx.z), then at most three atomics per workgroup
  __shared__ int red[kDnZ][3];
  if (threadIdx.x == 0) { red[threadIdx.z][kClUpdated] = n_upd; red[threadIdx.z][kClLabel] = n_lab; red[threadIdx.z][kClBand] = n_band; }
  __syncthreads();
  if (threadIdx.x < 3 && threadIdx.z == 0) {
    int sum = 0;
    for (int z = 0; z < kDnZ; ++z) sum += red[z][threadIdx.x];
    const unsigned slot = (blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) & (unsigned)(kDnSlots - 1);
    if (sum) atomicAdd(cnt + slot * kDnCounters + threadIdx.x, (unsigned long long)sum);
  }
}

// the colour of the world point p: R | G << 8 | B << 16 | alpha << 24, 0 when no corner counts
__device__ __forceinline__ uint32_t cl_sample(const ClVol& v, const uint32_t* __restrict__ col, const float p[3], int min_w) {
  int b[3], fi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float u = p[k] / v.voxel;
    u = u - 0.5f;
    const float fl = floorf(u), f = u - fl;
    if (!dn_indexable(p[k], fl)) return 0u;
    b[k] = (int)fl; fi[k] = (int)floorf(f * 256.0f);
  }
  // per axis and offset: the slot, or -1 outside the volume, and the axis weight
  int slot[3][2], aw[3][2];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const int g = b[k] + d;
      int s = -1;
      if (g >= v.o[k] && g < v.o[k] + v.n[k]) s = dn_slot(g - v.o[k], v.om[k], v.n[k]);
      slot[k][d] = s; aw[k][d] = d ? fi[k] : 256 - fi[k];
    }
  long long S = 0, C[3] = {0, 0, 0};
#pragma unroll
  for (int dz = 0; dz < 2; ++dz)
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        if (slot[0][dx] < 0 || slot[1][dy] < 0 || slot[2][dz] < 0) continue;
        const uint32_t w = col[((size_t)slot[2][dz] * v.n[1] + slot[1][dy]) * v.n[0] + slot[0][dx]];
        if ((int)(w >> 24) < min_w) continue;
        const long long wgt = (long long)(aw[0][dx] * aw[1][dy]) * aw[2][dz];
        S += wgt;
#pragma unroll
        for (int c = 0; c < 3; ++c) C[c] += wgt * (long long)((w >> (8 * c)) & 0xffu);
      }
  if (S == 0) return 0u;
  const long long al = (255 * S + (1LL << 23)) >> 24;
  uint32_t out = (uint32_t)(al < 1 ? 1 : al) << 24;
#pragma unroll
  for (int c = 0; c < 3; ++c) out |= (uint32_t)((2 * C[c] + S) / (2 * S)) << (8 * c);
  return out;
}

// the workgroup's count of `flag` added to counter `which` of one of the kDnSlots copies; every thread of the workgroup calls it
__device__ __forceinline__ void cl_count(bool flag, int which, int* red, unsigned long long* __restrict__ cnt) {
  const int n = (int)__popcll(__ballot(flag));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int sum = (red[0] + red[1]) + (red[2] + red[3]);
    if (sum) atomicAdd(cnt + (blockIdx.x & (unsigned)(kDnSlots - 1)) * kDnCounters + which, (unsigned long long)sum);
  }
  __syncthreads();
}

// points [0, n) of a window
__global__ __launch_bounds__(256) void k_cl_sample(ClVol v, const uint32_t* __restrict__ col, long long n, const float* __restrict__ xyz, int min_w, uint32_t* __restrict__ rgba,
                                                   unsigned long long* __restrict__ cnt) {
  __shared__ int red[4];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  uint32_t out = 0u;
  if (i < n) {
    const float p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    out = cl_sample(v, col, p, min_w);
    rgba[i] = out;
  }
  cl_count(out != 0u, 0, red, cnt);
}

// pixels [base, base + n) of the image; depth and rgba point at pixel `base`
__global__ __launch_bounds__(256) void k_cl_render(ClVol v, ClView vw, const uint32_t* __restrict__ col, int base, int n, const float* __restrict__ depth, int min_w,
                                                   uint32_t* __restrict__ rgba, unsigned long long* __restrict__ cnt) {
  __shared__ int red[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  uint32_t out = 0u;
  bool has_depth = false;
  if (i < n) {
    const float d = depth[i];
    has_depth = dn_finite(d) && d > 0.f;
    if (has_depth) {
      const int pix = base + i;
      float r[3], p[3];
      dn_ray((float)(pix % vw.W), (float)(pix / vw.W), vw.fx, vw.fy, vw.cx, vw.cy, vw.R, r);
#pragma unroll
      for (int k = 0; k < 3; ++k) p[k] = vw.c[k] + d * r[k];
      out = cl_sample(v, col, p, min_w);
    }
    rgba[i] = out;
  }
  cl_count(out != 0u, 0, red, cnt);
  cl_count(has_depth && out == 0u, 1, red, cnt);
}

}  // namespace vdo

struct vdo_colour {
  vdo_dense* map = nullptr;                               // borrowed
  vdo_colour_params p{};
  int vpt = 4;
  int o[3] = {0, 0, 0};                                   // the map origin the colour volume stands at
  int64_t stage_points = 0;
  uint32_t* d_col = nullptr;                              // [nz][ny][nx] words in slot order
  uint32_t* d_img = nullptr;                              // [H][W] packed R | G << 8 | B << 16
  uint8_t* d_src = nullptr;                               // [H][W * 4] staging of a host image
  vdo::SlotCounts cnt;                                    // [kDnSlots][kDnCounters]
  float* d_xyz = nullptr;                                 // [stage_points][3]: a window of host points, or [stage_points] of a host depth image
  uint32_t* d_rgba = nullptr;                             // [stage_points]
  vdo::StageTimer tm;
};

using namespace vdo;

static void cl_free(vdo_colour* h) {
  hipFree(h->d_col); hipFree(h->d_img); hipFree(h->d_src); hipFree(h->d_xyz); hipFree(h->d_rgba);
  h->cnt.destroy();
  h->tm.destroy();
  delete h;
}

// Queues what brings the colour volume to the map's present origin: nothing when it has not moved
static void cl_follow(vdo_colour* h, hipStream_t s) {
  dn_queue_move(s, h->d_col, h->map->a.n, h->map->nvox, h->o, h->map->a.o);
  for (int k = 0; k < 3; ++k) h->o[k] = h->map->a.o[k];
}

static ClVol cl_vol(const vdo_colour* h) {
  ClVol v;
  v.voxel = h->map->a.voxel;
  for (int k = 0; k < 3; ++k) { v.n[k] = h->map->a.n[k]; v.o[k] = h->map->a.o[k]; v.om[k] = h->map->a.om[k]; }
  return v;
}

static int cl_check_image(const char* who, int W, const uint8_t* image, int64_t stride, int channels, int rgb_order) {
  if (!image) return set_error(VDO_ERR_INVALID, "%s: image is null", who);
  if (channels != 1 && channels != 3 && channels != 4) return set_error(VDO_ERR_INVALID, "%s: channels %d not 1, 3 or 4", who, channels);
  if (rgb_order != 0 && rgb_order != 1) return set_error(VDO_ERR_INVALID, "%s: rgb_order %d not 0 or 1", who, rgb_order);
  if (stride < (int64_t)W * channels) return set_error(VDO_ERR_INVALID, "%s: image_stride_bytes %lld smaller than width * channels = %lld", who, (long long)stride, (long long)W * channels);
  return VDO_OK;
}

template <int VPT>
static void cl_launch_integrate(vdo_colour* h, hipStream_t s, const DnArgs& a, const ClFuse& cf, const float* depth, const int32_t* mask) {
  const dim3 grid((a.n[0] + 63) / 64, (a.n[1] + VPT - 1) / VPT, (a.n[2] + kDnZ - 1) / kDnZ);
  hipLaunchKernelGGL(k_cl_integrate<VPT>, grid, dim3(64, 1, kDnZ), 0, s, a, cf, depth, mask, (const uint32_t*)h->d_img, h->map->W, h->map->H, h->d_col, h->cnt.d);
}

// what the two integrate entries share, from the follow on; depth and mask are packed device images
static int cl_integrate(const char* who, vdo_colour* h, const float* d_depth, const int32_t* d_mask, const uint8_t* image, int64_t stride, int channels, int rgb_order, int image_is_device,
                        int label, const float T[16], int64_t out[3], StageClock::time_point t0) {
  hipStream_t s = h->map->ctx->stream;
  const int W = h->map->W, H = h->map->H;
  cl_follow(h, s);
  const uint8_t* src = image;
  if (!image_is_device) {
    hipMemcpy2DAsync(h->d_src, (size_t)W * channels, image, (size_t)stride, (size_t)W * channels, H, hipMemcpyHostToDevice, s);
    src = h->d_src; stride = (int64_t)W * channels;
  }
  hipLaunchKernelGGL(k_cl_pack, dim3((unsigned)(((int64_t)W * H + 255) / 256)), dim3(256), 0, s, src, (long long)stride, channels, rgb_order, W, H, h->d_img);
  DnArgs a = h->map->a;
  for (int k = 0; k < 12; ++k) a.T[k] = T[k];
  const ClFuse cf{h->p.band, h->p.max_weight, label};
  h->cnt.zero(s);
  switch (h->vpt) {
    case 1: cl_launch_integrate<1>(h, s, a, cf, d_depth, d_mask); break;
    case 2: cl_launch_integrate<2>(h, s, a, cf, d_depth, d_mask); break;
    case 8: cl_launch_integrate<8>(h, s, a, cf, d_depth, d_mask); break;
    default: cl_launch_integrate<4>(h, s, a, cf, d_depth, d_mask); break;
  }
  h->tm.mark_end(s);
  h->cnt.download(s);
  const int rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  for (int k = 0; k < 3; ++k) out[k] = h->cnt.sum(k);
  h->tm.finish(t0);
  return VDO_OK;
}

extern "C" int vdo_colour_create(vdo_dense* map, const vdo_colour_params* p, vdo_colour** out) {
  static const char* who = "vdo_colour_create";
  if (!map) return set_error(VDO_ERR_INVALID, "%s: map is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (!p) return set_error(VDO_ERR_INVALID, "%s: params is null", who);
  if (!is_finite(p->band) || !(p->band > 0.f) || !(p->band <= map->a.trunc))
    return set_error(VDO_ERR_INVALID, "%s: band %g must be positive and at most the map's trunc %g", who, (double)p->band, (double)map->a.trunc);
  if (p->max_weight < 1 || p->max_weight > 255) return set_error(VDO_ERR_INVALID, "%s: max_weight %d outside 1..255", who, p->max_weight);
  if (p->stage_points < 1) return set_error(VDO_ERR_INVALID, "%s: stage_points %d < 1", who, p->stage_points);
  const int rc = ctx_bind(map->ctx);
  if (rc != VDO_OK) return rc;
  vdo_colour* h = new vdo_colour;
  h->map = map; h->p = *p; h->stage_points = p->stage_points;
  for (int k = 0; k < 3; ++k) h->o[k] = map->a.o[k];
  const size_t npix = (size_t)map->W * map->H, sp = (size_t)p->stage_points, nvox = (size_t)map->nvox;
  const bool ok = hipMalloc((void**)&h->d_col, nvox * sizeof(uint32_t)) == hipSuccess && hipMalloc((void**)&h->d_img, npix * sizeof(uint32_t)) == hipSuccess &&
                  hipMalloc((void**)&h->d_src, npix * 4) == hipSuccess && h->cnt.create(kDnSlots, kDnCounters) &&
                  hipMalloc((void**)&h->d_xyz, sp * 3 * sizeof(float)) == hipSuccess && hipMalloc((void**)&h->d_rgba, sp * sizeof(uint32_t)) == hipSuccess && h->tm.create() &&
                  hipMemsetAsync(h->d_col, 0, nvox * sizeof(uint32_t), map->ctx->stream) == hipSuccess && hipStreamSynchronize(map->ctx->stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    cl_free(h);
    return set_error(VDO_ERR_OOM, "%s: device allocation failed for %d x %d x %d voxels and %d x %d images", who, map->a.n[0], map->a.n[1], map->a.n[2], map->W, map->H);
  }
  *out = h;
  return VDO_OK;
}

extern "C" int vdo_colour_destroy(vdo_colour* h) {
  if (!h) return VDO_OK;
  if (ctx_bind(h->map->ctx) == VDO_OK) hipStreamSynchronize(h->map->ctx->stream);
  cl_free(h);
  return VDO_OK;
}

extern "C" int vdo_colour_set_voxels_per_thread(vdo_colour* h, int voxels) {
  if (!h) return set_error(VDO_ERR_INVALID, "vdo_colour_set_voxels_per_thread: handle is null");
  if (voxels != 1 && voxels != 2 && voxels != 4 && voxels != 8) return set_error(VDO_ERR_INVALID, "vdo_colour_set_voxels_per_thread: voxels %d not 1, 2, 4 or 8", voxels);
  h->vpt = voxels;
  return VDO_OK;
}

extern "C" int vdo_colour_integrate(vdo_colour* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, const uint8_t* image,
                                    int64_t image_stride_bytes, int channels, int rgb_order, int src_is_device, int label, const float T[16], int64_t out[3]) {
  static const char* who = "vdo_colour_integrate";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  vdo_dense* m = h->map;
  int rc = check_depth_mask(who, m->W, depth, depth_stride_floats, mask, mask_stride_ints, false);
  if (rc == VDO_OK) rc = cl_check_image(who, m->W, image, image_stride_bytes, channels, rgb_order);
  if (rc != VDO_OK) return rc;
  if (!T) return set_error(VDO_ERR_INVALID, "%s: T is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  rc = ctx_bind(m->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = m->ctx->stream;
  const auto t0 = h->tm.begin(s);
  const float* d_depth = stage_rows(s, m->d_depth, depth, depth_stride_floats, m->W, m->H, src_is_device);
  const int32_t* d_mask = mask ? stage_rows(s, m->d_mask, mask, mask_stride_ints, m->W, m->H, src_is_device) : nullptr;
  return cl_integrate(who, h, d_depth, d_mask, image, image_stride_bytes, channels, rgb_order, src_is_device, label, T, out, t0);
}

extern "C" int vdo_colour_integrate_frame(vdo_colour* h, const vdo_frame_images* f, const uint8_t* image, int64_t image_stride_bytes, int channels, int rgb_order, int image_is_device,
                                          int label, const float T[16], int64_t out[3]) {
  static const char* who = "vdo_colour_integrate_frame";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  int rc = check_frame(who, f, h->map->W, h->map->H, "the map's");
  if (rc == VDO_OK) rc = cl_check_image(who, h->map->W, image, image_stride_bytes, channels, rgb_order);
  if (rc != VDO_OK) return rc;
  if (!T) return set_error(VDO_ERR_INVALID, "%s: T is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  rc = ctx_bind(h->map->ctx);
  if (rc != VDO_OK) return rc;
  const auto t0 = h->tm.begin(h->map->ctx->stream);
  return cl_integrate(who, h, f->d_depth, f->d_mask, image, image_stride_bytes, channels, rgb_order, image_is_device, label, T, out, t0);
}

extern "C" int vdo_colour_sample(vdo_colour* h, int64_t n, const float* xyz, int min_weight, uint8_t* rgba, int is_device, int64_t* n_coloured) {
  static const char* who = "vdo_colour_sample";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (n < 0) return set_error(VDO_ERR_INVALID, "%s: n %lld < 0", who, (long long)n);
  if (n > 0 && !xyz) return set_error(VDO_ERR_INVALID, "%s: xyz is null", who);
  if (n > 0 && !rgba) return set_error(VDO_ERR_INVALID, "%s: rgba is null", who);
  if (min_weight < 1 || min_weight > 255) return set_error(VDO_ERR_INVALID, "%s: min_weight %d outside 1..255", who, min_weight);
  if (!n_coloured) return set_error(VDO_ERR_INVALID, "%s: n_coloured is null", who);
  if (is_device && ((uintptr_t)rgba & 3u)) return set_error(VDO_ERR_INVALID, "%s: a device rgba must be 4-byte aligned (it is written one word per point)", who);
  int rc = ctx_bind(h->map->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->map->ctx->stream;
  const auto t0 = h->tm.begin(s);
  cl_follow(h, s);
  const ClVol v = cl_vol(h);
  h->cnt.zero(s);
  // a device output in windows of 2^30 points, a host output through the staging lists, stage_points at a time
  const long long window = is_device ? kClMaxWindow : (long long)h->stage_points;
  for (long long base = 0; base < n; base += window) {
    const long long cap = n - base < window ? n - base : window;
    const float* i_xyz = xyz + 3 * base;
    uint32_t* o_rgba = (uint32_t*)rgba + base;
    if (!is_device) {
      hipMemcpyAsync(h->d_xyz, xyz + 3 * base, (size_t)cap * 3 * sizeof(float), hipMemcpyHostToDevice, s);
      i_xyz = h->d_xyz; o_rgba = h->d_rgba;
    }
    hipLaunchKernelGGL(k_cl_sample, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, v, (const uint32_t*)h->d_col, cap, i_xyz, min_weight, o_rgba, h->cnt.d);
    if (!is_device) {
      hipMemcpyAsync(rgba + 4 * base, h->d_rgba, (size_t)cap * 4, hipMemcpyDeviceToHost, s);
      rc = check_hip(who, hipStreamSynchronize(s));                          // the staging lists are free for the next window
      if (rc != VDO_OK) return rc;
    }
  }
  h->tm.mark_end(s);
  h->cnt.download(s);
  rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  *n_coloured = h->cnt.sum(0);
  h->tm.finish(t0);
  return VDO_OK;
}

extern "C" int vdo_colour_render(vdo_colour* h, const float* depth, int width, int height, const float K[4], const float T[16], int min_weight, uint8_t* rgba, int is_device,
                                 int64_t out[2]) {
  static const char* who = "vdo_colour_render";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!depth) return set_error(VDO_ERR_INVALID, "%s: depth is null", who);
  if (width < 1) return set_error(VDO_ERR_INVALID, "%s: width %d < 1", who, width);
  if (height < 1) return set_error(VDO_ERR_INVALID, "%s: height %d < 1", who, height);
  if (!K) return set_error(VDO_ERR_INVALID, "%s: K is null", who);
  int rc = check_intrinsics(who, "K", K);
  if (rc != VDO_OK) return rc;
  if (!T) return set_error(VDO_ERR_INVALID, "%s: T is null", who);
  if (min_weight < 1 || min_weight > 255) return set_error(VDO_ERR_INVALID, "%s: min_weight %d outside 1..255", who, min_weight);
  if (!rgba) return set_error(VDO_ERR_INVALID, "%s: rgba is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (is_device && ((uintptr_t)rgba & 3u)) return set_error(VDO_ERR_INVALID, "%s: a device rgba must be 4-byte aligned (it is written one word per pixel)", who);
  rc = check_image_size(who, "width x height =", width, height);
  if (rc == VDO_OK) rc = ctx_bind(h->map->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->map->ctx->stream;
  const auto t0 = h->tm.begin(s);
  cl_follow(h, s);
  const ClVol v = cl_vol(h);
  ClView vw;
  vw.fx = K[0]; vw.fy = K[1]; vw.cx = K[2]; vw.cy = K[3]; vw.W = width;
  dn_centre(T, vw.c);
  for (int k = 0; k < 3; ++k) { vw.R[k] = T[k]; vw.R[3 + k] = T[4 + k]; vw.R[6 + k] = T[8 + k]; }
  h->cnt.zero(s);
  const int npix = width * height;                                           // at most 2^26
  const int window = is_device ? npix : (int)(h->stage_points < npix ? h->stage_points : npix);
  for (int base = 0; base < npix; base += window) {
    const int cap = npix - base < window ? npix - base : window;
    const float* i_depth = depth + base;
    uint32_t* o_rgba = (uint32_t*)rgba + base;
    if (!is_device) {
      hipMemcpyAsync(h->d_xyz, depth + base, (size_t)cap * sizeof(float), hipMemcpyHostToDevice, s);
      i_depth = h->d_xyz; o_rgba = h->d_rgba;
    }
    hipLaunchKernelGGL(k_cl_render, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, v, vw, (const uint32_t*)h->d_col, base, cap, i_depth, min_weight, o_rgba, h->cnt.d);
    if (!is_device) {
      hipMemcpyAsync(rgba + 4 * (size_t)base, h->d_rgba, (size_t)cap * 4, hipMemcpyDeviceToHost, s);
      rc = check_hip(who, hipStreamSynchronize(s));
      if (rc != VDO_OK) return rc;
    }
  }
  h->tm.mark_end(s);
  h->cnt.download(s);
  rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  out[0] = h->cnt.sum(0); out[1] = h->cnt.sum(1);
  h->tm.finish(t0);
  return VDO_OK;
}

extern "C" int vdo_colour_clear(vdo_colour* h) {
  static const char* who = "vdo_colour_clear";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  const int rc = ctx_bind(h->map->ctx);
  if (rc != VDO_OK) return rc;
  hipMemsetAsync(h->d_col, 0, (size_t)h->map->nvox * sizeof(uint32_t), h->map->ctx->stream);
  for (int k = 0; k < 3; ++k) h->o[k] = h->map->a.o[k];
  return check_hip(who, hipStreamSynchronize(h->map->ctx->stream));
}

extern "C" int vdo_colour_get_volume(vdo_colour* h, uint32_t* words, int32_t origin[3]) {
  static const char* who = "vdo_colour_get_volume";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!words && !origin) return set_error(VDO_ERR_INVALID, "%s: words and origin are both null", who);
  const int rc = ctx_bind(h->map->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->map->ctx->stream;
  cl_follow(h, s);
  if (words) hipMemcpyAsync(words, h->d_col, (size_t)h->map->nvox * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
  const int rs = sync_check(who, s);
  if (rs != VDO_OK) return rs;
  if (origin) for (int k = 0; k < 3; ++k) origin[k] = h->o[k];
  return VDO_OK;
}

extern "C" int vdo_colour_set_volume(vdo_colour* h, const uint32_t* words) {
  static const char* who = "vdo_colour_set_volume";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!words) return set_error(VDO_ERR_INVALID, "%s: words is null", who);
  const int rc = ctx_bind(h->map->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->map->ctx->stream;
  cl_follow(h, s);
  hipMemcpyAsync(h->d_col, words, (size_t)h->map->nvox * sizeof(uint32_t), hipMemcpyHostToDevice, s);
  return sync_check(who, s);
}

extern "C" int vdo_colour_last_timing(vdo_colour* h, double ms[2]) {
  return last_timing("vdo_colour_last_timing", h ? &h->tm : nullptr, ms);
}
