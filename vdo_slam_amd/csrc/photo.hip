// Photometric aligner: the intensity term beside the aligner's point-to-plane ICP (align.hip) - the grey value of every frame pixel against the
// bilinear grey value of a model image at the pixel's projection, one 6-vector Jacobian row per sample about the same twist, the same 28 sums in the
// same tree, and the joint solve: both linearisations at the same T, their weighted sum, the aligner's host step.  The semantics are this
// library's own, stated in include/vdo_slam_hip.h ("Photometric aligner") and restated in NumPy by tests/photo_ref.py.  The rows are fp32 with one
// rounded operation per step in the header's order (the library is built with -ffp-contract=off; / and floorf are correctly rounded); the terms are
// exact products in double; every sum is ONE fixed adjacent-pair tree over the slot vector.
//
//   k_ph_grey        one thread per pixel: 1, 3 or 4 bytes -> Y = (77 R + 150 G + 29 B + 128) >> 8 as a float.
//   k_ph_pack_model  one thread per model pixel: (depth, intensity) -> one 8-byte pair; with the keep-as-model rule the depth is 0 where the frame's
//                    depth test fails or the mask is set.
//   k_ph_rows<ROWS>  the shape of k_al_rows: one thread per sample, one wave per 8 x 8 sample tile, four consecutive tiles per workgroup, the
//                    transposing xor-butterfly into 256 bytes per tile (k_al_rows' own text: shared through a function it costs that kernel a
//                    register).  The interleaved model makes the four corners of the bilinear cell two pairs of adjacent 8-byte words,
//                    (y0, x0) (y0, x0 + 1) and the same one row down.
//   k_ph_tree        pt_tree of pair_tree.hpp, the tree k_al_tree runs: eight levels per launch, until one node is left.
//
// NO OUT-OF-RANGE ACCESS: the one gathered address of the model comes from float compares of floorf(u), floorf(v) against 0 and Wm - 2 / Hm - 2 made
// before any conversion to int (a NaN fails them; Wm < 2 or Hm < 2 fails them always), so x0 + 1 <= Wm - 1 and y0 + 1 <= Hm - 1; the frame and the
// grey image are read at (i * s, j * s) with i < Ws, j < Hs; a partial is written at tile < tiles, a row at a sample of the grid, a pixel of the
// pack kernels at an index below the pixel count.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"
#include "frame_images.hpp"
#include "stage.hpp"
#include "dense.hpp"
#include "pair_tree.hpp"

namespace vdo {

constexpr int kPhTerms = 28;
constexpr int kPhVals = kPtVals;                                              // the 28 terms, then used, masked, no model, far as doubles
constexpr int kPhSpan = kPtSpan;                                             // nodes per workgroup of k_ph_tree

// what the row kernel takes by value
struct PhArgs {
  float fx, fy, cx, cy, min_d, max_d, max_dist, max_diff;
  int W, s, Ws, Hs, tiles_x, tiles;
  float T[12];
  float fxm, fym, cxm, cym, xmax, ymax;                                    // xmax = (float)(Wm - 2), ymax = (float)(Hm - 2)
  int Wm;
  float Tm[12];
};

enum { kPhUsed = 0, kPhNoDepth, kPhMasked, kPhNoModel, kPhFar };

__device__ __forceinline__ bool ph_valid(float i) { return dn_finite(i) && i >= 0.f; }
__device__ __forceinline__ bool ph_usable(float2 p) { return dn_finite(p.x) && p.x > 0.f && ph_valid(p.y); }

__global__ __launch_bounds__(256) void k_ph_grey(const uint8_t* __restrict__ src, long long stride, int channels, int bgr, int W, int H, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W * H) return;
  const int x = i % W, y = i / W;
  const uint8_t* p = src + (size_t)y * (size_t)stride + (size_t)x * channels;
  uint32_t Y;
  if (channels == 1) {
    Y = p[0];
  } else {
    const uint32_t r = p[bgr ? 2 : 0], g = p[1], b = p[bgr ? 0 : 2];
    Y = (77u * r + 150u * g + 29u * b + 128u) >> 8;
  }
  out[i] = (float)Y;
}

// gate != 0: the keep-as-model rule with the frame's depth range (min_d already max(min_depth, 0)) and mask (may be null)
__global__ __launch_bounds__(256) void k_ph_pack_model(const float* __restrict__ depth, const int32_t* __restrict__ mask, const float* __restrict__ inten, int n, int gate, float min_d,
                                                       float max_d, float2* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float d = depth[i];
  if (gate && !(dn_finite(d) && d > min_d && d <= max_d && !(mask && mask[i] != 0))) d = 0.0f;
  out[i] = make_float2(d, inten[i]);
}

// one sample in the header's order: its class, and J, e when it is used
__device__ __forceinline__ int ph_sample(const PhArgs& a, int x, int y, const float* __restrict__ depth, const int32_t* __restrict__ mask, const float* __restrict__ grey,
                                         const float2* __restrict__ model, float J[6], float* e_out) {
  const size_t at = (size_t)y * a.W + x;
  const float d = depth[at], iF = grey[at];
  if (!(dn_finite(d) && d > a.min_d && d <= a.max_d && ph_valid(iF))) return kPhNoDepth;
  if (mask && mask[at] != 0) return kPhMasked;
  const float dx = ((float)x - a.cx) / a.fx, dy = ((float)y - a.cy) / a.fy;
  const float Pc[3] = {dx * d, dy * d, d};
  const float q[3] = {Pc[0] - a.T[3], Pc[1] - a.T[7], Pc[2] - a.T[11]};
  float Pw[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) Pw[k] = (a.T[k] * q[0] + a.T[4 + k] * q[1]) + a.T[8 + k] * q[2];
  const float Xm = (a.Tm[0] * Pw[0] + a.Tm[1] * Pw[1]) + (a.Tm[2] * Pw[2] + a.Tm[3]);
  const float Ym = (a.Tm[4] * Pw[0] + a.Tm[5] * Pw[1]) + (a.Tm[6] * Pw[2] + a.Tm[7]);
  const float Zm = (a.Tm[8] * Pw[0] + a.Tm[9] * Pw[1]) + (a.Tm[10] * Pw[2] + a.Tm[11]);
  if (!(dn_finite(Zm) && Zm > FLT_MIN)) return kPhNoModel;
  const float u = (a.fxm * Xm) / Zm + a.cxm, v = (a.fym * Ym) / Zm + a.cym;
  const float x0 = floorf(u), y0 = floorf(v);
  if (!(dn_finite(u) && dn_finite(v) && x0 >= 0.f && x0 <= a.xmax && y0 >= 0.f && y0 <= a.ymax)) return kPhNoModel;
  const float fa = u - x0, fb = v - y0;
  const float2* m = model + ((size_t)(int)y0 * a.Wm + (int)x0);
  const float2 p00 = m[0], p10 = m[1], p01 = m[a.Wm], p11 = m[a.Wm + 1];
  if (!(ph_usable(p00) && ph_usable(p10) && ph_usable(p01) && ph_usable(p11))) return kPhNoModel;
  if (!(fabsf(p00.x - Zm) <= a.max_dist && fabsf(p10.x - Zm) <= a.max_dist && fabsf(p01.x - Zm) <= a.max_dist && fabsf(p11.x - Zm) <= a.max_dist)) return kPhFar;
  const float dt = p10.y - p00.y, db = p11.y - p01.y;
  const float top = p00.y + fa * dt, bot = p01.y + fa * db;
  const float im = top + fb * (bot - top);
  const float gx = dt + fb * (db - dt), gy = bot - top;
  const float e = im - iF;
  if (!(fabsf(e) <= a.max_diff)) return kPhFar;
  const float iz = 1.0f / Zm, ax = (a.fxm * gx) * iz, ay = (a.fym * gy) * iz, az = -(((ax * Xm) + (ay * Ym)) * iz);
  float gw[3], gc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) gw[k] = (a.Tm[k] * ax + a.Tm[4 + k] * ay) + a.Tm[8 + k] * az;
#pragma unroll
  for (int k = 0; k < 3; ++k) gc[k] = (a.T[4 * k] * gw[0] + a.T[4 * k + 1] * gw[1]) + a.T[4 * k + 2] * gw[2];
  *e_out = e;
  J[0] = gc[0]; J[1] = gc[1]; J[2] = gc[2];
  J[3] = Pc[1] * gc[2] - Pc[2] * gc[1];
  J[4] = Pc[2] * gc[0] - Pc[0] * gc[2];
  J[5] = Pc[0] * gc[1] - Pc[1] * gc[0];
  return kPhUsed;
}

template <bool ROWS>
__global__ __launch_bounds__(256) void k_ph_rows(PhArgs a, const float* __restrict__ depth, const int32_t* __restrict__ mask, const float* __restrict__ grey,
                                                 const float2* __restrict__ model, double* __restrict__ part, float* __restrict__ rows) {
  const int lane = threadIdx.x, tile = (int)blockIdx.x * 4 + (int)threadIdx.y;
  if (tile >= a.tiles) return;                                             // the whole wave leaves: nothing below waits for another wave
  const int i = (tile % a.tiles_x) * 8 + (lane & 7), j = (tile / a.tiles_x) * 8 + (lane >> 3);
  float J[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, e = 0.f, w = 0.f;
  int cls = -1;
  if (i < a.Ws && j < a.Hs) {
    float Jt[6], et = 0.f;
    cls = ph_sample(a, i * a.s, j * a.s, depth, mask, grey, model, Jt, &et);
    if (cls == kPhUsed) {
#pragma unroll
      for (int k = 0; k < 6; ++k) J[k] = Jt[k];
      e = et; w = 1.f;
    }
    if (ROWS) {
      float4* o = reinterpret_cast<float4*>(rows + ((size_t)j * a.Ws + i) * 8);
      o[0] = make_float4(J[0], J[1], J[2], J[3]);
      o[1] = make_float4(J[4], J[5], e, w);
    }
  }
  double v[kPhVals];
  {
    double Jd[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) Jd[k] = (double)J[k];
    int t = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) v[t++] = Jd[r] * Jd[c];
#pragma unroll
    for (int r = 0; r < 6; ++r) v[21 + r] = Jd[r] * (double)e;
    v[27] = (double)e * (double)e;
    v[28] = cls == kPhUsed ? 1.0 : 0.0; v[29] = cls == kPhMasked ? 1.0 : 0.0; v[30] = cls == kPhNoModel ? 1.0 : 0.0; v[31] = cls == kPhFar ? 1.0 : 0.0;
  }
  // the first six levels: at mask m the lane with the bit clear keeps the lower half of its values, its partner the upper half
#pragma unroll
  for (int m = 1, n = kPhVals / 2; m <= 16; m <<= 1, n >>= 1) {
    const bool up = (lane & m) != 0;
#pragma unroll
    for (int k = 0; k < n; ++k) {
      const double keep = up ? v[k + n] : v[k], send = up ? v[k] : v[k + n];
      v[k] = keep + __shfl_xor(send, m, 64);
    }
  }
  v[0] = v[0] + __shfl_xor(v[0], 32, 64);
  if (lane < 32) {
    const int idx = ((lane & 1) << 4) | ((lane & 2) << 2) | (lane & 4) | ((lane & 8) >> 2) | ((lane & 16) >> 4);
    part[(size_t)tile * kPhVals + idx] = v[0];
  }
}

// Eight levels of the tree over the nodes [256 * block, 256 * block + 256) of every value: in [n_real][32] (a node >= n_real holds +0.0), P the
// padded node count (a power of two >= n_real), out [max(P / 256, 1)][32].  A pair whose second node lies beyond P's level does not exist.
__global__ __launch_bounds__(256) void k_ph_tree(const double* __restrict__ in, int n_real, int P, double* __restrict__ out) {
  __shared__ double lds[8][kPhVals];
  pt_tree(in, n_real, P, out, lds);
}

}  // namespace vdo

struct vdo_photo {
  vdo_ctx* ctx = nullptr;
  int W = 0, H = 0, Ws = 0, Hs = 0, Wm = 0, Hm = 0;
  vdo_photo_params p{};
  vdo::PhArgs a{};
  size_t npix = 0;
  bool has_image = false, has_model = false, has_rows = false;
  float* d_depth = nullptr;                               // [H][W] staging (a host model's depth too)
  int32_t* d_mask = nullptr;                              // [H][W] staging (a host model's intensity too, as floats)
  uint8_t* d_src = nullptr;                               // [H][W][4] staging of a host image
  float* d_grey = nullptr;                                // [H][W] the current frame's I
  float2* d_model = nullptr;                              // [npix] the (depth, intensity) pairs
  double* d_part[2] = {nullptr, nullptr};                 // [tiles][32] the tile partials; [max(P / 256, 1)][32] the level above; then in turns
  float* d_rows = nullptr;                                // [Hs][Ws][8] with keep_rows
  double* h_sums = nullptr;                               // pinned, [32]
  vdo::StageTimer tm;
};

using namespace vdo;

static void ph_free(vdo_photo* h) {
  hipFree(h->d_depth); hipFree(h->d_mask); hipFree(h->d_src); hipFree(h->d_grey); hipFree(h->d_model); hipFree(h->d_part[0]); hipFree(h->d_part[1]); hipFree(h->d_rows);
  if (h->h_sums) hipHostFree(h->h_sums);
  h->tm.destroy();
  delete h;
}

extern "C" int vdo_photo_create(vdo_ctx* ctx, int width, int height, const vdo_photo_params* p, vdo_photo** out) {
  static const char* who = "vdo_photo_create";
  if (!ctx) return set_error(VDO_ERR_INVALID, "%s: ctx is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (!p) return set_error(VDO_ERR_INVALID, "%s: params is null", who);
  if (width < 1) return set_error(VDO_ERR_INVALID, "%s: width %d < 1", who, width);
  if (height < 1) return set_error(VDO_ERR_INVALID, "%s: height %d < 1", who, height);
  int rc = check_intrinsics(who, "K", p->K);
  if (rc == VDO_OK) rc = check_depth_range(who, p->min_depth, p->max_depth);
  if (rc != VDO_OK) return rc;
  if (!is_finite(p->max_dist) || !(p->max_dist > 0.f)) return set_error(VDO_ERR_INVALID, "%s: max_dist %g must be positive and finite", who, (double)p->max_dist);
  if (!is_finite(p->max_diff) || !(p->max_diff > 0.f)) return set_error(VDO_ERR_INVALID, "%s: max_diff %g must be positive and finite", who, (double)p->max_diff);
  if (p->subsample < 1 || p->subsample > 8) return set_error(VDO_ERR_INVALID, "%s: subsample %d outside 1..8", who, p->subsample);
  if (p->min_pixels < 6) return set_error(VDO_ERR_INVALID, "%s: min_pixels %d < 6", who, p->min_pixels);
  if (p->max_iterations < 1 || p->max_iterations > 64) return set_error(VDO_ERR_INVALID, "%s: max_iterations %d outside 1..64", who, p->max_iterations);
  if (!is_finite(p->eps) || !(p->eps >= 0.f)) return set_error(VDO_ERR_INVALID, "%s: eps %g must be finite and >= 0", who, (double)p->eps);
  if (p->keep_rows != 0 && p->keep_rows != 1) return set_error(VDO_ERR_INVALID, "%s: keep_rows %d not 0 or 1", who, p->keep_rows);
  rc = check_image_size(who, "width x height =", width, height);
  if (rc == VDO_OK) rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  vdo_photo* h = new vdo_photo;
  h->ctx = ctx; h->W = width; h->H = height; h->p = *p;
  const int s = p->subsample;
  h->Ws = (width + s - 1) / s; h->Hs = (height + s - 1) / s;
  PhArgs& a = h->a;
  a.fx = p->K[0]; a.fy = p->K[1]; a.cx = p->K[2]; a.cy = p->K[3];
  a.min_d = p->min_depth > 0.f ? p->min_depth : 0.f; a.max_d = p->max_depth; a.max_dist = p->max_dist; a.max_diff = p->max_diff;
  a.W = width; a.s = s; a.Ws = h->Ws; a.Hs = h->Hs; a.tiles_x = (h->Ws + 7) / 8; a.tiles = a.tiles_x * ((h->Hs + 7) / 8);
  h->npix = (size_t)width * height;
  const size_t n1 = (size_t)(pt_pow2(a.tiles) / kPhSpan > 1 ? pt_pow2(a.tiles) / kPhSpan : 1);
  bool ok = hipMalloc((void**)&h->d_depth, h->npix * sizeof(float)) == hipSuccess && hipMalloc((void**)&h->d_mask, h->npix * sizeof(int32_t)) == hipSuccess &&
            hipMalloc((void**)&h->d_src, h->npix * 4) == hipSuccess && hipMalloc((void**)&h->d_grey, h->npix * sizeof(float)) == hipSuccess &&
            hipMalloc((void**)&h->d_model, h->npix * sizeof(float2)) == hipSuccess &&
            hipMalloc((void**)&h->d_part[0], (size_t)a.tiles * kPhVals * sizeof(double)) == hipSuccess && hipMalloc((void**)&h->d_part[1], n1 * kPhVals * sizeof(double)) == hipSuccess &&
            hipHostMalloc((void**)&h->h_sums, kPhVals * sizeof(double), hipHostMallocDefault) == hipSuccess && h->tm.create();
  if (ok && p->keep_rows) ok = hipMalloc((void**)&h->d_rows, (size_t)h->Ws * h->Hs * 8 * sizeof(float)) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    ph_free(h);
    return set_error(VDO_ERR_OOM, "%s: device allocation failed for %d x %d images", who, width, height);
  }
  *out = h;
  return VDO_OK;
}

extern "C" int vdo_photo_destroy(vdo_photo* h) {
  if (!h) return VDO_OK;
  if (ctx_bind(h->ctx) == VDO_OK) hipStreamSynchronize(h->ctx->stream);
  ph_free(h);
  return VDO_OK;
}

extern "C" int vdo_photo_set_image(vdo_photo* h, const uint8_t* image, int64_t stride, int channels, int rgb_order, int is_device) {
  static const char* who = "vdo_photo_set_image";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!image) return set_error(VDO_ERR_INVALID, "%s: image is null", who);
  if (channels != 1 && channels != 3 && channels != 4) return set_error(VDO_ERR_INVALID, "%s: channels %d not 1, 3 or 4", who, channels);
  if (rgb_order != 0 && rgb_order != 1) return set_error(VDO_ERR_INVALID, "%s: rgb_order %d not 0 or 1", who, rgb_order);
  if (stride < (int64_t)h->W * channels) return set_error(VDO_ERR_INVALID, "%s: image_stride_bytes %lld smaller than width * channels = %lld", who, (long long)stride, (long long)h->W * channels);
  int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const uint8_t* src = image;
  if (!is_device) {
    hipMemcpy2DAsync(h->d_src, (size_t)h->W * channels, image, (size_t)stride, (size_t)h->W * channels, h->H, hipMemcpyHostToDevice, s);
    src = h->d_src; stride = (int64_t)h->W * channels;
  }
  hipLaunchKernelGGL(k_ph_grey, dim3((unsigned)((h->npix + 255) / 256)), dim3(256), 0, s, src, (long long)stride, channels, rgb_order, h->W, h->H, h->d_grey);
  rc = sync_check(who, s);
  h->has_image = rc == VDO_OK;
  return rc;
}

// the model's intrinsics, size and pose into the kernel arguments
static void ph_take_model(vdo_photo* h, int Wm, int Hm, const float Km[4], const float Tm[16]) {
  PhArgs& a = h->a;
  a.fxm = Km[0]; a.fym = Km[1]; a.cxm = Km[2]; a.cym = Km[3]; a.xmax = (float)(Wm - 2); a.ymax = (float)(Hm - 2); a.Wm = Wm;
  for (int k = 0; k < 12; ++k) a.Tm[k] = Tm[k];
  h->Wm = Wm; h->Hm = Hm; h->has_model = true;
}

extern "C" int vdo_photo_set_model(vdo_photo* h, const float* depth, const float* intensity, int Wm, int Hm, const float Km[4], const float Tm[16], int is_device) {
  static const char* who = "vdo_photo_set_model";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!depth) return set_error(VDO_ERR_INVALID, "%s: depth is null", who);
  if (!intensity) return set_error(VDO_ERR_INVALID, "%s: intensity is null", who);
  if (!Km) return set_error(VDO_ERR_INVALID, "%s: Km is null", who);
  if (!Tm) return set_error(VDO_ERR_INVALID, "%s: Tm is null", who);
  if (Wm < 1) return set_error(VDO_ERR_INVALID, "%s: model_width %d < 1", who, Wm);
  if (Hm < 1) return set_error(VDO_ERR_INVALID, "%s: model_height %d < 1", who, Hm);
  int rc = check_intrinsics(who, "Km", Km);
  if (rc == VDO_OK) rc = check_image_size(who, "the model of", Wm, Hm);
  if (rc != VDO_OK) return rc;
  const size_t nm = (size_t)Wm * Hm;
  if (nm > h->npix) return set_error(VDO_ERR_UNSUPPORTED, "%s: a model of %d x %d has more pixels than the %d x %d frame the handle's model was sized for", who, Wm, Hm, h->W, h->H);
  rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  if (!is_device) {
    hipMemcpyAsync(h->d_depth, depth, nm * sizeof(float), hipMemcpyHostToDevice, s);
    hipMemcpyAsync(h->d_mask, intensity, nm * sizeof(float), hipMemcpyHostToDevice, s);
    depth = h->d_depth; intensity = reinterpret_cast<const float*>(h->d_mask);
  }
  hipLaunchKernelGGL(k_ph_pack_model, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, s, depth, (const int32_t*)nullptr, intensity, (int)nm, 0, 0.f, 0.f, h->d_model);
  rc = sync_check(who, s);
  if (rc != VDO_OK) { h->has_model = false; return rc; }
  ph_take_model(h, Wm, Hm, Km, Tm);
  return VDO_OK;
}

namespace vdo {

// where a call's depth and mask lie on the device once ph_stage has queued the copies
struct PhSrc { const float* depth; const int32_t* mask; };

static PhSrc ph_stage(vdo_photo* h, const float* depth, int64_t dstride, const int32_t* mask, int64_t mstride, int src_is_device) {
  hipStream_t s = h->ctx->stream;
  return PhSrc{stage_rows(s, h->d_depth, depth, dstride, h->W, h->H, src_is_device), mask ? stage_rows(s, h->d_mask, mask, mstride, h->W, h->H, src_is_device) : nullptr};
}

static int ph_check_images(const char* who, vdo_photo* h, const float* depth, int64_t dstride, const int32_t* mask, int64_t mstride) {
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  return check_depth_mask(who, h->W, depth, dstride, mask, mstride, false);
}

static int ph_check_frame(const char* who, vdo_photo* h, const vdo_frame_images* f) {
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  return check_frame(who, f, h->W, h->H, "the photometric aligner's");
}

// the two keep-as-model entries after their own checks
static int ph_keep_entry(const char* who, vdo_photo* h, bool staged, const float* depth, int64_t dstride, const int32_t* mask, int64_t mstride, int src_is_device, const float T[16]) {
  if (!T) return set_error(VDO_ERR_INVALID, "%s: T is null", who);
  if (!h->has_image) return set_error(VDO_ERR_INVALID, "%s: no image is set", who);
  int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const PhSrc src = staged ? ph_stage(h, depth, dstride, mask, mstride, src_is_device) : PhSrc{depth, mask};
  hipLaunchKernelGGL(k_ph_pack_model, dim3((unsigned)((h->npix + 255) / 256)), dim3(256), 0, s, src.depth, src.mask, (const float*)h->d_grey, (int)h->npix, 1, h->a.min_d, h->a.max_d,
                     h->d_model);
  rc = sync_check(who, s);
  if (rc != VDO_OK) { h->has_model = false; return rc; }
  ph_take_model(h, h->W, h->H, h->p.K, T);
  return VDO_OK;
}

// one linearisation of packed device images at T: the launches, the download of the 32 values; *dev_ms the device time from ev0 (recorded by the caller)
static int ph_linearise(const char* who, vdo_photo* h, PhSrc src, const float T[16], double sums[28], int64_t counts[5], double* dev_ms) {
  hipStream_t s = h->ctx->stream;
  PhArgs a = h->a;
  for (int k = 0; k < 12; ++k) a.T[k] = T[k];
  const dim3 grid((unsigned)((a.tiles + 3) / 4)), block(64, 4);
  if (h->d_rows) hipLaunchKernelGGL(k_ph_rows<true>, grid, block, 0, s, a, src.depth, src.mask, (const float*)h->d_grey, (const float2*)h->d_model, h->d_part[0], h->d_rows);
  else hipLaunchKernelGGL(k_ph_rows<false>, grid, block, 0, s, a, src.depth, src.mask, (const float*)h->d_grey, (const float2*)h->d_model, h->d_part[0], (float*)nullptr);
  int n = a.tiles, P = pt_pow2(a.tiles), from = 0;
  do {
    const int blocks = P / kPhSpan > 1 ? P / kPhSpan : 1;
    hipLaunchKernelGGL(k_ph_tree, dim3((unsigned)blocks), dim3(256), 0, s, (const double*)h->d_part[from], n, P, h->d_part[from ^ 1]);
    n = P = blocks;
    from ^= 1;
  } while (P > 1);
  h->tm.mark_end(s);
  hipMemcpyAsync(h->h_sums, h->d_part[from], kPhVals * sizeof(double), hipMemcpyDeviceToHost, s);
  const int rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  h->has_rows = h->d_rows != nullptr;
  for (int k = 0; k < kPhTerms; ++k) sums[k] = h->h_sums[k];
  counts[kPhUsed] = (int64_t)h->h_sums[28]; counts[kPhMasked] = (int64_t)h->h_sums[29]; counts[kPhNoModel] = (int64_t)h->h_sums[30]; counts[kPhFar] = (int64_t)h->h_sums[31];
  counts[kPhNoDepth] = (int64_t)h->Ws * h->Hs - counts[kPhUsed] - counts[kPhMasked] - counts[kPhNoModel] - counts[kPhFar];
  *dev_ms = elapsed_ms(h->tm.ev0, h->tm.ev1);
  return VDO_OK;
}

static int ph_check_ready(const char* who, vdo_photo* h) {
  if (!h->has_image) return set_error(VDO_ERR_INVALID, "%s: no image is set", who);
  if (!h->has_model) return set_error(VDO_ERR_INVALID, "%s: no model is set", who);
  return VDO_OK;
}

// the two linearise entries after their own checks; staged: the images go through ph_stage
static int ph_linearise_entry(const char* who, vdo_photo* h, bool staged, const float* depth, int64_t dstride, const int32_t* mask, int64_t mstride, int src_is_device, const float T[16],
                              double sums[28], int64_t counts[5]) {
  if (!T) return set_error(VDO_ERR_INVALID, "%s: T is null", who);
  if (!sums) return set_error(VDO_ERR_INVALID, "%s: sums is null", who);
  if (!counts) return set_error(VDO_ERR_INVALID, "%s: counts is null", who);
  int rc = ph_check_ready(who, h);
  if (rc == VDO_OK) rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  const auto t0 = h->tm.begin(h->ctx->stream);
  const PhSrc src = staged ? ph_stage(h, depth, dstride, mask, mstride, src_is_device) : PhSrc{depth, mask};
  double s28[28], dev_ms = 0;
  int64_t c5[5];
  const int rl = ph_linearise(who, h, src, T, s28, c5, &dev_ms);
  if (rl != VDO_OK) return rl;
  std::memcpy(sums, s28, sizeof s28); std::memcpy(counts, c5, sizeof c5);
  h->tm.finish(t0, dev_ms);
  return VDO_OK;
}

static bool ph_weight_ok(double w) { return std::isfinite(w) && w > 0.0; }

static void ph_combine(const double* geo, const double* photo, double weight, double* out) {
  const double lam = weight * weight;
  for (int k = 0; k < 28; ++k) {
    const double scaled = lam * photo[k];
    out[k] = (geo ? geo[k] : 0.0) + scaled;
  }
}

// the two solve entries after their own checks
static int ph_solve_entry(const char* who, vdo_photo* h, vdo_align* geo, bool staged, const float* depth, int64_t dstride, const int32_t* mask, int64_t mstride, int src_is_device,
                          double weight, const float T_init[16], float T_out[16], vdo_photo_report* report, double* trace) {
  if (!T_init) return set_error(VDO_ERR_INVALID, "%s: T_init is null", who);
  if (!T_out) return set_error(VDO_ERR_INVALID, "%s: T_out is null", who);
  if (!ph_weight_ok(weight)) return set_error(VDO_ERR_INVALID, "%s: weight %g must be positive and finite", who, weight);
  int rc = ph_check_ready(who, h);
  if (rc != VDO_OK) return rc;
  int geo_min = 0;
  if (geo) {
    int gW = 0, gH = 0;
    bool g_model = false;
    vdo_ctx* gctx = nullptr;
    al_info(geo, &gW, &gH, &geo_min, &g_model, &gctx);
    if (gW != h->W || gH != h->H) return set_error(VDO_ERR_INVALID, "%s: geo is for %d x %d frames, the handle for %d x %d", who, gW, gH, h->W, h->H);
    if (gctx->device != h->ctx->device) return set_error(VDO_ERR_INVALID, "%s: geo lives on device %d, the handle on device %d", who, gctx->device, h->ctx->device);
    if (!g_model) return set_error(VDO_ERR_INVALID, "%s: geo has no model set", who);
  }
  rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const auto t0 = h->tm.begin(s);
  const PhSrc src = staged ? ph_stage(h, depth, dstride, mask, mstride, src_is_device) : PhSrc{depth, mask};
  if (geo) {                                                                // the aligner reads the packed device images on its own stream: they are complete first
    rc = sync_check(who, s);
    if (rc != VDO_OK) return rc;
  }
  float T[16], Tn[16];
  std::memcpy(T, T_init, sizeof T);
  vdo_photo_report rep{};
  double dev_total = 0;
  for (int it = 0; it < h->p.max_iterations; ++it) {
    double sp[28], sg[28] = {}, joint[28], dev_ms = 0, rms = 0;
    int64_t cp[5], cg[5] = {0, 0, 0, 0, 0};
    if (it > 0 || geo) hipEventRecord(h->tm.ev0, s);
    const int rl = ph_linearise(who, h, src, T, sp, cp, &dev_ms);
    if (rl != VDO_OK) return rl;
    dev_total += dev_ms;
    if (geo) {
      const int rg = vdo_align_linearise(geo, src.depth, h->W, src.mask, h->W, 1, T, sg, cg);
      if (rg != VDO_OK) return rg;
      rc = ctx_bind(h->ctx);
      if (rc != VDO_OK) return rc;
    }
    if (trace) {
      double* row = trace + (size_t)it * VDO_PHOTO_TRACE_ROW;
      for (int k = 0; k < 16; ++k) row[k] = (double)T[k];
      for (int k = 0; k < 28; ++k) { row[16 + k] = sg[k]; row[49 + k] = sp[k]; }
      for (int k = 0; k < 5; ++k) { row[44 + k] = (double)cg[k]; row[77 + k] = (double)cp[k]; }
    }
    const double rms_g = cg[0] > 0 ? std::sqrt(sg[27] / (double)cg[0]) : 0.0, rms_p = cp[0] > 0 ? std::sqrt(sp[27] / (double)cp[0]) : 0.0;
    rep.iterations = it + 1; rep.used_geo = cg[0]; rep.used_photo = cp[0]; rep.rms_geo_last = rms_g; rep.rms_photo_last = rms_p;
    if (it == 0) { rep.rms_geo_first = rms_g; rep.rms_photo_first = rms_p; }
    if (cp[0] < h->p.min_pixels || (geo && cg[0] < geo_min)) {
      rep.status = 1;
      for (int k = 0; k < 6; ++k) rep.xi[k] = 0.0;
      break;
    }
    ph_combine(geo ? sg : nullptr, sp, weight, joint);
    rep.status = vdo_align_step(joint, cg[0] + cp[0], 6, T, Tn, rep.xi, &rms);
    if (rep.status != 0) break;
    std::memcpy(T, Tn, sizeof T);
    bool small = true;
    for (int k = 0; k < 6; ++k) small = small && std::fabs(rep.xi[k]) <= (double)h->p.eps;
    if (small) break;
  }
  std::memcpy(T_out, T, sizeof T);
  if (report) *report = rep;
  h->tm.finish(t0, dev_total);
  return VDO_OK;
}

}  // namespace vdo

extern "C" int vdo_photo_keep_as_model(vdo_photo* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device, const float T[16]) {
  static const char* who = "vdo_photo_keep_as_model";
  const int rc = ph_check_images(who, h, depth, depth_stride_floats, mask, mask_stride_ints);
  if (rc != VDO_OK) return rc;
  return ph_keep_entry(who, h, true, depth, depth_stride_floats, mask, mask_stride_ints, src_is_device, T);
}

extern "C" int vdo_photo_keep_as_model_frame(vdo_photo* h, const vdo_frame_images* f, const float T[16]) {
  static const char* who = "vdo_photo_keep_as_model_frame";
  const int rc = ph_check_frame(who, h, f);
  if (rc != VDO_OK) return rc;
  return ph_keep_entry(who, h, false, f->d_depth, h->W, f->d_mask, h->W, 1, T);
}

extern "C" int vdo_photo_get_image(vdo_photo* h, float* grey) {
  static const char* who = "vdo_photo_get_image";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!grey) return set_error(VDO_ERR_INVALID, "%s: grey is null", who);
  if (!h->has_image) return set_error(VDO_ERR_INVALID, "%s: no image is set", who);
  const int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipMemcpyAsync(grey, h->d_grey, h->npix * sizeof(float), hipMemcpyDeviceToHost, h->ctx->stream);
  return check_hip(who, hipStreamSynchronize(h->ctx->stream));
}

extern "C" int vdo_photo_get_model(vdo_photo* h, float* pairs, int* model_width, int* model_height) {
  static const char* who = "vdo_photo_get_model";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!h->has_model) return set_error(VDO_ERR_INVALID, "%s: no model is set", who);
  if (pairs) {
    const int rc = ctx_bind(h->ctx);
    if (rc != VDO_OK) return rc;
    hipMemcpyAsync(pairs, h->d_model, (size_t)h->Wm * h->Hm * sizeof(float2), hipMemcpyDeviceToHost, h->ctx->stream);
    const int rs = check_hip(who, hipStreamSynchronize(h->ctx->stream));
    if (rs != VDO_OK) return rs;
  }
  if (model_width) *model_width = h->Wm;
  if (model_height) *model_height = h->Hm;
  return VDO_OK;
}

extern "C" int vdo_photo_combine(const double geo[28], const double photo[28], double weight, double out[28]) {
  static const char* who = "vdo_photo_combine";
  if (!photo) return set_error(VDO_ERR_INVALID, "%s: photo is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (!ph_weight_ok(weight)) return set_error(VDO_ERR_INVALID, "%s: weight %g must be positive and finite", who, weight);
  ph_combine(geo, photo, weight, out);
  return VDO_OK;
}

extern "C" int vdo_photo_linearise(vdo_photo* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device, const float T[16],
                                   double sums[28], int64_t counts[5]) {
  static const char* who = "vdo_photo_linearise";
  const int rc = ph_check_images(who, h, depth, depth_stride_floats, mask, mask_stride_ints);
  if (rc != VDO_OK) return rc;
  return ph_linearise_entry(who, h, true, depth, depth_stride_floats, mask, mask_stride_ints, src_is_device, T, sums, counts);
}

extern "C" int vdo_photo_linearise_frame(vdo_photo* h, const vdo_frame_images* f, const float T[16], double sums[28], int64_t counts[5]) {
  static const char* who = "vdo_photo_linearise_frame";
  const int rc = ph_check_frame(who, h, f);
  if (rc != VDO_OK) return rc;
  return ph_linearise_entry(who, h, false, f->d_depth, h->W, f->d_mask, h->W, 1, T, sums, counts);
}

extern "C" int vdo_photo_solve(vdo_photo* h, vdo_align* geo, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device,
                               double weight, const float T_init[16], float T_out[16], vdo_photo_report* report, double* trace) {
  static const char* who = "vdo_photo_solve";
  const int rc = ph_check_images(who, h, depth, depth_stride_floats, mask, mask_stride_ints);
  if (rc != VDO_OK) return rc;
  return ph_solve_entry(who, h, geo, true, depth, depth_stride_floats, mask, mask_stride_ints, src_is_device, weight, T_init, T_out, report, trace);
}

extern "C" int vdo_photo_solve_frame(vdo_photo* h, vdo_align* geo, const vdo_frame_images* f, double weight, const float T_init[16], float T_out[16], vdo_photo_report* report,
                                     double* trace) {
  static const char* who = "vdo_photo_solve_frame";
  const int rc = ph_check_frame(who, h, f);
  if (rc != VDO_OK) return rc;
  return ph_solve_entry(who, h, geo, false, f->d_depth, h->W, f->d_mask, h->W, 1, weight, T_init, T_out, report, trace);
}

extern "C" int vdo_photo_get_rows(vdo_photo* h, float* rows) {
  static const char* who = "vdo_photo_get_rows";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!rows) return set_error(VDO_ERR_INVALID, "%s: rows is null", who);
  if (!h->d_rows) return set_error(VDO_ERR_INVALID, "%s: the handle was made without keep_rows", who);
  if (!h->has_rows) return set_error(VDO_ERR_INVALID, "%s: no linearisation yet", who);
  const int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipMemcpyAsync(rows, h->d_rows, (size_t)h->Ws * h->Hs * 8 * sizeof(float), hipMemcpyDeviceToHost, h->ctx->stream);
  return check_hip(who, hipStreamSynchronize(h->ctx->stream));
}

extern "C" int vdo_photo_last_timing(vdo_photo* h, double ms[2]) {
  return last_timing("vdo_photo_last_timing", h ? &h->tm : nullptr, ms);
}
