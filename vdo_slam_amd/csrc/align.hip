// Aligner: point-to-plane ICP of a measured depth frame against a view of the dense map (raycast.hip) - projective data association, one 6-vector
// Jacobian row per sample, the 28 sums of the normal equations over the image, and a Gauss-Newton step on the host.  The semantics are this
// library's own, stated in include/vdo_slam_hip.h ("Aligner") and restated in NumPy by tests/align_ref.py.  The rows are fp32 with one rounded
// operation per step in the header's order (the library is built with -ffp-contract=off; / and floorf are correctly rounded); the terms are exact
// products in double; every sum is ONE fixed adjacent-pair tree over the slot vector, so that no bit depends on the launch shape or the schedule.
//
//   k_al_rows<ROWS>  one thread per sample, one wave per 8 x 8 sample tile (lane = slot within the tile), four consecutive tiles per workgroup.  A
//                    skipped sample has J = e = w = 0 and so contributes +0.0 everywhere.  Per lane 32 doubles: the 28 terms and four of the five
//                    counts as 0.0 / 1.0 (integers below 2^53 add exactly in any order; the fifth count is what is left of Ws*Hs).  The wave's
//                    xor-butterfly over masks 1 .. 32 is the first six levels of the tree; it is done TRANSPOSING - at mask m a lane keeps the half
//                    of its values its bit of m selects and sends the other half, 16 + 8 + 4 + 2 + 1 + 1 = 32 exchanges of a double, not 32 x 6 -,
//                    which leaves lane l < 32 with the tile's sum of the value whose index is l's five bits reversed.  256 bytes per tile.
//   k_al_tree        pt_tree of pair_tree.hpp: eight levels over 256 consecutive nodes per workgroup, launched until one node is left.
//
// NO OUT-OF-RANGE ACCESS: the one gathered address of the model comes from float compares against 0 and Wm - 1 / Hm - 1 made before any conversion to
// int (a NaN fails them); the frame is read at (i * s, j * s) with i < Ws, j < Hs; a partial is written at tile < tiles, a row at a sample of the grid.
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

constexpr int kAlTerms = 28;
constexpr int kAlVals = kPtVals;                                           // the 28 terms, then used, masked, no model, far as doubles
constexpr int kAlSpan = kPtSpan;                                           // nodes per workgroup of k_al_tree

// what the kernels take by value
struct AlArgs {
  float fx, fy, cx, cy, min_d, max_d, max_dist2;
  int W, s, Ws, Hs, tiles_x, tiles;
  float T[12];
  float fxm, fym, cxm, cym, xmax, ymax;                                    // xmax = (float)(Wm - 1), ymax = (float)(Hm - 1)
  int Wm;
  float Tm[12], c[3], Rm[9];                                               // the model's pose, its camera centre, Rm[3 * i + a] = Tm(i, a)
};

enum { kAlUsed = 0, kAlNoDepth, kAlMasked, kAlNoModel, kAlFar };

// one sample in the header's order: its class, and J, e, w when it is used
__device__ __forceinline__ int al_sample(const AlArgs& a, int x, int y, const float* __restrict__ depth, const int32_t* __restrict__ mask, const float* __restrict__ mdepth,
                                         const float* __restrict__ mgrad, float J[6], float* e_out, float* w_out) {
  const size_t at = (size_t)y * a.W + x;
  const float d = depth[at];
  if (!(dn_finite(d) && d > a.min_d && d <= a.max_d)) return kAlNoDepth;
  if (mask && mask[at] != 0) return kAlMasked;
  const float dx = ((float)x - a.cx) / a.fx, dy = ((float)y - a.cy) / a.fy;
  const float Pc[3] = {dx * d, dy * d, d};
  const float q[3] = {Pc[0] - a.T[3], Pc[1] - a.T[7], Pc[2] - a.T[11]};
  float Pw[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) Pw[k] = (a.T[k] * q[0] + a.T[4 + k] * q[1]) + a.T[8 + k] * q[2];
  const float Xm = (a.Tm[0] * Pw[0] + a.Tm[1] * Pw[1]) + (a.Tm[2] * Pw[2] + a.Tm[3]);
  const float Ym = (a.Tm[4] * Pw[0] + a.Tm[5] * Pw[1]) + (a.Tm[6] * Pw[2] + a.Tm[7]);
  const float Zm = (a.Tm[8] * Pw[0] + a.Tm[9] * Pw[1]) + (a.Tm[10] * Pw[2] + a.Tm[11]);
  if (!(dn_finite(Zm) && Zm > FLT_MIN)) return kAlNoModel;
  const float u = (a.fxm * Xm) / Zm + a.cxm, v = (a.fym * Ym) / Zm + a.cym;
  const float xq = floorf(u + 0.5f), yq = floorf(v + 0.5f);
  if (!(dn_finite(u) && dn_finite(v) && xq >= 0.f && xq <= a.xmax && yq >= 0.f && yq <= a.ymax)) return kAlNoModel;
  const size_t m = (size_t)(int)yq * a.Wm + (int)xq;
  const float dm = mdepth[m];
  const float g[3] = {mgrad[3 * m], mgrad[3 * m + 1], mgrad[3 * m + 2]};
  const float gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
  if (!(dn_finite(dm) && dm > 0.f && dn_finite(gg) && gg > 0.f)) return kAlNoModel;
  float r[3], del[3];
  dn_ray(xq, yq, a.fxm, a.fym, a.cxm, a.cym, a.Rm, r);
#pragma unroll
  for (int k = 0; k < 3; ++k) del[k] = Pw[k] - (a.c[k] + dm * r[k]);
  const float dist2 = (del[0] * del[0] + del[1] * del[1]) + del[2] * del[2];
  if (!(dist2 <= a.max_dist2)) return kAlFar;
  *e_out = (g[0] * del[0] + g[1] * del[1]) + g[2] * del[2];
  *w_out = 1.0f / gg;
  float gc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) gc[k] = (a.T[4 * k] * g[0] + a.T[4 * k + 1] * g[1]) + a.T[4 * k + 2] * g[2];
  J[0] = gc[0]; J[1] = gc[1]; J[2] = gc[2];
  J[3] = Pc[1] * gc[2] - Pc[2] * gc[1];
  J[4] = Pc[2] * gc[0] - Pc[0] * gc[2];
  J[5] = Pc[0] * gc[1] - Pc[1] * gc[0];
  return kAlUsed;
}

template <bool ROWS>
__global__ __launch_bounds__(256) void k_al_rows(AlArgs a, const float* __restrict__ depth, const int32_t* __restrict__ mask, const float* __restrict__ mdepth,
                                                 const float* __restrict__ mgrad, double* __restrict__ part, float* __restrict__ rows) {
  const int lane = threadIdx.x, tile = (int)blockIdx.x * 4 + (int)threadIdx.y;
  if (tile >= a.tiles) return;                                             // the whole wave leaves: nothing below waits for another wave
  const int i = (tile % a.tiles_x) * 8 + (lane & 7), j = (tile / a.tiles_x) * 8 + (lane >> 3);
  float J[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, e = 0.f, w = 0.f;
  int cls = -1;
  if (i < a.Ws && j < a.Hs) {
    float Jt[6], et = 0.f, wt = 0.f;
    cls = al_sample(a, i * a.s, j * a.s, depth, mask, mdepth, mgrad, Jt, &et, &wt);
    if (cls == kAlUsed) {
#pragma unroll
      for (int k = 0; k < 6; ++k) J[k] = Jt[k];
      e = et; w = wt;
    }
    if (ROWS) {
      float4* o = reinterpret_cast<float4*>(rows + ((size_t)j * a.Ws + i) * 8);
      o[0] = make_float4(J[0], J[1], J[2], J[3]);
      o[1] = make_float4(J[4], J[5], e, w);
    }
  }
  double v[kAlVals];
  {
    double h[6], Jd[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { h[k] = (double)(w * J[k]); Jd[k] = (double)J[k]; }
    int t = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) v[t++] = h[r] * Jd[c];
#pragma unroll
    for (int r = 0; r < 6; ++r) v[21 + r] = h[r] * (double)e;
    v[27] = (double)(w * e) * (double)e;
    v[28] = cls == kAlUsed ? 1.0 : 0.0; v[29] = cls == kAlMasked ? 1.0 : 0.0; v[30] = cls == kAlNoModel ? 1.0 : 0.0; v[31] = cls == kAlFar ? 1.0 : 0.0;
  }
  // the first six levels: at mask m the lane with the bit clear keeps the lower half of its values, its partner the upper half
#pragma unroll
  for (int m = 1, n = kAlVals / 2; m <= 16; m <<= 1, n >>= 1) {
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
    part[(size_t)tile * kAlVals + idx] = v[0];
  }
}

// Eight levels of the tree over the nodes [256 * block, 256 * block + 256) of every value: in [n_real][32] (a node >= n_real holds +0.0), P the
// padded node count (a power of two >= n_real), out [max(P / 256, 1)][32].  A pair whose second node lies beyond P's level does not exist.
__global__ __launch_bounds__(256) void k_al_tree(const double* __restrict__ in, int n_real, int P, double* __restrict__ out) {
  __shared__ double lds[8][kAlVals];
  pt_tree(in, n_real, P, out, lds);
}

}  // namespace vdo

struct vdo_align {
  vdo_ctx* ctx = nullptr;
  int W = 0, H = 0, Ws = 0, Hs = 0;
  vdo_align_params p{};
  vdo::AlArgs a{};
  size_t npix = 0;
  bool has_model = false, has_rows = false;
  const float* m_depth = nullptr;                         // the model in use: the handle's images or borrowed ones
  const float* m_grad = nullptr;
  float* d_depth = nullptr;                               // [H][W] staging
  int32_t* d_mask = nullptr;                              // [H][W] staging
  float* d_mdepth = nullptr;                              // [npix] the model images the handle owns
  float* d_mgrad = nullptr;                               // [npix][3]
  double* d_part[2] = {nullptr, nullptr};                 // [tiles][32] the tile partials; [max(P / 256, 1)][32] the level above; then in turns
  float* d_rows = nullptr;                                // [Hs][Ws][8] with keep_rows
  double* h_sums = nullptr;                               // pinned, [32]
  vdo::StageTimer tm;
};

using namespace vdo;

void vdo::al_info(const vdo_align* h, int* W, int* H, int* min_pixels, bool* has_model, vdo_ctx** ctx) {
  *W = h->W; *H = h->H; *min_pixels = h->p.min_pixels; *has_model = h->has_model; *ctx = h->ctx;
}

static void al_free(vdo_align* h) {
  hipFree(h->d_depth); hipFree(h->d_mask); hipFree(h->d_mdepth); hipFree(h->d_mgrad); hipFree(h->d_part[0]); hipFree(h->d_part[1]); hipFree(h->d_rows);
  if (h->h_sums) hipHostFree(h->h_sums);
  h->tm.destroy();
  delete h;
}

extern "C" int vdo_align_create(vdo_ctx* ctx, int width, int height, const vdo_align_params* p, vdo_align** out) {
  static const char* who = "vdo_align_create";
  if (!ctx) return set_error(VDO_ERR_INVALID, "%s: ctx is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (!p) return set_error(VDO_ERR_INVALID, "%s: params is null", who);
  if (width < 1) return set_error(VDO_ERR_INVALID, "%s: width %d < 1", who, width);
  if (height < 1) return set_error(VDO_ERR_INVALID, "%s: height %d < 1", who, height);
  int rc = check_intrinsics(who, "K", p->K);
  if (rc == VDO_OK) rc = check_depth_range(who, p->min_depth, p->max_depth);
  if (rc != VDO_OK) return rc;
  if (!is_finite(p->max_dist) || !(p->max_dist > 0.f)) return set_error(VDO_ERR_INVALID, "%s: max_dist %g must be positive and finite", who, (double)p->max_dist);
  if (p->subsample < 1 || p->subsample > 8) return set_error(VDO_ERR_INVALID, "%s: subsample %d outside 1..8", who, p->subsample);
  if (p->min_pixels < 6) return set_error(VDO_ERR_INVALID, "%s: min_pixels %d < 6", who, p->min_pixels);
  if (p->max_iterations < 1 || p->max_iterations > 64) return set_error(VDO_ERR_INVALID, "%s: max_iterations %d outside 1..64", who, p->max_iterations);
  if (!is_finite(p->eps) || !(p->eps >= 0.f)) return set_error(VDO_ERR_INVALID, "%s: eps %g must be finite and >= 0", who, (double)p->eps);
  if (p->keep_rows != 0 && p->keep_rows != 1) return set_error(VDO_ERR_INVALID, "%s: keep_rows %d not 0 or 1", who, p->keep_rows);
  rc = check_image_size(who, "width x height =", width, height);
  if (rc == VDO_OK) rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  vdo_align* h = new vdo_align;
  h->ctx = ctx; h->W = width; h->H = height; h->p = *p;
  const int s = p->subsample;
  h->Ws = (width + s - 1) / s; h->Hs = (height + s - 1) / s;
  AlArgs& a = h->a;
  a.fx = p->K[0]; a.fy = p->K[1]; a.cx = p->K[2]; a.cy = p->K[3];
  a.min_d = p->min_depth > 0.f ? p->min_depth : 0.f; a.max_d = p->max_depth; a.max_dist2 = p->max_dist * p->max_dist;
  a.W = width; a.s = s; a.Ws = h->Ws; a.Hs = h->Hs; a.tiles_x = (h->Ws + 7) / 8; a.tiles = a.tiles_x * ((h->Hs + 7) / 8);
  h->npix = (size_t)width * height;
  const size_t n1 = (size_t)(pt_pow2(a.tiles) / kAlSpan > 1 ? pt_pow2(a.tiles) / kAlSpan : 1);
  bool ok = hipMalloc((void**)&h->d_depth, h->npix * sizeof(float)) == hipSuccess && hipMalloc((void**)&h->d_mask, h->npix * sizeof(int32_t)) == hipSuccess &&
            hipMalloc((void**)&h->d_mdepth, h->npix * sizeof(float)) == hipSuccess && hipMalloc((void**)&h->d_mgrad, h->npix * 3 * sizeof(float)) == hipSuccess &&
            hipMalloc((void**)&h->d_part[0], (size_t)a.tiles * kAlVals * sizeof(double)) == hipSuccess && hipMalloc((void**)&h->d_part[1], n1 * kAlVals * sizeof(double)) == hipSuccess &&
            hipHostMalloc((void**)&h->h_sums, kAlVals * sizeof(double), hipHostMallocDefault) == hipSuccess && h->tm.create();
  if (ok && p->keep_rows) ok = hipMalloc((void**)&h->d_rows, (size_t)h->Ws * h->Hs * 8 * sizeof(float)) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    al_free(h);
    return set_error(VDO_ERR_OOM, "%s: device allocation failed for %d x %d images", who, width, height);
  }
  *out = h;
  return VDO_OK;
}

extern "C" int vdo_align_destroy(vdo_align* h) {
  if (!h) return VDO_OK;
  if (ctx_bind(h->ctx) == VDO_OK) hipStreamSynchronize(h->ctx->stream);
  al_free(h);
  return VDO_OK;
}

// the model's intrinsics, size and pose into the kernel arguments
static void al_take_model(vdo_align* h, const float* depth, const float* grad, int Wm, int Hm, const float Km[4], const float Tm[16]) {
  AlArgs& a = h->a;
  a.fxm = Km[0]; a.fym = Km[1]; a.cxm = Km[2]; a.cym = Km[3]; a.xmax = (float)(Wm - 1); a.ymax = (float)(Hm - 1); a.Wm = Wm;
  for (int k = 0; k < 12; ++k) a.Tm[k] = Tm[k];
  dn_centre(Tm, a.c);
  for (int k = 0; k < 3; ++k) { a.Rm[k] = Tm[k]; a.Rm[3 + k] = Tm[4 + k]; a.Rm[6 + k] = Tm[8 + k]; }
  h->m_depth = depth; h->m_grad = grad; h->has_model = true;
}

extern "C" int vdo_align_set_model(vdo_align* h, const float* depth, const float* grad, int Wm, int Hm, const float Km[4], const float Tm[16], int is_device) {
  static const char* who = "vdo_align_set_model";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!depth) return set_error(VDO_ERR_INVALID, "%s: depth is null", who);
  if (!grad) return set_error(VDO_ERR_INVALID, "%s: grad is null", who);
  if (!Km) return set_error(VDO_ERR_INVALID, "%s: Km is null", who);
  if (!Tm) return set_error(VDO_ERR_INVALID, "%s: Tm is null", who);
  if (Wm < 1) return set_error(VDO_ERR_INVALID, "%s: model_width %d < 1", who, Wm);
  if (Hm < 1) return set_error(VDO_ERR_INVALID, "%s: model_height %d < 1", who, Hm);
  int rc = check_intrinsics(who, "Km", Km);
  if (rc == VDO_OK) rc = check_image_size(who, "the model of", Wm, Hm);
  if (rc != VDO_OK) return rc;
  if (!is_device) {
    const size_t nm = (size_t)Wm * Hm;
    if (nm > h->npix) return set_error(VDO_ERR_UNSUPPORTED, "%s: a host model of %d x %d has more pixels than the %d x %d frame the handle's model images were sized for", who, Wm, Hm, h->W, h->H);
    rc = ctx_bind(h->ctx);
    if (rc != VDO_OK) return rc;
    hipStream_t s = h->ctx->stream;
    hipMemcpyAsync(h->d_mdepth, depth, nm * sizeof(float), hipMemcpyHostToDevice, s);
    hipMemcpyAsync(h->d_mgrad, grad, nm * 3 * sizeof(float), hipMemcpyHostToDevice, s);
    rc = sync_check(who, s);
    if (rc != VDO_OK) { h->has_model = false; return rc; }
    depth = h->d_mdepth; grad = h->d_mgrad;
  }
  al_take_model(h, depth, grad, Wm, Hm, Km, Tm);
  return VDO_OK;
}

extern "C" int vdo_align_set_model_from_view(vdo_align* h, vdo_raycast* view, const float Tm[16], int64_t counts[3]) {
  static const char* who = "vdo_align_set_model_from_view";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!view) return set_error(VDO_ERR_INVALID, "%s: view is null", who);
  if (!Tm) return set_error(VDO_ERR_INVALID, "%s: Tm is null", who);
  int Wm = 0, Hm = 0;
  float Km[4];
  vdo_ctx* vctx = nullptr;
  rc_view_info(view, &Wm, &Hm, Km, &vctx);
  if (vctx->device != h->ctx->device) return set_error(VDO_ERR_INVALID, "%s: view lives on device %d, the aligner on device %d", who, vctx->device, h->ctx->device);
  if ((size_t)Wm * Hm > h->npix) return set_error(VDO_ERR_UNSUPPORTED, "%s: the view of %d x %d has more pixels than the %d x %d frame the handle's model images were sized for", who, Wm, Hm, h->W, h->H);
  int64_t out[3] = {0, 0, 0};
  const int rc = vdo_raycast_render(view, Tm, h->d_mdepth, h->d_mgrad, nullptr, 1, out);      // host-synchronous on the view's stream: the images are complete
  if (rc != VDO_OK) { h->has_model = false; return rc; }
  al_take_model(h, h->d_mdepth, h->d_mgrad, Wm, Hm, Km, Tm);
  if (counts) for (int k = 0; k < 3; ++k) counts[k] = out[k];
  return VDO_OK;
}

namespace vdo {

// where a call's depth and mask lie on the device once al_stage has queued the copies
struct AlSrc { const float* depth; const int32_t* mask; };

static AlSrc al_stage(vdo_align* h, const float* depth, int64_t dstride, const int32_t* mask, int64_t mstride, int src_is_device) {
  hipStream_t s = h->ctx->stream;
  return AlSrc{stage_rows(s, h->d_depth, depth, dstride, h->W, h->H, src_is_device), mask ? stage_rows(s, h->d_mask, mask, mstride, h->W, h->H, src_is_device) : nullptr};
}

// one linearisation of packed device images at T: the launches, the download of the 32 values; *dev_ms the device time from ev0 (recorded by the caller)
static int al_linearise(const char* who, vdo_align* h, AlSrc src, const float T[16], double sums[28], int64_t counts[5], double* dev_ms) {
  hipStream_t s = h->ctx->stream;
  AlArgs a = h->a;
  for (int k = 0; k < 12; ++k) a.T[k] = T[k];
  const dim3 grid((unsigned)((a.tiles + 3) / 4)), block(64, 4);
  if (h->d_rows) hipLaunchKernelGGL(k_al_rows<true>, grid, block, 0, s, a, src.depth, src.mask, h->m_depth, h->m_grad, h->d_part[0], h->d_rows);
  else hipLaunchKernelGGL(k_al_rows<false>, grid, block, 0, s, a, src.depth, src.mask, h->m_depth, h->m_grad, h->d_part[0], (float*)nullptr);
  int n = a.tiles, P = pt_pow2(a.tiles), from = 0;
  do {
    const int blocks = P / kAlSpan > 1 ? P / kAlSpan : 1;
    hipLaunchKernelGGL(k_al_tree, dim3((unsigned)blocks), dim3(256), 0, s, (const double*)h->d_part[from], n, P, h->d_part[from ^ 1]);
    n = P = blocks;
    from ^= 1;
  } while (P > 1);
  h->tm.mark_end(s);
  hipMemcpyAsync(h->h_sums, h->d_part[from], kAlVals * sizeof(double), hipMemcpyDeviceToHost, s);
  const int rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  h->has_rows = h->d_rows != nullptr;
  for (int k = 0; k < kAlTerms; ++k) sums[k] = h->h_sums[k];
  counts[kAlUsed] = (int64_t)h->h_sums[28]; counts[kAlMasked] = (int64_t)h->h_sums[29]; counts[kAlNoModel] = (int64_t)h->h_sums[30]; counts[kAlFar] = (int64_t)h->h_sums[31];
  counts[kAlNoDepth] = (int64_t)h->Ws * h->Hs - counts[kAlUsed] - counts[kAlMasked] - counts[kAlNoModel] - counts[kAlFar];
  *dev_ms = elapsed_ms(h->tm.ev0, h->tm.ev1);
  return VDO_OK;
}

static int al_check_images(const char* who, vdo_align* h, const float* depth, int64_t dstride, const int32_t* mask, int64_t mstride) {
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  return check_depth_mask(who, h->W, depth, dstride, mask, mstride, false);
}

static int al_check_frame(const char* who, vdo_align* h, const vdo_frame_images* f) {
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  return check_frame(who, f, h->W, h->H, "the aligner's");
}

// the two linearise entries after their own checks; staged: the images go through al_stage
static int al_linearise_entry(const char* who, vdo_align* h, bool staged, const float* depth, int64_t dstride, const int32_t* mask, int64_t mstride, int src_is_device, const float T[16],
                              double sums[28], int64_t counts[5]) {
  if (!T) return set_error(VDO_ERR_INVALID, "%s: T is null", who);
  if (!sums) return set_error(VDO_ERR_INVALID, "%s: sums is null", who);
  if (!counts) return set_error(VDO_ERR_INVALID, "%s: counts is null", who);
  if (!h->has_model) return set_error(VDO_ERR_INVALID, "%s: no model is set", who);
  const int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  const auto t0 = h->tm.begin(h->ctx->stream);
  const AlSrc src = staged ? al_stage(h, depth, dstride, mask, mstride, src_is_device) : AlSrc{depth, mask};
  double s28[28], dev_ms = 0;
  int64_t c5[5];
  const int rl = al_linearise(who, h, src, T, s28, c5, &dev_ms);
  if (rl != VDO_OK) return rl;
  std::memcpy(sums, s28, sizeof s28); std::memcpy(counts, c5, sizeof c5);
  h->tm.finish(t0, dev_ms);
  return VDO_OK;
}

// the two solve entries after their own checks
static int al_solve_entry(const char* who, vdo_align* h, bool staged, const float* depth, int64_t dstride, const int32_t* mask, int64_t mstride, int src_is_device, const float T_init[16],
                          float T_out[16], vdo_align_report* report, double* trace) {
  if (!T_init) return set_error(VDO_ERR_INVALID, "%s: T_init is null", who);
  if (!T_out) return set_error(VDO_ERR_INVALID, "%s: T_out is null", who);
  if (!h->has_model) return set_error(VDO_ERR_INVALID, "%s: no model is set", who);
  const int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  const auto t0 = h->tm.begin(h->ctx->stream);
  const AlSrc src = staged ? al_stage(h, depth, dstride, mask, mstride, src_is_device) : AlSrc{depth, mask};
  float T[16], Tn[16];
  std::memcpy(T, T_init, sizeof T);
  vdo_align_report rep{};
  double dev_total = 0;
  for (int it = 0; it < h->p.max_iterations; ++it) {
    double sums[28], dev_ms = 0, rms = 0;
    int64_t counts[5];
    if (it > 0) hipEventRecord(h->tm.ev0, h->ctx->stream);
    const int rl = al_linearise(who, h, src, T, sums, counts, &dev_ms);
    if (rl != VDO_OK) return rl;
    dev_total += dev_ms;
    if (trace) {
      double* row = trace + (size_t)it * 49;
      for (int k = 0; k < 16; ++k) row[k] = (double)T[k];
      for (int k = 0; k < 28; ++k) row[16 + k] = sums[k];
      for (int k = 0; k < 5; ++k) row[44 + k] = (double)counts[k];
    }
    rep.status = vdo_align_step(sums, counts[0], h->p.min_pixels, T, Tn, rep.xi, &rms);
    rep.iterations = it + 1; rep.used = counts[0]; rep.rms_last = rms;
    if (it == 0) rep.rms_first = rms;
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

extern "C" int vdo_align_linearise(vdo_align* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device, const float T[16],
                                   double sums[28], int64_t counts[5]) {
  static const char* who = "vdo_align_linearise";
  const int rc = al_check_images(who, h, depth, depth_stride_floats, mask, mask_stride_ints);
  if (rc != VDO_OK) return rc;
  return al_linearise_entry(who, h, true, depth, depth_stride_floats, mask, mask_stride_ints, src_is_device, T, sums, counts);
}

extern "C" int vdo_align_linearise_frame(vdo_align* h, const vdo_frame_images* f, const float T[16], double sums[28], int64_t counts[5]) {
  static const char* who = "vdo_align_linearise_frame";
  const int rc = al_check_frame(who, h, f);
  if (rc != VDO_OK) return rc;
  return al_linearise_entry(who, h, false, f->d_depth, h->W, f->d_mask, h->W, 1, T, sums, counts);
}

extern "C" int vdo_align_solve(vdo_align* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device, const float T_init[16],
                               float T_out[16], vdo_align_report* report, double* trace) {
  static const char* who = "vdo_align_solve";
  const int rc = al_check_images(who, h, depth, depth_stride_floats, mask, mask_stride_ints);
  if (rc != VDO_OK) return rc;
  return al_solve_entry(who, h, true, depth, depth_stride_floats, mask, mask_stride_ints, src_is_device, T_init, T_out, report, trace);
}

extern "C" int vdo_align_solve_frame(vdo_align* h, const vdo_frame_images* f, const float T_init[16], float T_out[16], vdo_align_report* report, double* trace) {
  static const char* who = "vdo_align_solve_frame";
  const int rc = al_check_frame(who, h, f);
  if (rc != VDO_OK) return rc;
  return al_solve_entry(who, h, false, f->d_depth, h->W, f->d_mask, h->W, 1, T_init, T_out, report, trace);
}

extern "C" int vdo_align_step(const double sums[28], int64_t used, int64_t min_pixels, const float T[16], float T_out[16], double xi_out[6], double* rms_out) {
  static const char* who = "vdo_align_step";
  if (!sums) return set_error(VDO_ERR_INVALID, "%s: sums is null", who);
  if (!T) return set_error(VDO_ERR_INVALID, "%s: T is null", who);
  if (!T_out) return set_error(VDO_ERR_INVALID, "%s: T_out is null", who);
  float Tin[16];
  std::memcpy(Tin, T, sizeof Tin);                                          // T_out may be T
  double xi[6] = {0, 0, 0, 0, 0, 0};
  auto leave = [&](int status) {
    std::memcpy(T_out, Tin, sizeof Tin);
    if (xi_out) for (int k = 0; k < 6; ++k) xi_out[k] = status == 0 ? xi[k] : 0.0;
    return status;
  };
  if (rms_out) *rms_out = used > 0 ? std::sqrt(sums[27] / (double)used) : 0.0;
  if (used < min_pixels) return leave(1);
  for (int k = 0; k < 28; ++k) if (!std::isfinite(sums[k])) return leave(2);
  double A[6][6], L[6][6] = {}, y[6];
  for (int r = 0, t = 0; r < 6; ++r) for (int c = r; c < 6; ++c, ++t) A[r][c] = A[c][r] = sums[t];
  for (int j = 0; j < 6; ++j) {
    double p = A[j][j];
    for (int k = 0; k < j; ++k) p -= L[j][k] * L[j][k];
    if (!(p > 0.0)) return leave(2);                                        // (a NaN fails too)
    L[j][j] = std::sqrt(p);
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  for (int i = 0; i < 6; ++i) {                                             // L y = -b
    double v = -sums[21 + i];
    for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {                                            // L^T xi = y
    double v = y[i];
    for (int k = i + 1; k < 6; ++k) v -= L[k][i] * xi[k];
    xi[i] = v / L[i][i];
  }
  for (int k = 0; k < 6; ++k) if (!std::isfinite(xi[k])) return leave(2);
  // Exp(-xi): v = -xi[0..3), w = -xi[3..6)
  const double v[3] = {-xi[0], -xi[1], -xi[2]}, w[3] = {-xi[3], -xi[4], -xi[5]};
  const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = std::sqrt(th2);
  double ca, cb, cc;
  if (th < 1e-4) { ca = 1.0 - th2 / 6.0; cb = 0.5 - th2 / 24.0; cc = 1.0 / 6.0 - th2 / 120.0; }
  else { ca = std::sin(th) / th; cb = (1.0 - std::cos(th)) / th2; cc = (th - std::sin(th)) / (th2 * th); }
  const double Wx[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
  double W2[3][3], R[3][3], t[3];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) W2[r][c] = (Wx[r][0] * Wx[0][c] + Wx[r][1] * Wx[1][c]) + Wx[r][2] * Wx[2][c];
  for (int r = 0; r < 3; ++r) {
    double tv = 0;
    for (int c = 0; c < 3; ++c) {
      R[r][c] = (r == c ? 1.0 : 0.0) + ca * Wx[r][c] + cb * W2[r][c];
      tv += ((r == c ? 1.0 : 0.0) + cb * Wx[r][c] + cc * W2[r][c]) * v[c];
    }
    t[r] = tv;
  }
  float Tn[16];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) {
      double s = (R[r][0] * (double)Tin[c] + R[r][1] * (double)Tin[4 + c]) + R[r][2] * (double)Tin[8 + c];
      if (c == 3) s += t[r];
      if (!std::isfinite(s) || !(std::fabs(s) <= (double)FLT_MAX)) return leave(2);
      Tn[4 * r + c] = (float)s;
    }
  Tn[12] = Tn[13] = Tn[14] = 0.f; Tn[15] = 1.f;
  std::memcpy(T_out, Tn, sizeof Tn);
  if (xi_out) for (int k = 0; k < 6; ++k) xi_out[k] = xi[k];
  return 0;
}

extern "C" int vdo_align_get_rows(vdo_align* h, float* rows) {
  static const char* who = "vdo_align_get_rows";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!rows) return set_error(VDO_ERR_INVALID, "%s: rows is null", who);
  if (!h->d_rows) return set_error(VDO_ERR_INVALID, "%s: the handle was made without keep_rows", who);
  if (!h->has_rows) return set_error(VDO_ERR_INVALID, "%s: no linearisation yet", who);
  const int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipMemcpyAsync(rows, h->d_rows, (size_t)h->Ws * h->Hs * 8 * sizeof(float), hipMemcpyDeviceToHost, h->ctx->stream);
  return check_hip(who, hipStreamSynchronize(h->ctx->stream));
}

extern "C" int vdo_align_last_timing(vdo_align* h, double ms[2]) {
  return last_timing("vdo_align_last_timing", h ? &h->tm : nullptr, ms);
}
