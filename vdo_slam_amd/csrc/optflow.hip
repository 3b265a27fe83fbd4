// Dense optical-flow matcher: 2 x 2 mean pyramid, 9 x 7 census per level, coarse-to-fine block search over the census words, 3 x 3 median between
// levels, integer sub-pixel and a forward-backward check - from two 8-bit grey images to the flow[H][W][2] fp32 image FramePipeline::Step takes.  The
// reference consumes such images (a .flo per frame) but its authors made them with an offline network; the semantics are this library's own, stated
// in include/vdo_slam_hip.h (vdo_optflow_compute) and restated in NumPy by tests/optflow_ref.py.  Integer arithmetic end to end: the only fp32
// operation is the conversion of the result.
//
//   k_flow_pyramid   one workgroup per 64 x 64 region of level 0 and image: the region is self-contained down to level 6 (a 2 x 2 block never
//                    straddles a multiple of 64 >> l), so ALL levels of both images come from one launch through two LDS buffers.
//   k_flow_census    every level of both images in one launch; the tile is census.hpp's, shared with stereo.hip.
//   k_flow_search    the hot kernel, one launch per level, both directions in it (blockIdx.z): one thread per pixel, 32 x 8 pixels per workgroup, the
//                    (2r+1)^2 block sums in registers (templated on r: every index is static, nothing spills).  The c0 block comes from an LDS tile
//                    with a 4 pixel halo; the c1 words are a gather around (x + u0, y + v0), walked row by row: each of the (2w+2r+1)^2 words is loaded
//                    once into a register row and feeds every accumulator it belongs to.  Argmin by the packed key (A << 8) | k, and at level 0 the
//                    sub-pixel offsets and the fp32 output, fused.
//   k_flow_median    3 x 3 median of a level's flow (levels >= 1), both directions in one launch.
//   k_flow_check     forward-backward check, validity image and the count of valid pixels (wave ballot, one integer atomic per wave).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vdo_slam_hip.h"
#include "census.hpp"
#include "ctx.hpp"
#include "stage.hpp"

namespace vdo {

constexpr int kFlowMaxLevels = 7;
constexpr int kFlowTX = 32, kFlowTY = 8;                // pixels per search workgroup
constexpr int kFlowHalo = 4;                            // the largest window
constexpr int kFlowRegion = 64;                         // level-0 pixels per pyramid workgroup and axis: 2^(kFlowMaxLevels - 1)
constexpr int64_t kFlowMaxPixels = int64_t(1) << 26;

struct FlowGeom {                                       // of one image; the second image's arrays lie `tot` elements behind the first's
  int L, tot;
  int W[kFlowMaxLevels], H[kFlowMaxLevels], off[kFlowMaxLevels];
  int tiles_x[kFlowMaxLevels], tile0[kFlowMaxLevels + 1];      // census tiles
};

}  // namespace vdo

struct vdo_optflow {
  vdo_ctx* ctx = nullptr;
  int W = 0, H = 0;
  vdo_optflow_params p{};
  vdo::FlowGeom g{};
  uint8_t* d_pyr = nullptr;                             // [2][tot]: level 0 is the packed image
  uint64_t* d_census = nullptr;                         // [2][tot]
  int2* d_level_flow = nullptr;                         // [2 directions][tot], as the level below reads them
  int2* d_raw = nullptr;                                // [2][W_1 * H_1]: a level's flow before its median
  float* d_flow = nullptr;                              // [H][W][2]
  uint8_t* d_valid = nullptr;                           // [H][W]
  int* d_count = nullptr;
  int* h_count = nullptr;                               // pinned
  int32_t* d_mask = nullptr;                            // vdo_optflow_stage_mask, made on first use
  vdo::StageTimer tm;
  bool computed = false;
};

namespace vdo {

__global__ __launch_bounds__(256) void k_flow_pyramid(uint8_t* __restrict__ pyr, FlowGeom G) {
  __shared__ uint8_t buf[2][kFlowRegion * kFlowRegion];
  uint8_t* img = pyr + (size_t)blockIdx.z * G.tot;
  int x0 = blockIdx.x * kFlowRegion, y0 = blockIdx.y * kFlowRegion;
  int wp = min(kFlowRegion, G.W[0] - x0), hp = min(kFlowRegion, G.H[0] - y0);       // the region's valid extent at the level below
  for (int i = threadIdx.x; i < wp * hp; i += 256) { const int yy = i / wp, xx = i - yy * wp; buf[0][yy * kFlowRegion + xx] = img[(size_t)(y0 + yy) * G.W[0] + x0 + xx]; }
  __syncthreads();
  int sp = kFlowRegion;                                 // row pitch of the level below in its buffer
  for (int l = 1; l < G.L; ++l) {
    const uint8_t* src = buf[(l - 1) & 1];
    uint8_t* dst = buf[l & 1];
    x0 >>= 1; y0 >>= 1;
    const int n = kFlowRegion >> l, wl = min(n, G.W[l] - x0), hl = min(n, G.H[l] - y0);
    uint8_t* out = img + G.off[l];
    for (int i = threadIdx.x; i < wl * hl; i += 256) {
      const int yy = i / wl, xx = i - yy * wl;
      const int xa = 2 * xx, xb = min(xa + 1, wp - 1), ya = 2 * yy, yb = min(ya + 1, hp - 1);
      const int v = (src[ya * sp + xa] + src[ya * sp + xb] + src[yb * sp + xa] + src[yb * sp + xb] + 2) >> 2;
      dst[yy * n + xx] = (uint8_t)v;
      out[(size_t)(y0 + yy) * G.W[l] + x0 + xx] = (uint8_t)v;
    }
    __syncthreads();
    wp = wl; hp = hl; sp = n;
  }
}

__global__ __launch_bounds__(256) void k_flow_census(const uint8_t* __restrict__ pyr, FlowGeom G, uint64_t* __restrict__ census) {
  const int tiles = G.tile0[G.L];
  const int which = blockIdx.x / tiles;
  int t = blockIdx.x % tiles, l = 0;
  while (l + 1 < G.L && t >= G.tile0[l + 1]) ++l;
  t -= G.tile0[l];
  const size_t base = (size_t)which * G.tot + G.off[l];
  census_tile(pyr + base, G.W[l], G.W[l], G.H[l], (t % G.tiles_x[l]) * kCensusTX, (t / G.tiles_x[l]) * kCensusTY, census + base);
}

// rank of (du, dv) among the candidates of radius r in ascending (du^2 + dv^2, dv, du); folds to a constant where the arguments are
__device__ __forceinline__ constexpr int flow_rank(int r, int du, int dv) {
  int k = 0;
  const int d = du * du + dv * dv;
  for (int b = -r; b <= r; ++b)
    for (int a = -r; a <= r; ++a) {
      const int e = a * a + b * b;
      if (e < d || (e == d && (b < dv || (b == dv && a < du)))) ++k;
    }
  return k;
}

__device__ __forceinline__ int flow_subpixel(int am, int a0, int ap) {
  const int den = am + ap - 2 * a0;
  if (den <= 0) return 0;
  const int num = 128 * (am - ap);
  const int mag = (2 * abs(num) + den) / (2 * den);
  return num < 0 ? -mag : mag;
}

// One level, both directions (blockIdx.z; direction 1 swaps the census images).  census: [2][tot], the level at `off`.  prior: the flows of the level
// above (null at the coarsest level), direction d at prior + d * prior_stride, rows of Wup.  out: direction d at out + d * out_stride, rows of W.
// flow: the fp32 output of direction 0 (level 0 only, else null).
template <int R>
__global__ __launch_bounds__(256) void k_flow_search(const uint64_t* __restrict__ census, int tot, int off, int W, int H, int w, const int2* __restrict__ prior,
                                                     int prior_stride, int Wup, int2* __restrict__ out, int out_stride, int subpixel, float2* __restrict__ flow) {
  constexpr int N = 2 * R + 1, TW = kFlowTX + 2 * kFlowHalo, TH = kFlowTY + 2 * kFlowHalo, ROW = 2 * kFlowHalo + N;
  __shared__ uint64_t tile[TH][TW];
  const int dir = blockIdx.z;
  const uint64_t* __restrict__ c0 = census + (size_t)dir * tot + off;
  const uint64_t* __restrict__ c1 = census + (size_t)(1 - dir) * tot + off;
  const int x0 = blockIdx.x * kFlowTX, y0 = blockIdx.y * kFlowTY;
  for (int i = threadIdx.x; i < TH * TW; i += 256) {
    const int r = i / TW, c = i - r * TW;
    const int gx = min(max(x0 + c - kFlowHalo, 0), W - 1), gy = min(max(y0 + r - kFlowHalo, 0), H - 1);
    tile[r][c] = c0[(size_t)gy * W + gx];
  }
  __syncthreads();
  const int tx = threadIdx.x % kFlowTX, ty = threadIdx.x / kFlowTX;
  const int x = x0 + tx, y = y0 + ty;
  const int xc = min(x, W - 1), yc = min(y, H - 1);     // threads past the image work on its last pixel and store nothing
  int u0 = 0, v0 = 0;
  if (prior) {
    const int2 p = prior[(size_t)dir * prior_stride + (size_t)(yc >> 1) * Wup + (xc >> 1)];
    u0 = 2 * p.x; v0 = 2 * p.y;
  }
  int acc[N][N];
#pragma unroll
  for (int b = 0; b < N; ++b)
#pragma unroll
    for (int a = 0; a < N; ++a) acc[b][a] = 0;
  const int reach = w + R;
  for (int py = -reach; py <= reach; ++py) {            // one row of the c1 patch: each word is loaded once
    const uint64_t* __restrict__ rowp = c1 + (size_t)min(max(yc + v0 + py, 0), H - 1) * W;
    uint64_t c1row[ROW];
#pragma unroll
    for (int t = 0; t < ROW; ++t) {
      const int px = t - (kFlowHalo + R);
      c1row[t] = (px >= -reach && px <= reach) ? rowp[min(max(xc + u0 + px, 0), W - 1)] : 0;
    }
#pragma unroll
    for (int b = 0; b < N; ++b) {                       // dv = b - R: the window row this patch row is for that candidate
      const int j = py - (b - R);
      if (j < -w || j > w) continue;                    // (uniform)
#pragma unroll
      for (int ii = 0; ii <= 2 * kFlowHalo; ++ii) {
        if (ii - kFlowHalo < -w || ii - kFlowHalo > w) continue;       // (uniform)
        const uint64_t c = tile[ty + kFlowHalo + j][tx + ii];
#pragma unroll
        for (int a = 0; a < N; ++a) acc[b][a] += __popcll(c ^ c1row[ii + a]);      // patch column i + du: index (i + 4) + (du + R)
      }
    }
  }
  uint32_t best = ~0u;
  int bdu = 0, bdv = 0;
#pragma unroll
  for (int b = 0; b < N; ++b)
#pragma unroll
    for (int a = 0; a < N; ++a) {
      const uint32_t key = ((uint32_t)acc[b][a] << 8) | (uint32_t)flow_rank(R, a - R, b - R);
      if (key < best) { best = key; bdu = a - R; bdv = b - R; }
    }
  if (x >= W || y >= H) return;
  const int u = u0 + bdu, v = v0 + bdv;
  out[(size_t)dir * out_stride + (size_t)y * W + x] = make_int2(u, v);
  if (flow && dir == 0) {
    int offu = 0, offv = 0;
    if (subpixel) {
      const int a0 = (int)(best >> 8);
      int um = 0, up = 0, vm = 0, vp = 0;
#pragma unroll
      for (int b = 0; b < N; ++b)
#pragma unroll
        for (int a = 0; a < N; ++a) {
          const int du = a - R, dv = b - R;
          if (dv == bdv && du == bdu - 1) um = acc[b][a];
          if (dv == bdv && du == bdu + 1) up = acc[b][a];
          if (du == bdu && dv == bdv - 1) vm = acc[b][a];
          if (du == bdu && dv == bdv + 1) vp = acc[b][a];
        }
      if (abs(bdu) < R) offu = flow_subpixel(um, a0, up);
      if (abs(bdv) < R) offv = flow_subpixel(vm, a0, vp);
    }
    flow[(size_t)y * W + x] = make_float2((float)(256 * u + offu) * (1.f / 256.f), (float)(256 * v + offv) * (1.f / 256.f));
  }
}

__device__ __forceinline__ void sort2(int& a, int& b) { const int lo = min(a, b); b = max(a, b); a = lo; }

// the fifth of nine (Paeth's 19-exchange median network)
__device__ __forceinline__ int median9(int p0, int p1, int p2, int p3, int p4, int p5, int p6, int p7, int p8) {
  sort2(p1, p2); sort2(p4, p5); sort2(p7, p8); sort2(p0, p1); sort2(p3, p4); sort2(p6, p7); sort2(p1, p2); sort2(p4, p5); sort2(p7, p8);
  sort2(p0, p3); sort2(p5, p8); sort2(p4, p7); sort2(p3, p6); sort2(p1, p4); sort2(p2, p5); sort2(p4, p7); sort2(p4, p2); sort2(p6, p4); sort2(p4, p2);
  return p4;
}

__global__ __launch_bounds__(256) void k_flow_median(const int2* __restrict__ in, int in_stride, int W, int H, int2* __restrict__ out, int out_stride) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= W * H) return;
  const int y = pix / W, x = pix - y * W;
  const int2* src = in + (size_t)blockIdx.z * in_stride;
  int us[9], vs[9];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int2 f = src[(size_t)min(max(y + j - 1, 0), H - 1) * W + min(max(x + i - 1, 0), W - 1)];
      us[3 * j + i] = f.x; vs[3 * j + i] = f.y;
    }
  out[(size_t)blockIdx.z * out_stride + pix] = make_int2(median9(us[0], us[1], us[2], us[3], us[4], us[5], us[6], us[7], us[8]),
                                                         median9(vs[0], vs[1], vs[2], vs[3], vs[4], vs[5], vs[6], vs[7], vs[8]));
}

// B null: no check, every pixel is valid.  valid may be null.  A workgroup takes kFlowCheckBatches x 256 consecutive pixels, so that a wave adds the
// ballots of its batches and sends ONE atomic: all of them hit the same counter, and one per 64 pixels was most of this kernel's time.
constexpr int kFlowCheckBatches = 8;
__global__ __launch_bounds__(256) void k_flow_check(const int2* __restrict__ F, const int2* __restrict__ B, int W, int H, int fb_max_diff, uint8_t* __restrict__ valid,
                                                    int* __restrict__ n_valid) {
  int count = 0;                                        // (wave-uniform)
#pragma unroll
  for (int k = 0; k < kFlowCheckBatches; ++k) {
    const int pix = (blockIdx.x * kFlowCheckBatches + k) * 256 + threadIdx.x;
    bool ok = false;
    if (pix < W * H) {
      ok = true;
      if (B) {
        const int y = pix / W, x = pix - y * W;
        const int2 f = F[pix];
        const int xp = x + f.x, yp = y + f.y;
        ok = xp >= 0 && xp < W && yp >= 0 && yp < H;
        if (ok) {
          const int2 b = B[(size_t)yp * W + xp];
          ok = max(abs(f.x + b.x), abs(f.y + b.y)) <= fb_max_diff;
        }
      }
      if (valid) valid[pix] = ok ? 1 : 0;
    }
    count += (int)__popcll(__ballot(ok));
  }
  if ((threadIdx.x & 63) == 0 && count) atomicAdd(n_valid, count);
}

static void flow_free(vdo_optflow* h) {
  hipFree(h->d_pyr); hipFree(h->d_census); hipFree(h->d_level_flow); hipFree(h->d_raw); hipFree(h->d_flow); hipFree(h->d_valid); hipFree(h->d_count); hipFree(h->d_mask);
  if (h->h_count) hipHostFree(h->h_count);
  h->tm.destroy();
  delete h;
}

template <int R>
static void flow_launch_search(hipStream_t s, dim3 grid, const uint64_t* census, int tot, int off, int W, int H, int w, const int2* prior, int prior_stride, int Wup,
                               int2* out, int out_stride, int subpixel, float2* flow) {
  hipLaunchKernelGGL(k_flow_search<R>, grid, dim3(256), 0, s, census, tot, off, W, H, w, prior, prior_stride, Wup, out, out_stride, subpixel, flow);
}

}  // namespace vdo

using namespace vdo;

extern "C" int vdo_optflow_create(vdo_ctx* ctx, int width, int height, const vdo_optflow_params* p, vdo_optflow** out) {
  static const char* who = "vdo_optflow_create";
  if (!ctx) return set_error(VDO_ERR_INVALID, "%s: ctx is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (!p) return set_error(VDO_ERR_INVALID, "%s: params is null", who);
  if (width < 1) return set_error(VDO_ERR_INVALID, "%s: width %d < 1", who, width);
  if (height < 1) return set_error(VDO_ERR_INVALID, "%s: height %d < 1", who, height);
  if (p->levels < 1 || p->levels > kFlowMaxLevels) return set_error(VDO_ERR_INVALID, "%s: levels %d outside 1..%d", who, p->levels, kFlowMaxLevels);
  if (p->radius < 1 || p->radius > 4) return set_error(VDO_ERR_INVALID, "%s: radius %d outside 1..4", who, p->radius);
  if (p->window < 0 || p->window > kFlowHalo) return set_error(VDO_ERR_INVALID, "%s: window %d outside 0..%d", who, p->window, kFlowHalo);
  if (p->median != 0 && p->median != 1) return set_error(VDO_ERR_INVALID, "%s: median %d is neither 0 nor 1", who, p->median);
  if (p->fb_max_diff < -1) return set_error(VDO_ERR_INVALID, "%s: fb_max_diff %d below -1", who, p->fb_max_diff);
  if (p->subpixel != 0 && p->subpixel != 1) return set_error(VDO_ERR_INVALID, "%s: subpixel %d is neither 0 nor 1", who, p->subpixel);
  if ((int64_t)width * height > kFlowMaxPixels) return set_error(VDO_ERR_UNSUPPORTED, "%s: width x height = %d x %d exceeds 2^26 pixels", who, width, height);
  if (height > 65535 * kFlowTY) return set_error(VDO_ERR_UNSUPPORTED, "%s: height %d above %d (the search grid's second dimension)", who, height, 65535 * kFlowTY);
  int rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  vdo_optflow* h = new vdo_optflow;
  h->ctx = ctx; h->W = width; h->H = height; h->p = *p;
  FlowGeom& g = h->g;
  g.L = p->levels;
  int tot = 0, tiles = 0;
  for (int l = 0; l < g.L; ++l) {
    g.W[l] = l ? (g.W[l - 1] + 1) / 2 : width;
    g.H[l] = l ? (g.H[l - 1] + 1) / 2 : height;
    g.off[l] = tot; tot += g.W[l] * g.H[l];
    g.tiles_x[l] = (g.W[l] + kCensusTX - 1) / kCensusTX;
    g.tile0[l] = tiles; tiles += g.tiles_x[l] * ((g.H[l] + kCensusTY - 1) / kCensusTY);
  }
  g.tot = tot; g.tile0[g.L] = tiles;
  const size_t n = (size_t)width * height, n1 = g.L > 1 ? (size_t)g.W[1] * g.H[1] : 1;
  const bool ok = hipMalloc((void**)&h->d_pyr, 2 * (size_t)tot) == hipSuccess && hipMalloc((void**)&h->d_census, 2 * (size_t)tot * sizeof(uint64_t)) == hipSuccess &&
                  hipMalloc((void**)&h->d_level_flow, 2 * (size_t)tot * sizeof(int2)) == hipSuccess && hipMalloc((void**)&h->d_raw, 2 * n1 * sizeof(int2)) == hipSuccess &&
                  hipMalloc((void**)&h->d_flow, 2 * n * sizeof(float)) == hipSuccess && hipMalloc((void**)&h->d_valid, n) == hipSuccess &&
                  hipMalloc((void**)&h->d_count, sizeof(int)) == hipSuccess && hipHostMalloc((void**)&h->h_count, sizeof(int), hipHostMallocDefault) == hipSuccess &&
                  h->tm.create();
  if (!ok) {
    (void)hipGetLastError();
    flow_free(h);
    return set_error(VDO_ERR_OOM, "%s: device allocation failed for %d x %d, %d levels", who, width, height, p->levels);
  }
  *out = h;
  return VDO_OK;
}

extern "C" int vdo_optflow_destroy(vdo_optflow* h) {
  if (!h) return VDO_OK;
  if (ctx_bind(h->ctx) == VDO_OK) hipStreamSynchronize(h->ctx->stream);
  flow_free(h);
  return VDO_OK;
}

extern "C" int vdo_optflow_compute(vdo_optflow* h, const uint8_t* im0, int64_t stride0, const uint8_t* im1, int64_t stride1, int src_is_device, float* flow, uint8_t* valid,
                                   int out_is_device, int32_t* n_valid) {
  static const char* who = "vdo_optflow_compute";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!im0) return set_error(VDO_ERR_INVALID, "%s: im0 is null", who);
  if (!im1) return set_error(VDO_ERR_INVALID, "%s: im1 is null", who);
  if (stride0 < h->W) return set_error(VDO_ERR_INVALID, "%s: stride0 %lld smaller than the width %d", who, (long long)stride0, h->W);
  if (stride1 < h->W) return set_error(VDO_ERR_INVALID, "%s: stride1 %lld smaller than the width %d", who, (long long)stride1, h->W);
  if (!flow) return set_error(VDO_ERR_INVALID, "%s: flow is null", who);
  if (!n_valid) return set_error(VDO_ERR_INVALID, "%s: n_valid is null", who);
  int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const FlowGeom& g = h->g;
  const int W = h->W, H = h->H, L = g.L, tot = g.tot;
  const size_t n_pix = (size_t)W * H;
  const auto t0 = h->tm.begin(s);
  // level 0 of the two pyramids is the pair, packed (a device pair that already lies there stays where it is)
  const hipMemcpyKind kind = src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (!(src_is_device && im0 == h->d_pyr && stride0 == W)) hipMemcpy2DAsync(h->d_pyr, W, im0, (size_t)stride0, W, H, kind, s);
  if (!(src_is_device && im1 == h->d_pyr + tot && stride1 == W)) hipMemcpy2DAsync(h->d_pyr + tot, W, im1, (size_t)stride1, W, H, kind, s);
  if (L > 1) hipLaunchKernelGGL(k_flow_pyramid, dim3((W + kFlowRegion - 1) / kFlowRegion, (H + kFlowRegion - 1) / kFlowRegion, 2), dim3(256), 0, s, h->d_pyr, g);
  hipLaunchKernelGGL(k_flow_census, dim3(2 * g.tile0[L]), dim3(256), 0, s, (const uint8_t*)h->d_pyr, g, h->d_census);
  hipMemsetAsync(h->d_count, 0, sizeof(int), s);
  const int n_dir = h->p.fb_max_diff >= 0 ? 2 : 1;
  float* d_flow = out_is_device ? flow : h->d_flow;
  uint8_t* d_valid = !valid ? nullptr : out_is_device ? valid : h->d_valid;
  const int n1 = L > 1 ? g.W[1] * g.H[1] : 1;
  for (int l = L - 1; l >= 0; --l) {
    const bool filtered = h->p.median && l >= 1;
    const dim3 grid((g.W[l] + kFlowTX - 1) / kFlowTX, (g.H[l] + kFlowTY - 1) / kFlowTY, n_dir);
    const int2* prior = l == L - 1 ? nullptr : h->d_level_flow + g.off[l + 1];
    const int Wup = l == L - 1 ? 0 : g.W[l + 1];
    int2* out = filtered ? h->d_raw : h->d_level_flow + g.off[l];
    const int out_stride = filtered ? n1 : tot;
    float2* fl = l == 0 ? (float2*)d_flow : nullptr;
    const uint64_t* cen = h->d_census;
    switch (h->p.radius) {
      case 1: flow_launch_search<1>(s, grid, cen, tot, g.off[l], g.W[l], g.H[l], h->p.window, prior, tot, Wup, out, out_stride, h->p.subpixel, fl); break;
      case 2: flow_launch_search<2>(s, grid, cen, tot, g.off[l], g.W[l], g.H[l], h->p.window, prior, tot, Wup, out, out_stride, h->p.subpixel, fl); break;
      case 3: flow_launch_search<3>(s, grid, cen, tot, g.off[l], g.W[l], g.H[l], h->p.window, prior, tot, Wup, out, out_stride, h->p.subpixel, fl); break;
      default: flow_launch_search<4>(s, grid, cen, tot, g.off[l], g.W[l], g.H[l], h->p.window, prior, tot, Wup, out, out_stride, h->p.subpixel, fl); break;
    }
    if (filtered)
      hipLaunchKernelGGL(k_flow_median, dim3((g.W[l] * g.H[l] + 255) / 256, 1, n_dir), dim3(256), 0, s, (const int2*)h->d_raw, n1, g.W[l], g.H[l], h->d_level_flow + g.off[l], tot);
  }
  hipLaunchKernelGGL(k_flow_check, dim3((unsigned)((n_pix + 256 * kFlowCheckBatches - 1) / (256 * kFlowCheckBatches))), dim3(256), 0, s, (const int2*)h->d_level_flow, n_dir == 2 ? (const int2*)(h->d_level_flow + tot) : nullptr, W, H,
                     h->p.fb_max_diff, d_valid, h->d_count);
  h->tm.mark_end(s);
  hipMemcpyAsync(h->h_count, h->d_count, sizeof(int), hipMemcpyDeviceToHost, s);
  if (!out_is_device) {
    hipMemcpyAsync(flow, h->d_flow, 2 * n_pix * sizeof(float), hipMemcpyDeviceToHost, s);
    if (valid) hipMemcpyAsync(valid, h->d_valid, n_pix, hipMemcpyDeviceToHost, s);
  }
  rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  *n_valid = *h->h_count;
  h->tm.finish(t0);
  h->computed = true;
  return VDO_OK;
}

extern "C" int vdo_optflow_level_size(vdo_optflow* h, int level, int* width, int* height) {
  static const char* who = "vdo_optflow_level_size";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (level < 0 || level >= h->g.L) return set_error(VDO_ERR_INVALID, "%s: level %d outside 0..%d", who, level, h->g.L - 1);
  if (!width || !height) return set_error(VDO_ERR_INVALID, "%s: %s is null", who, !width ? "width" : "height");
  *width = h->g.W[level]; *height = h->g.H[level];
  return VDO_OK;
}

// the level's part of one of the [2][tot] arrays, elem bytes per pixel, to the host
static int flow_fetch(const char* who, vdo_optflow* h, const char* sel_name, int sel, int level, const void* dev, size_t elem, void* out) {
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (sel != 0 && sel != 1) return set_error(VDO_ERR_INVALID, "%s: %s %d is neither 0 nor 1", who, sel_name, sel);
  if (level < 0 || level >= h->g.L) return set_error(VDO_ERR_INVALID, "%s: level %d outside 0..%d", who, level, h->g.L - 1);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (!h->computed) return set_error(VDO_ERR_INVALID, "%s: no vdo_optflow_compute on this handle yet", who);
  const int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  const size_t first = (size_t)sel * h->g.tot + h->g.off[level], count = (size_t)h->g.W[level] * h->g.H[level];
  hipMemcpyAsync(out, (const char*)dev + first * elem, count * elem, hipMemcpyDeviceToHost, h->ctx->stream);
  return check_hip(who, hipStreamSynchronize(h->ctx->stream));
}

extern "C" int vdo_optflow_get_pyramid(vdo_optflow* h, int which, int level, uint8_t* out) {
  return flow_fetch("vdo_optflow_get_pyramid", h, "which", which, level, h ? h->d_pyr : nullptr, sizeof(uint8_t), out);
}

extern "C" int vdo_optflow_get_census(vdo_optflow* h, int which, int level, uint64_t* out) {
  return flow_fetch("vdo_optflow_get_census", h, "which", which, level, h ? h->d_census : nullptr, sizeof(uint64_t), out);
}

extern "C" int vdo_optflow_get_level_flow(vdo_optflow* h, int dir, int level, int32_t* out) {
  if (h && dir == 1 && h->p.fb_max_diff < 0) return set_error(VDO_ERR_INVALID, "vdo_optflow_get_level_flow: dir 1 with fb_max_diff -1: nothing backward runs");
  return flow_fetch("vdo_optflow_get_level_flow", h, "dir", dir, level, h ? h->d_level_flow : nullptr, sizeof(int2), out);
}

extern "C" int vdo_optflow_last_timing(vdo_optflow* h, double ms[2]) {
  return last_timing("vdo_optflow_last_timing", h ? &h->tm : nullptr, ms);
}

extern "C" int vdo_optflow_device_images(vdo_optflow* h, uint8_t** im0, uint8_t** im1, float** flow, uint8_t** valid) {
  if (!h) return set_error(VDO_ERR_INVALID, "vdo_optflow_device_images: handle is null");
  if (im0) *im0 = h->d_pyr;
  if (im1) *im1 = h->d_pyr + h->g.tot;
  if (flow) *flow = h->d_flow;
  if (valid) *valid = h->d_valid;
  return VDO_OK;
}

extern "C" int vdo_optflow_stage_mask(vdo_optflow* h, const int32_t* mask, int32_t** mask_dev) {
  static const char* who = "vdo_optflow_stage_mask";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!mask || !mask_dev) return set_error(VDO_ERR_INVALID, "%s: %s is null", who, !mask ? "mask" : "mask_dev");
  const int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  const size_t n = (size_t)h->W * h->H;
  if (!h->d_mask && hipMalloc((void**)&h->d_mask, n * sizeof(int32_t)) != hipSuccess) { h->d_mask = nullptr; return set_error(VDO_ERR_OOM, "%s: device allocation failed", who); }
  hipMemcpyAsync(h->d_mask, mask, n * sizeof(int32_t), hipMemcpyHostToDevice, h->ctx->stream);
  const int rs = check_hip(who, hipStreamSynchronize(h->ctx->stream));
  if (rs != VDO_OK) return rs;
  *mask_dev = h->d_mask;
  return VDO_OK;
}
