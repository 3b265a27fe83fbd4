// ORB front-end on gfx950 — replaces ORBextractor::operator() (reference src/ORBextractor.cc:1035-1110):
//   K3 ComputePyramid          :1112-1137  cv::resize(INTER_LINEAR, 8u) from the previous level + REFLECT_101 border (19 px)
//   K4 ComputeKeyPointsOctTree :754-818    cv::FAST(cell, thr=iniTh, NMS) with fallback minTh, per 30-px cell (+6 px overlap)
//   K5 DistributeOctTree       :470-752    quadtree, best response per node      (k_quadtree: one workgroup per level, rounds built from
//                                          scans; QuadTree, host C++, is the fallback over its limits and under VDO_ORB_HOST_TREE=1)
//   K6 IC_Angle                :66-93      31x31 circular patch moments + cv::fastAtan2
//   K7 GaussianBlur 7x7 s=2    :1083-1084  executed by the reference although its consumer (BRIEF) is commented out
//   K8 computeOrbDescriptor    :97-136     256 rotated pair tests on the blurred level (call site commented out :1083-1091;
//                                          here on request: vdo_orb_descriptors / vdo_orb_extract_desc)
// Image-sized work is HBM/L2-bound integer arithmetic: tiles are staged in LDS (cell ROI 37x37,
// blur tile + 3-px halo), one workgroup per FAST cell over ALL pyramid levels in a single launch,
// candidates are compacted in raster order with a workgroup scan so that the reference's feature
// order — and therefore every downstream feature index — is reproduced exactly.
// OpenCV 3.4 fixed-point semantics are restated (parity unpinned).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <cstring>
#include <vector>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"
#include "host_pool.hpp"
#include "orb_match.hpp"
#include "orb_pattern.hpp"

namespace vdo {

constexpr int kEdge = 19, kHalfPatch = 15, kPatch = 31;
constexpr int kSpecCand = 24576;       // VDO_ORB_FUSED_ANGLE=1: candidates copied speculatively together with the header (typ. 10-15 k per KITTI frame)
constexpr int kMaxCellDim = 68;        // hCell = ceil(height/nRows) < 60, +6 overlap
static_assert(kMaxCellDim <= 128, "k_fast_cells packs cell-local coordinates in 7 bits");

struct LevelDesc { int w, h, bw, bh; int64_t off; int64_t off_inner; int64_t off_blur; };   // bordered image at img + off; blurred interior (w x h, contiguous) at blur + off_blur
struct CellDesc { int level, x0, y0, x1, y1, addx, addy, pad; };          // ROI in level interior coords; add = j*wCell, i*hCell

__device__ __forceinline__ int reflect101(int p, int len) {
  if (len == 1) return 0;
  while (p < 0 || p >= len) { if (p < 0) p = -p; else p = 2 * (len - 1) - p; }
  return p;
}

// ------------------------------------------------------------------------------------ K2
__global__ void k_rgb2gray(const uint8_t* __restrict__ src, int64_t n, int ch, int rgb_order, uint8_t* __restrict__ dst) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* p = src + i * ch;
  const int r = rgb_order ? p[0] : p[2], g = p[1], b = rgb_order ? p[2] : p[0];
  dst[i] = (uint8_t)((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14);
}

// K1: d<0 -> 0 ; else bf / (d / factor)       (src/Tracking.cc:180-204)
__global__ void k_depth_preprocess(float* __restrict__ d, int64_t n, float bf, float factor) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = d[i];
  d[i] = v < 0 ? 0.f : bf / (v / factor);
}

// ------------------------------------------------------------------------------------ K3
// level 0: copy + border.
__global__ void k_border_copy(const uint8_t* __restrict__ src, int sw, int sh, int sstride, uint8_t* __restrict__ dst, int bw, int bh) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= bw || y >= bh) return;
  dst[(size_t)y * bw + x] = src[(size_t)reflect101(y - kEdge, sh) * sstride + reflect101(x - kEdge, sw)];
}
// level l>0: bilinear (11-bit fixed point) from the previous level's interior, border by reflection.
__global__ void k_resize_border(const uint8_t* __restrict__ src /*interior of level l-1*/, int sw, int sh, int sstride,
                                uint8_t* __restrict__ dst, int dw, int dh, double scale_x, double scale_y) {
  const int bx = blockIdx.x * blockDim.x + threadIdx.x, by = blockIdx.y * blockDim.y + threadIdx.y;
  const int bw = dw + 2 * kEdge, bh = dh + 2 * kEdge;
  if (bx >= bw || by >= bh) return;
  const int dx = reflect101(bx - kEdge, dw), dy = reflect101(by - kEdge, dh);
  float fx = (float)((dx + 0.5) * scale_x - 0.5);
  int sx = (int)floorf(fx);
  fx -= sx;
  bool xedge = false;
  if (sx < 0) { fx = 0; sx = 0; }
  if (sx + 1 >= sw) { xedge = true; fx = 0; sx = sw - 1; }
  const int a0 = max(-32768, min(32767, (int)rintf((1.f - fx) * 2048))), a1 = max(-32768, min(32767, (int)rintf(fx * 2048)));
  float fy = (float)((dy + 0.5) * scale_y - 0.5);
  int sy = (int)floorf(fy);
  fy -= sy;
  const int b0 = max(-32768, min(32767, (int)rintf((1.f - fy) * 2048))), b1 = max(-32768, min(32767, (int)rintf(fy * 2048)));
  const int sy0 = min(max(sy, 0), sh - 1), sy1 = min(max(sy + 1, 0), sh - 1);
  const uint8_t* S0 = src + (size_t)sy0 * sstride;
  const uint8_t* S1 = src + (size_t)sy1 * sstride;
  int r0, r1;
  if (!xedge) { r0 = S0[sx] * a0 + S0[sx + 1] * a1; r1 = S1[sx] * a0 + S1[sx + 1] * a1; }
  else { r0 = S0[sx] * 2048; r1 = S1[sx] * 2048; }
  dst[(size_t)by * bw + bx] = (uint8_t)((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2);
}

// The whole pyramid in ONE launch.  A level is resized from the level below, so eight dependent launches used to build it (~60 us of
// stream time, 8 launch overheads on the host).  Here every workgroup owns one 32x32 tile of one level and recomputes, in LDS, the
// regions of the levels below that feed it, cascading up from the source image: level 0 region -> level 1 region -> ... -> the
// tile.  Every pixel of every level is computed with the same fixed-point formula from the same exact inputs as in the
// level-by-level version (k_resize_border), so the result is bit-identical; the recomputation (a level-7 tile needs a ~130x130
// source window) costs a few microseconds of an otherwise idle GPU.  The 19-px REFLECT_101 border is written by the owner of
// the mirrored interior pixel.
struct PyrDesc {
  int n_levels;                 // levels of the pyramid (0: this launch form is not used)
  int base, lv0, lv1;           // this launch builds levels [lv0, lv1) from the image of level `base` (0: the source image)
  int w[8], h[8];
  double sx[8], sy[8];          // scale of level l relative to level l-1 (inv of cv::resize's inv_scale), [0] unused
  int tile_off[9];              // first workgroup of every level
  int tiles_x[8];
};
constexpr int kPyrRegion = 96;    // max edge of a cascaded region (checked on the host at create time)

__device__ __forceinline__ void resize_src(int d, double scale, int slen, int& s0, int& s1, int& c0, int& c1) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int si = (int)floorf(f);
  f -= si;
  bool edge = false;
  if (si < 0) { f = 0; si = 0; }
  if (si + 1 >= slen) { edge = true; f = 0; si = slen - 1; }
  c0 = max(-32768, min(32767, (int)rintf((1.f - f) * 2048))); c1 = max(-32768, min(32767, (int)rintf(f * 2048)));
  s0 = si; s1 = edge ? si : si + 1;
  if (edge) { c0 = 2048; c1 = 0; }
}
// vertical taps of cv::resize are NOT collapsed at the border: both rows are clamped (k_resize_border does the same)
__device__ __forceinline__ void resize_src_y(int d, double scale, int slen, int& s0, int& s1, int& c0, int& c1) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int si = (int)floorf(f);
  f -= si;
  c0 = max(-32768, min(32767, (int)rintf((1.f - f) * 2048))); c1 = max(-32768, min(32767, (int)rintf(f * 2048)));
  s0 = min(max(si, 0), slen - 1); s1 = min(max(si + 1, 0), slen - 1);
}

__global__ __launch_bounds__(256) void k_pyramid_all(const uint8_t* __restrict__ src, int sstride, PyrDesc P, const LevelDesc* __restrict__ levels, uint8_t* __restrict__ pyr) {
  __shared__ uint8_t bufA[kPyrRegion * kPyrRegion];
  __shared__ uint8_t bufB[kPyrRegion * kPyrRegion];
  __shared__ int rx0[8], rx1[8], ry0[8], ry1[8];
  int lvl = P.lv0;
  while (lvl + 1 < P.lv1 && (int)blockIdx.x >= P.tile_off[lvl + 1]) ++lvl;
  const int t = blockIdx.x - P.tile_off[lvl], ty = t / P.tiles_x[lvl], tx = t - ty * P.tiles_x[lvl];
  if (threadIdx.x == 0) {
    // inclusive pixel ranges needed at every level, from the tile down to the source
    int x0 = tx * 32, x1 = min(x0 + 31, P.w[lvl] - 1), y0 = ty * 32, y1 = min(y0 + 31, P.h[lvl] - 1);
    rx0[lvl] = x0; rx1[lvl] = x1; ry0[lvl] = y0; ry1[lvl] = y1;
    for (int k = lvl; k > P.base; --k) {
      int a0, a1, c0, c1, b0, b1;
      resize_src(x0, P.sx[k], P.w[k - 1], a0, a1, c0, c1);
      resize_src(x1, P.sx[k], P.w[k - 1], b0, b1, c0, c1);
      x0 = a0; x1 = b1;
      resize_src_y(y0, P.sy[k], P.h[k - 1], a0, a1, c0, c1);
      resize_src_y(y1, P.sy[k], P.h[k - 1], b0, b1, c0, c1);
      y0 = a0; y1 = b1;
      rx0[k - 1] = x0; rx1[k - 1] = x1; ry0[k - 1] = y0; ry1[k - 1] = y1;
    }
  }
  __syncthreads();
  // region of the base level from its image (the source, or a level an earlier launch wrote)
  uint8_t* cur = bufA;
  uint8_t* nxt = bufB;
  {
    const int bs = P.base;
    const int w0 = rx1[bs] - rx0[bs] + 1, h0 = ry1[bs] - ry0[bs] + 1;
    for (int i = threadIdx.x; i < w0 * h0; i += 256) { const int yy = i / w0, xx = i - yy * w0; cur[yy * kPyrRegion + xx] = src[(size_t)(ry0[bs] + yy) * sstride + rx0[bs] + xx]; }
  }
  __syncthreads();
  for (int k = P.base + 1; k <= lvl; ++k) {
    const int wk = rx1[k] - rx0[k] + 1, hk = ry1[k] - ry0[k] + 1;
    const int ox = rx0[k - 1], oy = ry0[k - 1];
    for (int i = threadIdx.x; i < wk * hk; i += 256) {
      const int yy = i / wk, xx = i - yy * wk;
      int sx0, sx1, a0, a1, sy0, sy1, b0, b1;
      resize_src(rx0[k] + xx, P.sx[k], P.w[k - 1], sx0, sx1, a0, a1);
      resize_src_y(ry0[k] + yy, P.sy[k], P.h[k - 1], sy0, sy1, b0, b1);
      const uint8_t* S0 = cur + (sy0 - oy) * kPyrRegion - ox;
      const uint8_t* S1 = cur + (sy1 - oy) * kPyrRegion - ox;
      const int r0 = S0[sx0] * a0 + S0[sx1] * a1, r1 = S1[sx0] * a0 + S1[sx1] * a1;
      nxt[yy * kPyrRegion + xx] = (uint8_t)((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2);
    }
    __syncthreads();
    uint8_t* tmp = cur; cur = nxt; nxt = tmp;
  }
  // the tile (interior) + the border pixels that mirror its pixels (REFLECT_101: p <-> -p and p <-> 2(len-1) - p, 19 px wide)
  const LevelDesc L = levels[lvl];
  uint8_t* dst = pyr + L.off;
  const int wt = rx1[lvl] - rx0[lvl] + 1, ht = ry1[lvl] - ry0[lvl] + 1;
  for (int i = threadIdx.x; i < wt * ht; i += 256) {
    const int yy = i / wt, xx = i - yy * wt;
    const int x = rx0[lvl] + xx, y = ry0[lvl] + yy;
    const uint8_t v = cur[yy * kPyrRegion + xx];
    int xs[2] = {x, 0}, ys[2] = {y, 0};
    bool mx = false, my = false;
    if (x >= 1 && x <= kEdge) { xs[1] = -x; mx = true; } else if (x <= L.w - 2 && x >= L.w - 1 - kEdge) { xs[1] = 2 * (L.w - 1) - x; mx = true; }
    if (y >= 1 && y <= kEdge) { ys[1] = -y; my = true; } else if (y <= L.h - 2 && y >= L.h - 1 - kEdge) { ys[1] = 2 * (L.h - 1) - y; my = true; }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
        if ((a == 0 || my) && (b == 0 || mx)) dst[(size_t)(ys[a] + kEdge) * L.bw + xs[b] + kEdge] = v;
  }
}

// ------------------------------------------------------------------------------------ K4
__device__ __forceinline__ int fast_score_lds(const uint8_t* roi, int stride, int x, int y, int t) {
  const uint8_t* c = roi + y * stride + x;
  const int v = c[0];
  int r[16];
  r[0] = c[3 * stride]; r[1] = c[3 * stride + 1]; r[2] = c[2 * stride + 2]; r[3] = c[stride + 3];
  r[4] = c[3]; r[5] = c[-stride + 3]; r[6] = c[-2 * stride + 2]; r[7] = c[-3 * stride + 1];
  r[8] = c[-3 * stride]; r[9] = c[-3 * stride - 1]; r[10] = c[-2 * stride - 2]; r[11] = c[-stride - 3];
  r[12] = c[-3]; r[13] = c[stride - 3]; r[14] = c[2 * stride - 2]; r[15] = c[3 * stride - 1];
  // cheap necessary condition (opposite pairs): a 9-arc contains one pixel of every opposite pair
  int best = -1000;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    int mb = 1000, md = 1000;
#pragma unroll
    for (int k = 0; k < 9; ++k) { const int q = r[(s + k) & 15]; mb = min(mb, q - v); md = min(md, v - q); }
    best = max(best, max(mb, md));
  }
  return best > t ? best - 1 : 0;
}

// One workgroup per cell.  out_cnt[cell], out_pack[cell*cell_cap + k] = x | y<<7 | score<<24 (cell-local coords, < kMaxCellDim:
// any level size fits; k_compact_angle adds the cell's addx / addy).  cell_cap bounds the count of every cell (vdo_orb_create).
__global__ __launch_bounds__(256) void k_fast_cells(const uint8_t* __restrict__ pyr, const LevelDesc* __restrict__ levels,
                                                    const CellDesc* __restrict__ cells, int ini_th, int min_th, int cell_cap,
                                                    int* __restrict__ out_cnt, uint32_t* __restrict__ out_pack) {
  __shared__ uint8_t roi[kMaxCellDim * kMaxCellDim];
  __shared__ uint8_t sc[kMaxCellDim * kMaxCellDim];
  __shared__ int s_wave[4], s_total;
  const CellDesc C = cells[blockIdx.x];
  const LevelDesc L = levels[C.level];
  const int w = C.x1 - C.x0, h = C.y1 - C.y0, tid = threadIdx.x;
  const uint8_t* img = pyr + L.off_inner;     // interior origin, row stride L.bw
  for (int i = tid; i < w * h; i += 256) { const int y = i / w, x = i - y * w; roi[y * kMaxCellDim + x] = img[(size_t)(C.y0 + y) * L.bw + (C.x0 + x)]; }
  __syncthreads();
  const int npix = w * h;
  const int per = (npix + 255) / 256;          // contiguous raster chunk per thread -> ordered compaction
  int t = ini_th;
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = tid; i < npix; i += 256) {
      const int y = i / w, x = i - y * w;
      int s = 0;
      if (x >= 3 && x < w - 3 && y >= 3 && y < h - 3 && w >= 7 && h >= 7) s = fast_score_lds(roi, kMaxCellDim, x, y, t);
      sc[y * kMaxCellDim + x] = (uint8_t)s;
    }
    __syncthreads();
    // NMS (strict > against the 8 neighbours) + count in this thread's raster chunk
    unsigned keep = 0;
    int cnt = 0;
    for (int k = 0; k < per; ++k) {
      const int i = tid * per + k;
      if (i >= npix) break;
      const int y = i / w, x = i - y * w;
      const int s = sc[y * kMaxCellDim + x];
      if (s == 0) continue;
      const uint8_t* p = sc + y * kMaxCellDim + x;
      if (s > p[-1] && s > p[1] && s > p[-kMaxCellDim - 1] && s > p[-kMaxCellDim] && s > p[-kMaxCellDim + 1] &&
          s > p[kMaxCellDim - 1] && s > p[kMaxCellDim] && s > p[kMaxCellDim + 1]) { keep |= 1u << k; ++cnt; }
    }
    // workgroup exclusive scan of cnt
    const int lane = tid & 63, wv = tid >> 6;
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(incl, off, 64); if (lane >= off) incl += v; }
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    if (tid == 0) { int a = 0; for (int q = 0; q < 4; ++q) { const int v = s_wave[q]; s_wave[q] = a; a += v; } s_total = a; }
    __syncthreads();
    const int total = s_total;
    if (total > 0 || pass == 1) {
      int pos = s_wave[wv] + incl - cnt;
      for (int k = 0; k < per; ++k) {
        if (!(keep & (1u << k))) continue;
        const int i = tid * per + k;
        const int y = i / w, x = i - y * w;
        if (pos < cell_cap)
          out_pack[(size_t)blockIdx.x * cell_cap + pos] = (uint32_t)x | ((uint32_t)y << 7) | ((uint32_t)sc[y * kMaxCellDim + x] << 24);
        ++pos;
      }
      if (tid == 0) out_cnt[blockIdx.x] = total;
      return;
    }
    t = min_th;          // vKeysCell.empty() -> retry the whole cell with minThFAST
    __syncthreads();
  }
}

// umax of the circular patch (ORBextractor.cc:443-458), filled on the host
struct UMax { int v[kHalfPatch + 2]; };

// cv::fastAtan2, degrees
__device__ __forceinline__ float fast_atan2_dev(float y, float x) {
  const float p1 = 0.9997878412794807f * (float)(180 / M_PI), p3 = -0.3258083974640975f * (float)(180 / M_PI);
  const float p5 = 0.1555786518463281f * (float)(180 / M_PI), p7 = -0.04432655554792128f * (float)(180 / M_PI);
  const float ax = fabsf(x), ay = fabsf(y);
  float a, c, c2;
  if (ax >= ay) { c = ay / (ax + (float)2.2204460492503131e-16); c2 = c * c; a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c; }
  else { c = ax / (ay + (float)2.2204460492503131e-16); c2 = c * c; a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c; }
  if (x < 0) a = 180.f - a;
  if (y < 0) a = 360.f - a;
  return a;
}

// Compaction to dense arrays + K6 angle for every candidate: one wave per candidate (31 rows over the lanes).
// dense: x,y (float, relative to (16,16)), resp, angle, level
__global__ __launch_bounds__(256) void k_compact_angle(const uint8_t* __restrict__ pyr, const LevelDesc* __restrict__ levels,
                                                       const CellDesc* __restrict__ cells, const int* __restrict__ cnt, const int* __restrict__ cell_level,
                                                       int* __restrict__ level_cnt, const uint32_t* __restrict__ pack, int ncells, int cell_cap, UMax um,
                                                       float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ oresp,
                                                       float* __restrict__ oang, int* __restrict__ olevel) {
  const int cell = blockIdx.x;
  const int n = min(cnt[cell], cell_cap);
  const CellDesc C = cells[cell];
  const int lvl = C.level;
  const LevelDesc L = levels[lvl];
  const uint8_t* img = pyr + L.off_inner;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // dense offset of this cell = number of candidates in the cells before it (every workgroup sums its own prefix: ~1100 counts,
  // L2-resident - cheaper than a separate single-workgroup scan kernel in front of this one); workgroup 0 also writes the header
  // (per-level counts + total + the largest count of one cell, checked against cell_cap) the host fetches next to the candidates
  __shared__ int s_part[4], s_lvl[17];
  int base;
  {
    int a = 0;
    for (int c = threadIdx.x; c < cell; c += 256) a += min(cnt[c], cell_cap);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    if (lane == 0) s_part[wv] = a;
    if (cell == 0 && threadIdx.x < 17) s_lvl[threadIdx.x] = 0;
    __syncthreads();
    base = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    if (cell == 0) {
      int mx = 0;
      for (int c = threadIdx.x; c < ncells; c += 256) { const int r = cnt[c], v = min(r, cell_cap); if (v) atomicAdd(&s_lvl[cell_level[c]], v); mx = max(mx, r); }
      atomicMax(&s_lvl[16], mx);
      __syncthreads();
      if (threadIdx.x < 16) level_cnt[threadIdx.x] = s_lvl[threadIdx.x];
      if (threadIdx.x == 0) { int t = 0; for (int q = 0; q < 16; ++q) t += s_lvl[q]; level_cnt[16] = t; level_cnt[17] = s_lvl[16]; }
    }
  }
  for (int k = wv; k < n; k += 4) {
    const uint32_t pk = pack[(size_t)cell * cell_cap + k];
    const int x = (int)(pk & 0x7f) + C.addx, y = (int)((pk >> 7) & 0x7f) + C.addy, s = (int)(pk >> 24);     // level coords rel. (16,16)
    const int cx = x + (kEdge - 3), cy = y + (kEdge - 3);       // cvRound of integer-valued coordinates
    // rows v = -15..15 -> lanes 0..30
    int m10 = 0, m01 = 0;
    if (lane < 31) {
      const int v = lane - kHalfPatch;
      const int d = um.v[v < 0 ? -v : v];
      const uint8_t* row = img + (size_t)(cy + v) * L.bw + cx;
      int rs = 0;
      for (int u = -d; u <= d; ++u) { const int p = row[u]; m10 += u * p; rs += p; }
      m01 = v * rs;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { m10 += __shfl_down(m10, off, 64); m01 += __shfl_down(m01, off, 64); }
    if (lane == 0) {
      const int o = base + k;
      ox[o] = (float)x; oy[o] = (float)y; oresp[o] = (float)s; olevel[o] = lvl;
      oang[o] = fast_atan2_dev((float)m01, (float)m10);
    }
  }
}

// The split form of k_compact_angle (default; VDO_ORB_FUSED_ANGLE=1 keeps the kernel above).  The host quadtrees read x, y and
// resp only, so the angles need not stand between k_fast_cells and the host:
//   k_compact  the same prefix over the cell counts and the same header, then x, y, resp, level of every candidate to the dense
//              device arrays AND x, y, resp + the header to mapped pinned memory (hx / hy / hresp / hhdr: coalesced rows, written
//              once) - no copy operation in front of the event the host waits for;
//   k_angle    queued behind that event: the per-candidate loop of k_compact_angle (one wave per candidate, 31 rows over the
//              lanes, the same integer moments and fast_atan2_dev) over the dense arrays.
__global__ __launch_bounds__(256) void k_compact(const CellDesc* __restrict__ cells, const int* __restrict__ cnt, const int* __restrict__ cell_level,
                                                 int* __restrict__ level_cnt, const uint32_t* __restrict__ pack, int ncells, int cell_cap,
                                                 float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ oresp, int* __restrict__ olevel,
                                                 int* __restrict__ hhdr, float* __restrict__ hx, float* __restrict__ hy, float* __restrict__ hresp) {
  const int cell = blockIdx.x;
  const int n = min(cnt[cell], cell_cap);
  const CellDesc C = cells[cell];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __shared__ int s_part[4], s_lvl[17];
  int a = 0;
  for (int c = threadIdx.x; c < cell; c += 256) a += min(cnt[c], cell_cap);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
  if (lane == 0) s_part[wv] = a;
  if (cell == 0 && threadIdx.x < 17) s_lvl[threadIdx.x] = 0;
  __syncthreads();
  const int base = s_part[0] + s_part[1] + s_part[2] + s_part[3];
  if (cell == 0) {
    int mx = 0;
    for (int c = threadIdx.x; c < ncells; c += 256) { const int r = cnt[c], v = min(r, cell_cap); if (v) atomicAdd(&s_lvl[cell_level[c]], v); mx = max(mx, r); }
    atomicMax(&s_lvl[16], mx);
    __syncthreads();
    if (threadIdx.x < 16) level_cnt[threadIdx.x] = hhdr[threadIdx.x] = s_lvl[threadIdx.x];
    if (threadIdx.x == 0) { int t = 0; for (int q = 0; q < 16; ++q) t += s_lvl[q]; level_cnt[16] = hhdr[16] = t; level_cnt[17] = hhdr[17] = s_lvl[16]; }
  }
  for (int k = threadIdx.x; k < n; k += 256) {       // (n <= cell_cap: base + k < ncells * cell_cap = dense_cap, the length of every row)
    const uint32_t pk = pack[(size_t)cell * cell_cap + k];
    const float x = (float)((int)(pk & 0x7f) + C.addx), y = (float)((int)((pk >> 7) & 0x7f) + C.addy), s = (float)(int)(pk >> 24);
    const int o = base + k;
    ox[o] = x; oy[o] = y; oresp[o] = s; olevel[o] = C.level;
    hx[o] = x; hy[o] = y; hresp[o] = s;
  }
}

// One wave per candidate as in k_compact_angle; a wave takes kAngChunk consecutive candidates and stores their angles with one
// instruction (one contiguous write to the mapped row instead of kAngChunk single floats).  total = level_cnt[16] (k_compact).
constexpr int kAngChunk = 8;
// IC_Angle of the candidate at (x, y) of level L by one wave: 31 rows over the lanes, integer moments, fast_atan2_dev (every lane returns it)
__device__ __forceinline__ float wave_ic_angle(const uint8_t* __restrict__ pyr, const LevelDesc& L, const UMax& um, int x, int y, int lane) {
  const uint8_t* img = pyr + L.off_inner;
  const int cx = x + (kEdge - 3), cy = y + (kEdge - 3);
  int m10 = 0, m01 = 0;
  if (lane < 31) {
    const int v = lane - kHalfPatch;
    const int d = um.v[v < 0 ? -v : v];
    const uint8_t* row = img + (size_t)(cy + v) * L.bw + cx;
    int rs = 0;
    for (int u = -d; u <= d; ++u) { const int p = row[u]; m10 += u * p; rs += p; }
    m01 = v * rs;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { m10 += __shfl_down(m10, off, 64); m01 += __shfl_down(m01, off, 64); }
  return fast_atan2_dev((float)__shfl(m01, 0, 64), (float)__shfl(m10, 0, 64));
}
__global__ __launch_bounds__(256) void k_angle(const uint8_t* __restrict__ pyr, const LevelDesc* __restrict__ levels, const int* __restrict__ level_cnt, UMax um,
                                               const float* __restrict__ ox, const float* __restrict__ oy, const int* __restrict__ olevel,
                                               float* __restrict__ oang, float* __restrict__ hang) {
  const int total = level_cnt[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int c0 = (blockIdx.x * 4 + wv) * kAngChunk; c0 < total; c0 += gridDim.x * 4 * kAngChunk) {
    float mine = 0.f;
    const int ce = min(c0 + kAngChunk, total);
    for (int o = c0; o < ce; ++o) {
      const int x = (int)ox[o], y = (int)oy[o];                 // integer-valued floats (k_compact)
      const LevelDesc L = levels[olevel[o]];
      const float ang = wave_ic_angle(pyr, L, um, x, y, lane);
      if (lane == o - c0) mine = ang;
    }
    if (c0 + lane < ce) { oang[c0 + lane] = mine; hang[c0 + lane] = mine; }
  }
}

// ------------------------------------------------------------------------------------ K7
// 7x7 Gaussian, sigma 2, 8-bit fixed-point separable (OpenCV 3.4.0 path), REFLECT_101 at the interior edge.
struct Blur7 { int k[7]; };
// ------------------------------------------------------------------------------------ K8
// computeOrbDescriptor (reference src/ORBextractor.cc:97-136): for each of the 256 learned point pairs, rotated by the
// keypoint angle, compare two pixels of the blurred level image: bit = I(p0) < I(p1); pixel index =
// cvRound(x*b + y*a)*step + cvRound(x*a - y*b) around cvRound(kp) with a = cos, b = sin (fp32 products and sums, no
// contraction).  One wave per keypoint: lane i evaluates tests 4i..4i+3 (one 16-byte load of its slice of the pattern),
// neighbouring lanes merge their nibbles into a byte, even lanes write the 32 bytes.
// cos/sin: evaluated in double from +,-,* only and rounded to float (= correctly rounded cosf/sinf up to double-rounding
// ties); the oracle runs the same operations, so the descriptor BITS agree although ocml and glibc sinf/cosf do not.
struct OrbPattern { int4 q[64]; };

__device__ __forceinline__ void sincos_exact_dev(float angle, float* s_out, float* c_out) {
  const double x = (double)angle;
  const int k = (int)(x * 0.63661977236758138 + 0.5);
  const double r = (x - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11;
  const double z = r * r;
  const double sp = r * (1.0 + z * (-1.0 / 6 + z * (1.0 / 120 + z * (-1.0 / 5040 + z * (1.0 / 362880 + z * (-1.0 / 39916800 + z * (1.0 / 6227020800.0 +
                    z * (-1.0 / 1307674368000.0 + z * (1.0 / 355687428096000.0)))))))));
  const double cp = 1.0 + z * (-1.0 / 2 + z * (1.0 / 24 + z * (-1.0 / 720 + z * (1.0 / 40320 + z * (-1.0 / 3628800 + z * (1.0 / 479001600 +
                    z * (-1.0 / 87178291200.0 + z * (1.0 / 20922789888000.0))))))));
  double sn, cs;
  switch (k & 3) {
    case 0: sn = sp; cs = cp; break;
    case 1: sn = cp; cs = -sp; break;
    case 2: sn = -sp; cs = -cp; break;
    default: sn = -cp; cs = sp; break;
  }
  *s_out = (float)sn; *c_out = (float)cs;
}

__global__ __launch_bounds__(256) void k_orb_desc(const uint8_t* __restrict__ blur, const LevelDesc* __restrict__ levels, const int* __restrict__ sel, int n,
                                                  const float* __restrict__ dx, const float* __restrict__ dy, const float* __restrict__ dang,
                                                  const int* __restrict__ dlvl, const OrbPattern* __restrict__ pat, uint8_t* __restrict__ desc) {
  const int kp = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (kp >= n) return;
  const int id = sel[kp];
  const LevelDesc L = levels[dlvl[id]];
  const int cx = (int)dx[id] + (kEdge - 3), cy = (int)dy[id] + (kEdge - 3);       // cvRound of integer-valued level coordinates
  const float factorPI = (float)(3.1415926535897932384626433832795 / 180.f);
  float a, b;
  sincos_exact_dev(dang[id] * factorPI, &b, &a);
  const uint8_t* center = blur + L.off_blur + (size_t)cy * L.w + cx;
  const int4 q = pat->q[lane];                      // 16 signed bytes: (x0,y0,x1,y1) of 4 tests
  const int words[4] = {q.x, q.y, q.z, q.w};
  int nib = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float x0 = (float)(signed char)(words[t] & 0xff), y0 = (float)(signed char)((words[t] >> 8) & 0xff);
    const float x1 = (float)(signed char)((words[t] >> 16) & 0xff), y1 = (float)(signed char)((words[t] >> 24) & 0xff);
    const int t0 = center[__float2int_rn(x0 * b + y0 * a) * L.w + __float2int_rn(x0 * a - y0 * b)];
    const int t1 = center[__float2int_rn(x1 * b + y1 * a) * L.w + __float2int_rn(x1 * a - y1 * b)];
    nib |= (t0 < t1) << t;
  }
  const int hi = __shfl_down(nib, 1, 64);
  if ((lane & 1) == 0) desc[(size_t)kp * 32 + (lane >> 1)] = (uint8_t)(nib | (hi << 4));
}

// The keypoints of the last extraction as vdo_orb_extract_end returns them, written on the device for the matcher: x, y of level 0 (the host's
// arithmetic: candidate + 13 as one fp32 add, then - above level 0 - one fp32 multiply by the level's scale) and the octave, in output order.
struct OrbScales { float v[16]; };
__global__ __launch_bounds__(256) void k_orb_match_pos(const int* __restrict__ sel, int n, const float* __restrict__ dx, const float* __restrict__ dy,
                                                       const int* __restrict__ dlvl, OrbScales sc, float* __restrict__ ox, float* __restrict__ oy,
                                                       int32_t* __restrict__ ooct) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int id = sel[i], l = dlvl[id];
  float x = dx[id] + (float)(kEdge - 3), y = dy[id] + (float)(kEdge - 3);
  if (l != 0) { x = x * sc.v[l]; y = y * sc.v[l]; }
  ox[i] = x; oy[i] = y; ooct[i] = l;
}

// all pyramid levels in ONE launch: blockIdx.x -> (level, tile) through the per-level tile offsets
struct BlurTiles { int off[17]; int tiles_x[16]; };
__global__ __launch_bounds__(256) void k_blur7_all(const uint8_t* __restrict__ pyr, const LevelDesc* __restrict__ levels, int n_levels, BlurTiles bt, Blur7 K,
                                                   uint8_t* __restrict__ blur) {
  int lvl = 0;
  while (lvl + 1 < n_levels && (int)blockIdx.x >= bt.off[lvl + 1]) ++lvl;
  const LevelDesc L = levels[lvl];
  const int t = blockIdx.x - bt.off[lvl], by = t / bt.tiles_x[lvl], bx = t - by * bt.tiles_x[lvl];
  const uint8_t* __restrict__ src = pyr + L.off_inner;
  uint8_t* __restrict__ dst = blur + L.off_blur;
  const int w = L.w, h = L.h, sstride = L.bw;
  __shared__ uint8_t tile[38][40];
  __shared__ int hbuf[38][32];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8 threads, tile 32x32
  const int x0 = bx * 32, y0 = by * 32;
  for (int i = threadIdx.x; i < 38 * 38; i += 256) {
    const int yy = i / 38, xx = i - yy * 38;
    tile[yy][xx] = src[(size_t)reflect101(y0 + yy - 3, h) * sstride + reflect101(x0 + xx - 3, w)];
  }
  __syncthreads();
  for (int yy = ty; yy < 38; yy += 8) {
    int a = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) a += K.k[i] * tile[yy][tx + i];
    hbuf[yy][tx] = a;
  }
  __syncthreads();
  for (int yy = ty; yy < 32; yy += 8) {
    const int x = x0 + tx, y = y0 + yy;
    if (x >= w || y >= h) continue;
    int a = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) a += K.k[i] * hbuf[yy + i][tx];
    const int v = (a + (1 << 15)) >> 16;
    dst[(size_t)y * w + x] = (uint8_t)min(255, max(0, v));
  }
}

// --------------------------------------------------------------------------- host: quadtree (K5)
struct QNode {
  int ULx, ULy, URx, URy, BLx, BLy, BRx, BRy;
  int b = 0, e = 0;         // keys = idx[b, e): every node owns a contiguous run of the shared index array
  int prev = -1, next = -1; // intrusive list (front = head)
  bool noMore = false;
};

// DistributeOctTree (reference src/ORBextractor.cc:528-752, DivideNode :470-526) with an index-based
// intrusive list (same traversal/insert order as the reference's std::list: children are pushed to the
// FRONT, parents erased).  Ties in the "expand largest first" phase are broken by node creation order
// (the reference breaks them by heap address).  Allocation-free in steady state: the keys
// of a node are a run of one index array, DivideNode is a stable 4-way partition of that run
// (children keep the parent's key order, like the reference's push_back loops), buffers are reused
// across levels and frames.
class QuadTree {
 public:
  // candidates as SoA (x, y relative to the level's (minX, minY); resp)
  void run(const float* cx, const float* cy, const float* cresp, int ncand, int minX, int maxX, int minY, int maxY, int N, std::vector<int>& out) {
    out.clear();
    if (ncand <= 0) return;
    x = cx; y = cy; resp = cresp;
    nodes.clear(); head = tail = -1; count = 0;
    idx.resize(ncand); tmp.resize(ncand); cls.resize(ncand);
    const int nIni = (int)std::round((float)(maxX - minX) / (maxY - minY));
    const float hX = (float)(maxX - minX) / nIni;
    // initial nodes: stable bucket sort of the candidates by column strip
    ini_cnt.assign(nIni + 1, 0);
    for (int k = 0; k < ncand; ++k) { const int q = (int)(x[k] / hX); cls[k] = q; ini_cnt[q + 1]++; }
    for (int i = 0; i < nIni; ++i) ini_cnt[i + 1] += ini_cnt[i];
    ini_fill.assign(ini_cnt.begin(), ini_cnt.end() - 1);
    for (int k = 0; k < ncand; ++k) idx[ini_fill[cls[k]]++] = k;
    for (int i = 0; i < nIni; ++i) {
      QNode n;
      n.ULx = (int)(hX * (float)i); n.ULy = 0; n.URx = (int)(hX * (float)(i + 1)); n.URy = 0;
      n.BLx = n.ULx; n.BLy = maxY - minY; n.BRx = n.URx; n.BRy = maxY - minY;
      n.b = ini_cnt[i]; n.e = ini_cnt[i + 1];
      push_back(n);
    }
    for (int it = head; it != -1;) {
      const int nx = nodes[it].next;
      const int sz = nodes[it].e - nodes[it].b;
      if (sz == 1) nodes[it].noMore = true;
      else if (sz == 0) erase(it);
      it = nx;
    }
    bool finish = false;
    while (!finish) {
      int prevSize = count;
      int nToExpand = 0;
      sizeAndNode.clear();
      for (int it = head; it != -1;) {
        if (nodes[it].noMore) { it = nodes[it].next; continue; }
        const int nx = nodes[it].next;
        divide_and_add(it, &nToExpand);
        erase(it);
        it = nx;
      }
      if (count >= N || count == prevSize) finish = true;
      else if (count + nToExpand * 3 > N) {
        while (!finish) {
          prevSize = count;
          prevSN.swap(sizeAndNode);
          sizeAndNode.clear();
          std::sort(prevSN.begin(), prevSN.end());
          for (int j = (int)prevSN.size() - 1; j >= 0; --j) {
            divide_and_add(prevSN[j].second, nullptr);
            erase(prevSN[j].second);
            if (count >= N) break;
          }
          if (count >= N || count == prevSize) finish = true;
        }
      }
    }
    for (int it = head; it != -1; it = nodes[it].next) {
      const QNode& n = nodes[it];
      int best = idx[n.b];
      float mr = resp[best];
      for (int k = n.b + 1; k < n.e; ++k) if (resp[idx[k]] > mr) { best = idx[k]; mr = resp[best]; }
      out.push_back(best);
    }
  }

 private:
  const float *x = nullptr, *y = nullptr, *resp = nullptr;
  std::vector<int> idx, tmp, ini_cnt, ini_fill;
  std::vector<int> cls;                                   // initial column (nIni > 255 on wide strips) or quadrant of a key
  std::vector<QNode> nodes;
  std::vector<std::pair<int, int>> sizeAndNode, prevSN;   // (size, node id); id order == creation order
  int head = -1, tail = -1, count = 0;
  int push_back(const QNode& n) {
    nodes.push_back(n);
    const int id = (int)nodes.size() - 1;
    nodes[id].prev = tail; nodes[id].next = -1;
    if (tail != -1) nodes[tail].next = id; else head = id;
    tail = id; ++count;
    return id;
  }
  int push_front(const QNode& n) {
    nodes.push_back(n);
    const int id = (int)nodes.size() - 1;
    nodes[id].prev = -1; nodes[id].next = head;
    if (head != -1) nodes[head].prev = id; else tail = id;
    head = id; ++count;
    return id;
  }
  void erase(int id) {
    const QNode n = nodes[id];
    if (n.prev != -1) nodes[n.prev].next = n.next; else head = n.next;
    if (n.next != -1) nodes[n.next].prev = n.prev; else tail = n.prev;
    --count;
  }
  void divide_and_add(int id, int* nToExpand) {
    QNode c[4];
    const QNode n = nodes[id];
    const int halfX = (int)std::ceil((float)(n.URx - n.ULx) / 2), halfY = (int)std::ceil((float)(n.BRy - n.ULy) / 2);
    QNode &n1 = c[0], &n2 = c[1], &n3 = c[2], &n4 = c[3];
    n1.ULx = n.ULx; n1.ULy = n.ULy; n1.URx = n.ULx + halfX; n1.URy = n.ULy; n1.BLx = n.ULx; n1.BLy = n.ULy + halfY; n1.BRx = n.ULx + halfX; n1.BRy = n.ULy + halfY;
    n2.ULx = n1.URx; n2.ULy = n1.URy; n2.URx = n.URx; n2.URy = n.URy; n2.BLx = n1.BRx; n2.BLy = n1.BRy; n2.BRx = n.URx; n2.BRy = n.ULy + halfY;
    n3.ULx = n1.BLx; n3.ULy = n1.BLy; n3.URx = n1.BRx; n3.URy = n1.BRy; n3.BLx = n.BLx; n3.BLy = n.BLy; n3.BRx = n1.BRx; n3.BRy = n.BLy;
    n4.ULx = n3.URx; n4.ULy = n3.URy; n4.URx = n2.BRx; n4.URy = n2.BRy; n4.BLx = n3.BRx; n4.BLy = n3.BRy; n4.BRx = n.BRx; n4.BRy = n.BRy;
    int cnt[4] = {0, 0, 0, 0};
    const float sx = (float)n1.URx, sy = (float)n1.BRy;      // kp.pt.x < n1.UR.x compares float with int -> float
    for (int k = n.b; k < n.e; ++k) {
      const int ki = idx[k];
      const int q = (x[ki] < sx) ? ((y[ki] < sy) ? 0 : 2) : ((y[ki] < sy) ? 1 : 3);
      cls[k] = q; ++cnt[q];
    }
    int cur[4];
    cur[0] = n.b; cur[1] = cur[0] + cnt[0]; cur[2] = cur[1] + cnt[1]; cur[3] = cur[2] + cnt[2];
    for (int q = 0; q < 4; ++q) { c[q].b = cur[q]; c[q].e = cur[q] + cnt[q]; c[q].noMore = cnt[q] == 1; }
    for (int k = n.b; k < n.e; ++k) tmp[cur[cls[k]]++] = idx[k];
    std::memcpy(idx.data() + n.b, tmp.data() + n.b, sizeof(int) * (size_t)(n.e - n.b));
    for (int q = 0; q < 4; ++q) {
      if (cnt[q] == 0) continue;
      const int nid = push_front(c[q]);
      if (cnt[q] > 1) {
        if (nToExpand) ++*nToExpand;
        sizeAndNode.push_back(std::make_pair(cnt[q], nid));
      }
    }
  }
};

// ------------------------------------------------------------------------- device: quadtree (K5)
// k_quadtree: QuadTree::run above, one workgroup of kQtThreads per pyramid level, behind k_compact on the extractor's stream.  The
// node list is an array in list order (LDS, two buffers); the keys are a permutation of the level's candidates (two buffers; LDS up to
// kQtLdsKeys candidates, the level's global scratch above) in which every node owns the run [b, e), plus the list index of the owning
// node per key.  One round =
//   A  keys: quadrant of every key of an expandable node, exclusive prefix of the four quadrant counts (4 x 16 bit in one word)
//      over the key positions -> P[k]; a node's child sizes are P[e] - P[b], a key's place in its child P[k] - P[b]: the stable
//      4-way partition of every node at once;
//   B  nodes: processing rank.  Full round: the expandable nodes in list order.  Final phase: by (size, creation id) descending,
//      rank by counting (what the host's sort + walk from the back visits);
//   C  prefix over the ranks of "non-empty children" -> how many are processed (final phase: up to the first prefix whose count
//      reaches N), where each parent's children land (children of the LAST processed parent first, each n4..n1) and their creation ids;
//   D  nodes: children and the untouched nodes (behind all children, old order) into the other node buffer;
//   E  keys: scatter into the other key buffer.
// Only integer arithmetic (the candidates' coordinates are integer-valued floats, so the host's float comparisons are integer comparisons
// here; the strip of a key is the host's float division): the host's list, bit for bit.  Bounds fixed before the launch: kQtMaxRounds rounds,
// N + 3 nodes (<= kQtMaxNodes), the level's share of the key scratch (<= kQtMaxCand keys: 16-bit quadrant counts).  On any of them the
// workgroup writes a status word and stops; vdo_orb_extract_end then runs QuadTree::run for that level.  No workgroup waits for another.
constexpr int kQtThreads = 1024, kQtMaxNodes = 1024, kQtLdsKeys = 4096, kQtMaxCand = 32768, kQtMaxRounds = 48;
enum { kQtOk = 0, kQtHostLevel = 1, kQtCandOverflow = 2, kQtNodeOverflow = 3, kQtRoundCap = 4, kQtBadStrip = 5 };
struct QtDesc {
  int on_device;        // 0: the level takes the host tree (capacity, checked in vdo_orb_create)
  int N, nIni, H;       // nfeat of the level, initial column strips, maxY - minY
  int node_cap;         // N + 3
  int cand_cap;         // keys the level's scratch holds
  int koff;             // scratch offset of the level in keys
  int out_off;          // first id of the level in the id rows (node_cap ids per level)
  float hX;             // strip width, (float)(maxX - minX) / nIni as on the host
  float scale;          // mvScaleFactor of the level
  int pad[2];
};
typedef unsigned long long qt_u64;

__device__ __forceinline__ int qt_field(qt_u64 v, int q) { return (int)((v >> (16 * q)) & 0xffffu); }
__device__ __forceinline__ int qt_nchild(qt_u64 v) { return (qt_field(v, 0) != 0) + (qt_field(v, 1) != 0) + (qt_field(v, 2) != 0) + (qt_field(v, 3) != 0); }
__device__ __forceinline__ int qt_nexp(qt_u64 v) { return (qt_field(v, 0) > 1) + (qt_field(v, 1) > 1) + (qt_field(v, 2) > 1) + (qt_field(v, 3) > 1); }

// exclusive prefix of v over the workgroup's threads; total: the sum over all of them.  s_w: 16 words.
__device__ __forceinline__ qt_u64 qt_block_scan(qt_u64 v, qt_u64* s_w, qt_u64& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  qt_u64 inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const qt_u64 u = __shfl_up(inc, off, 64); if (lane >= off) inc += u; }
  __syncthreads();
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  qt_u64 base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kQtThreads / 64; ++w) { const qt_u64 p = s_w[w]; if (w < wv) base += p; tot += p; }
  total = tot;
  return base + inc - v;
}

__global__ __launch_bounds__(kQtThreads) void k_quadtree(const QtDesc* __restrict__ qd, const int* __restrict__ level_cnt,
                                                         const float* __restrict__ ox, const float* __restrict__ oy, const float* __restrict__ oresp,
                                                         uint32_t* wi, qt_u64* wp, int* __restrict__ dsel, int* __restrict__ dhdr,
                                                         int* __restrict__ hsel, int* __restrict__ hhdr) {
  __shared__ uint32_t s_nx[2][kQtMaxNodes], s_ny[2][kQtMaxNodes];     // x0 | x1 << 16, y0 | y1 << 16  (UL.x, UR.x, UL.y, BR.y)
  __shared__ int s_b[2][kQtMaxNodes], s_e[2][kQtMaxNodes], s_cid[2][kQtMaxNodes];
  __shared__ qt_u64 s_qc[kQtMaxNodes];                                // child sizes of an expandable node
  __shared__ qt_u64 s_sc[kQtMaxNodes];                                // by rank: inclusive prefix of non-empty children | expandable children << 32
  __shared__ int s_rank[kQtMaxNodes], s_order[kQtMaxNodes], s_nb[kQtMaxNodes];
  __shared__ qt_u64 s_w[kQtThreads / 64];
  __shared__ int s_m;
  // the keys of a level with at most kQtLdsKeys candidates (otherwise the same arrays in the level's global scratch)
  __shared__ uint32_t s_xy[kQtLdsKeys];
  __shared__ uint16_t s_idx[2][kQtLdsKeys], s_kn[2][kQtLdsKeys];
  __shared__ qt_u64 s_P[kQtLdsKeys + 1];
  __shared__ uint8_t s_resp[kQtLdsKeys];                              // FAST scores are integers below 256
  const int l = blockIdx.x, t = threadIdx.x;
  const QtDesc D = qd[l];
  auto finish = [&](int status, int count) { if (t == 0) { dhdr[l] = hhdr[l] = count; dhdr[16 + l] = hhdr[16 + l] = status; } };
  if (!D.on_device) { finish(kQtHostLevel, 0); return; }
  int pos = 0;
  for (int q = 0; q < l; ++q) pos += level_cnt[q];
  const int n = level_cnt[l];
  if (n > D.cand_cap) { finish(kQtCandOverflow, 0); return; }
  if (n <= 0) { finish(kQtOk, 0); return; }
  const float *x = ox + pos, *y = oy + pos, *resp = oresp + pos;
  const int KC = (n + kQtThreads - 1) / kQtThreads;
  const int k0 = min(t * KC, n), k1 = min(k0 + KC, n);                // this thread's key positions
  const int N = D.N, cap = D.node_cap;

  // xy: x | y << 16 of candidate id (the candidates are integer-valued floats, k_compact: x < (float)m is the integer comparison);
  // idA / idB: candidate ids in list order, two buffers; knA / knB: list index of the node that owns the key; P: n + 1 prefix words
  const bool lds_keys = n <= kQtLdsKeys;
  auto run = [&](uint32_t* xy, uint16_t* idA, uint16_t* idB, uint16_t* knA, uint16_t* knB, qt_u64* P) __attribute__((always_inline)) {
    // initial nodes: stable bucket sort by column strip, four strips per pass; buffer 1 holds all nIni strips, buffer 0 the non-empty ones
    {
      int bad = 0;
      for (int k = k0; k < k1; ++k) {
        const float fx = x[k], fy = y[k];
        const int s = (int)__fdiv_rn(fx, D.hX);
        bad |= (s < 0 || s >= D.nIni || !(fx >= 0.f && fx < 65536.f && fy >= 0.f && fy < 65536.f));
        xy[k] = (uint32_t)(int)fx | ((uint32_t)(int)fy << 16);
        if (lds_keys) { const float r = resp[k]; bad |= !(r >= 0.f && r < 256.f); s_resp[k] = (uint8_t)(int)r; }
      }
      if (__syncthreads_or(bad)) { finish(kQtBadStrip, 0); return; }
      int base = 0;
      for (int g = 0; g < D.nIni; g += 4) {
        qt_u64 a = 0;
        for (int k = k0; k < k1; ++k) { const int s = (int)__fdiv_rn((float)(xy[k] & 0xffffu), D.hX) - g; if (s >= 0 && s < 4) a += 1ull << (16 * s); }
        qt_u64 tot;
        qt_u64 ex = qt_block_scan(a, s_w, tot);
        int st[5];
        st[0] = base;
        for (int j = 0; j < 4; ++j) st[j + 1] = st[j] + qt_field(tot, j);
        for (int k = k0; k < k1; ++k) {
          const int s = (int)__fdiv_rn((float)(xy[k] & 0xffffu), D.hX) - g;
          if (s < 0 || s >= 4) continue;
          const int p = st[s] + qt_field(ex, s);
          if ((unsigned)p < (unsigned)n) { idA[p] = (uint16_t)k; knA[p] = (uint16_t)(g + s); }
          ex += 1ull << (16 * s);
        }
        if (t < 4 && g + t < D.nIni) {
          const int i = g + t;
          const int sx0 = (int)(D.hX * (float)i), sx1 = (int)(D.hX * (float)(i + 1));
          s_nx[1][i] = (uint32_t)sx0 | ((uint32_t)sx1 << 16); s_ny[1][i] = (uint32_t)D.H << 16;
          s_b[1][i] = st[t]; s_e[1][i] = st[t + 1];
        }
        base = st[4];
      }
      __syncthreads();
    }
    int count;
    {
      const int NC = (D.nIni + kQtThreads - 1) / kQtThreads;
      const int i0 = min(t * NC, D.nIni), i1 = min(i0 + NC, D.nIni);
      int a = 0;
      for (int i = i0; i < i1; ++i) a += s_e[1][i] > s_b[1][i];
      qt_u64 tot;
      int ex = (int)qt_block_scan((qt_u64)a, s_w, tot);
      count = (int)tot;
      for (int i = i0; i < i1; ++i) {
        s_nb[i] = ex;
        if (s_e[1][i] > s_b[1][i]) { s_nx[0][ex] = s_nx[1][i]; s_ny[0][ex] = s_ny[1][i]; s_b[0][ex] = s_b[1][i]; s_e[0][ex] = s_e[1][i]; s_cid[0][ex] = i; ++ex; }
      }
      __syncthreads();
      for (int k = k0; k < k1; ++k) knA[k] = (uint16_t)s_nb[knA[k]];
      __syncthreads();
    }
    int c = 0, next_cid = D.nIni;
    bool final_phase = false;
    for (int round = 0;; ++round) {
      if (round >= kQtMaxRounds) { finish(kQtRoundCap, 0); return; }
      const int o = c ^ 1;
      const uint16_t *idc = c ? idB : idA, *knc = c ? knB : knA;
      uint16_t *ido = c ? idA : idB, *kno = c ? knA : knB;
      // A
      {
        auto quadrant = [&](int k) {
          const int i = knc[k];
          if (s_e[c][i] - s_b[c][i] <= 1) return 4;
          const uint32_t nx = s_nx[c][i], ny = s_ny[c][i];
          const int x0 = (int)(nx & 0xffffu), x1 = (int)(nx >> 16), y0 = (int)(ny & 0xffffu), y1 = (int)(ny >> 16);
          const int mx = x0 + ((x1 - x0 + 1) >> 1), my = y0 + ((y1 - y0 + 1) >> 1);      // x0 + ceil((x1 - x0) / 2)
          const uint32_t v = xy[idc[k]];
          const int kx = (int)(v & 0xffffu), ky = (int)(v >> 16);
          return (kx < mx) ? ((ky < my) ? 0 : 2) : ((ky < my) ? 1 : 3);
        };
        qt_u64 a = 0;
        uint32_t qs = 0;                                 // the quadrants of up to 8 keys, 4 bits each (more keys per thread: computed again)
        for (int k = k0; k < k1; ++k) { const int q = quadrant(k); if (q < 4) a += 1ull << (16 * q); if (k - k0 < 8) qs |= (uint32_t)q << (4 * (k - k0)); }
        qt_u64 tot;
        qt_u64 ex = qt_block_scan(a, s_w, tot);
        for (int k = k0; k < k1; ++k) { P[k] = ex; const int q = k - k0 < 8 ? (int)((qs >> (4 * (k - k0))) & 15u) : quadrant(k); if (q < 4) ex += 1ull << (16 * q); }
        if (t == 0) P[n] = tot;
        __syncthreads();
      }
      // B
      const int NC = (count + kQtThreads - 1) / kQtThreads;
      const int i0 = min(t * NC, count), i1 = min(i0 + NC, count);
      int E;
      {
        int a = 0;
        for (int i = i0; i < i1; ++i) {
          const int b = s_b[c][i], e = s_e[c][i];
          const bool ex = e - b > 1;
          s_qc[i] = ex ? P[e] - P[b] : 0ull;
          a += ex;
        }
        qt_u64 tot;
        int r = (int)qt_block_scan((qt_u64)a, s_w, tot);
        E = (int)tot;
        if (!final_phase) {
          for (int i = i0; i < i1; ++i) {
            if (s_e[c][i] - s_b[c][i] <= 1) { s_rank[i] = -1; continue; }
            s_rank[i] = r; s_order[r] = i; ++r;
          }
        } else {
          // rank = the expandable nodes with a larger (size, creation id): the keys go to s_sc (free until C), every node's count is
          // split over kQtThreads / count threads
          for (int i = i0; i < i1; ++i) {
            const int sz = s_e[c][i] - s_b[c][i];
            s_sc[i] = sz > 1 ? ((qt_u64)sz << 32) | (uint32_t)s_cid[c][i] : 0ull;
            s_rank[i] = sz > 1 ? 0 : -1;
          }
          __syncthreads();
          const int G = max(1, kQtThreads / count), per = kQtThreads / G, part = t % G;
          for (int i = t / G; i < count; i += per) {
            const qt_u64 ki = s_sc[i];
            if (!ki) continue;
            int rk = 0;
#pragma unroll 4
            for (int j = part; j < count; j += G) rk += s_sc[j] > ki;
            if (rk) atomicAdd(&s_rank[i], rk);
          }
          __syncthreads();
          for (int i = i0; i < i1; ++i) if (s_rank[i] >= 0) s_order[s_rank[i]] = i;
        }
        if (t == 0) s_m = E;
        __syncthreads();
      }
      // C
      {
        const int RC = (E + kQtThreads - 1) / kQtThreads;
        const int r0 = min(t * RC, E), r1 = min(r0 + RC, E);
        qt_u64 a = 0;
        for (int r = r0; r < r1; ++r) { const qt_u64 qc = s_qc[s_order[r]]; a += (qt_u64)qt_nchild(qc) | ((qt_u64)qt_nexp(qc) << 32); }
        qt_u64 tot;
        qt_u64 ex = qt_block_scan(a, s_w, tot);
        for (int r = r0; r < r1; ++r) {
          const qt_u64 qc = s_qc[s_order[r]];
          ex += (qt_u64)qt_nchild(qc) | ((qt_u64)qt_nexp(qc) << 32);
          s_sc[r] = ex;
          if (final_phase && count + (int)(ex & 0xffffffffu) - (r + 1) >= N) atomicMin(&s_m, r + 1);
        }
        __syncthreads();
      }
      const int m = s_m;
      const int TC = m > 0 ? (int)(s_sc[m - 1] & 0xffffffffu) : 0, n_to_expand = m > 0 ? (int)(s_sc[m - 1] >> 32) : 0;
      const int new_count = TC + count - m;
      if (new_count > cap) { finish(kQtNodeOverflow, 0); return; }
      // D
      {
        int a = 0;
        for (int i = i0; i < i1; ++i) { const int rk = s_rank[i]; a += !(rk >= 0 && rk < m); }
        qt_u64 tot;
        int u = (int)qt_block_scan((qt_u64)a, s_w, tot);
        for (int i = i0; i < i1; ++i) {
          const int rk = s_rank[i];
          if (!(rk >= 0 && rk < m)) {
            const int p = TC + u++;
            s_nx[o][p] = s_nx[c][i]; s_ny[o][p] = s_ny[c][i]; s_b[o][p] = s_b[c][i]; s_e[o][p] = s_e[c][i]; s_cid[o][p] = s_cid[c][i];
            s_nb[i] = p;
            continue;
          }
          const qt_u64 qc = s_qc[i];
          const int incl = (int)(s_sc[rk] & 0xffffffffu), nch = qt_nchild(qc);
          const int nbase = TC - incl;                  // the children of the parents processed later come first
          s_nb[i] = nbase;
          const uint32_t nx = s_nx[c][i], ny = s_ny[c][i];
          const int x0 = (int)(nx & 0xffffu), x1 = (int)(nx >> 16), y0 = (int)(ny & 0xffffu), y1 = (int)(ny >> 16);
          const int mx = x0 + ((x1 - x0 + 1) >> 1), my = y0 + ((y1 - y0 + 1) >> 1);
          int b = s_b[c][i], made = 0;
          for (int q = 0; q < 4; ++q) {
            const int sz = qt_field(qc, q);
            if (!sz) continue;
            const int p = nbase + nch - 1 - made;       // n4..n1 in the list
            s_nx[o][p] = (q & 1) ? ((uint32_t)mx | ((uint32_t)x1 << 16)) : ((uint32_t)x0 | ((uint32_t)mx << 16));
            s_ny[o][p] = (q & 2) ? ((uint32_t)my | ((uint32_t)y1 << 16)) : ((uint32_t)y0 | ((uint32_t)my << 16));
            s_b[o][p] = b; s_e[o][p] = b + sz; s_cid[o][p] = next_cid + incl - nch + made;
            b += sz; ++made;
          }
        }
        __syncthreads();
      }
      // E
      for (int k = k0; k < k1; ++k) {
        const int i = knc[k], rk = s_rank[i];
        int nk = k, nn = s_nb[i];
        if (rk >= 0 && rk < m) {
          const qt_u64 qc = s_qc[i], pk = P[k], d = P[k + 1] - pk;
          const int q = (d & 0xffffu) ? 0 : ((d >> 16) & 0xffffu) ? 1 : ((d >> 32) & 0xffffu) ? 2 : 3;
          const int b = s_b[c][i];
          int offq = 0, after = 0;
          for (int j = 0; j < 4; ++j) { const int sz = qt_field(qc, j); if (j < q) offq += sz; else if (j > q) after += sz != 0; }
          nk = b + offq + qt_field(pk, q) - qt_field(P[b], q);
          nn += after;
        }
        if ((unsigned)nk < (unsigned)n) { ido[nk] = idc[k]; kno[nk] = (uint16_t)nn; }   // (always: a permutation of [0, n))
      }
      __syncthreads();
      c = o; next_cid += TC;
      const int prev = count;
      count = new_count;
      if (count >= N || count == prev) break;
      if (!final_phase && count + 3 * n_to_expand > N) final_phase = true;
    }
    // one keypoint per node, list order: the largest response, the first of equals
    const uint16_t* idc = c ? idB : idA;
    for (int i = t; i < count; i += kQtThreads) {
      const int b = s_b[c][i], e = s_e[c][i];
      int best = idc[b];
      if (lds_keys) {
        int mr = s_resp[best];
        for (int k = b + 1; k < e; ++k) { const int ki = idc[k], r = s_resp[ki]; if (r > mr) { best = ki; mr = r; } }
      } else {
        float mr = resp[best];
        for (int k = b + 1; k < e; ++k) { const int ki = idc[k]; const float r = resp[ki]; if (r > mr) { best = ki; mr = r; } }
      }
      hsel[D.out_off + i] = best; dsel[D.out_off + i] = pos + best;
    }
    finish(kQtOk, count);
  };
  if (n <= kQtLdsKeys) run(s_xy, s_idx[0], s_idx[1], s_kn[0], s_kn[1], s_P);
  else {
    uint32_t* const w0 = wi + 3 * (size_t)D.koff;       // xy | ids (2 x 16 bit) | nodes (2 x 16 bit), cand_cap words each
    uint16_t* const h0 = (uint16_t*)(w0 + D.cand_cap);
    run(w0, h0, h0 + D.cand_cap, h0 + 2 * (size_t)D.cand_cap, h0 + 3 * (size_t)D.cand_cap, wp + D.koff + l);
  }
}

// The rows of the keypoints k_quadtree selected, as vdo_orb_extract returns them (x, y in level-0 pixels, response, IC_Angle), straight to the mapped
// block: half a wave per keypoint slot, one patch row per lane, all 31 bytes of the row loaded at once (the patch lies inside the bordered level).
__global__ __launch_bounds__(256) void k_qt_rows(const QtDesc* __restrict__ qd, int n_levels, const int* __restrict__ dhdr, const int* __restrict__ dsel,
                                                 const float* __restrict__ ox, const float* __restrict__ oy, const float* __restrict__ oresp,
                                                 const uint8_t* __restrict__ pyr, const LevelDesc* __restrict__ levels, UMax um, float* __restrict__ hrows, int row_pitch) {
  const int lane = threadIdx.x & 31;
  const int slot = (blockIdx.x * 256 + threadIdx.x) >> 5;
  int l = -1;
  for (int q = 0; q < n_levels; ++q) { const int off = qd[q].out_off; if (qd[q].on_device && slot >= off && slot < off + qd[q].node_cap) l = q; }
  const bool valid = l >= 0 && dhdr[16 + l] == kQtOk && slot - qd[l].out_off < dhdr[l];
  int m10 = 0, m01 = 0, kx = 0, ky = 0, dense = 0;
  if (valid) {
    dense = dsel[slot];
    kx = (int)ox[dense]; ky = (int)oy[dense];
    if (lane < 31) {
      const LevelDesc L = levels[l];
      const int v = lane - kHalfPatch;
      const int d = um.v[v < 0 ? -v : v];
      const uint8_t* row = pyr + L.off_inner + (size_t)(ky + (kEdge - 3) + v) * L.bw + (kx + (kEdge - 3));
      int px[kPatch];
#pragma unroll
      for (int u = 0; u < kPatch; ++u) px[u] = row[u - kHalfPatch];
      int rs = 0;
#pragma unroll
      for (int u = 0; u < kPatch; ++u) { const int uu = u - kHalfPatch; const int p = (uu >= -d && uu <= d) ? px[u] : 0; m10 += uu * p; rs += p; }
      m01 = v * rs;
    }
  }
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) { m10 += __shfl_down(m10, off, 32); m01 += __shfl_down(m01, off, 32); }
  if (valid && lane == 0) {
    const float ang = fast_atan2_dev((float)m01, (float)m10);
    float fx = (float)kx + (float)(kEdge - 3), fy = (float)ky + (float)(kEdge - 3);
    if (l != 0) { const float sc = qd[l].scale; fx = fx * sc; fy = fy * sc; }
    float* r = hrows + slot;
    r[0] = fx; r[row_pitch] = fy; r[2 * (size_t)row_pitch] = oresp[dense]; r[3 * (size_t)row_pitch] = ang;
  }
}

}  // namespace vdo

using namespace vdo;

struct vdo_orb {
  vdo_ctx* ctx = nullptr;
  vdo_orb_params prm{};
  int w = 0, h = 0, ncells = 0;
  int max_kp = 0;                // vdo_orb_max_keypoints
  int cell_cap = 1;              // candidates one FAST cell can have: row pitch of the per-cell candidate lists
  std::vector<LevelDesc> levels;
  std::vector<CellDesc> cells;
  std::vector<int> cell_level, nfeat;
  std::vector<float> scale;
  UMax um{};
  Blur7 blur{};
  PyrDesc pyr{};                 // cascaded pyramid launches (k_pyramid_all); n_levels == 0: level-by-level launches
  PyrDesc pyr2{};                // second cascade (upper levels from the top level of the first); lv1 == lv0: not used
  // device
  std::vector<void*> allocs;
  uint8_t *d_src = nullptr, *d_pyr = nullptr, *d_blur = nullptr;
  LevelDesc* d_levels = nullptr; CellDesc* d_cells = nullptr; int* d_cell_level = nullptr;
  int *d_cnt = nullptr, *d_offs = nullptr, *d_level_cnt = nullptr; uint32_t* d_pack = nullptr;
  float *d_x = nullptr, *d_y = nullptr, *d_resp = nullptr, *d_ang = nullptr; int* d_lvl = nullptr;
  int64_t pyr_bytes = 0, blur_bytes = 0;
  int dense_cap = 0;
  // K8 (on request): dense ids of the keypoints of the last extraction, device pattern / selection / descriptor rows
  std::vector<int> sel_dense;
  OrbPattern* d_pat = nullptr; int* d_sel = nullptr; uint8_t* d_desc = nullptr; int desc_cap = 0;
  // what the matcher reads of the last extraction (orb_match_view): d_desc holds its descriptors (desc_ready), m_x / m_y / m_oct its level-0 positions
  // and octaves in output order (pos_ready).  A new extraction clears both flags.
  bool desc_ready = false, pos_ready = false;
  float *m_x = nullptr, *m_y = nullptr; int32_t* m_oct = nullptr; int match_cap = 0;
  // mapped pinned staging: [32 ints: level counts, total, largest cell count][4: x, y, resp, angle][dense_cap].  Split path (default): k_compact writes the
  // header and the x / y / resp rows, k_angle the angle row, straight into it (d_pin: its device address).  VDO_ORB_FUSED_ANGLE=1
  // (fused_angle, read in vdo_orb_create): k_compact_angle, then the header and the first kSpecCand columns of the rows are copied
  // (all of them, in _end, for a frame with more candidates than that).
  float* h_pin = nullptr; float* d_pin = nullptr;
  bool fused_angle = false;
  // host view of the last extraction (pointers into the pinned staging)
  const float *hx = nullptr, *hy = nullptr, *hresp = nullptr, *hang = nullptr; std::vector<int> hlevel_cnt;
  int n_cand = 0;
  QuadTree qt[16];                                    // one per level: buffers reused across frames
  std::vector<int> sel[16];
  std::unique_ptr<LevelPool> pool;                    // helpers for the per-level host quadtrees (VDO_ORB_THREADS, default 3); not started with the device tree
  // device quadtree (k_quadtree; off with VDO_ORB_HOST_TREE=1 or VDO_ORB_FUSED_ANGLE=1).  The mapped block continues behind the four candidate rows with
  // [16 keypoint counts][16 status words][qt_out ids: level-local candidate ids in list order, level l from qtd[l].out_off][4 rows of qt_out: x, y, response,
  // angle of those keypoints as vdo_orb_extract returns them]; d_qsel / d_qhdr: ids and header resident, ids as dense candidate ids (what k_orb_desc /
  // k_orb_match_pos index with).
  bool dev_tree = false;
  bool ang_queued = false;                            // k_angle of this extraction is on the stream (device tree: only once something asks for the angle row)
  QtDesc qtd[16]; QtDesc* d_qtd = nullptr;
  int qt_out = 0;
  uint32_t* d_qt_i = nullptr; int *d_qsel = nullptr, *d_qhdr = nullptr; qt_u64* d_qt_p = nullptr;
  double ms_device = 0, ms_tree = 0;                  // last extraction: launch..sync, host quadtree
  bool begun = false;                                 // between vdo_orb_extract_begin and _end
  hipEvent_t ev_cand = nullptr;                       // candidates are on the host (the blur stage runs behind it)
  hipEvent_t ev_ang = nullptr;                        // split path: their angles are on the host (k_angle runs behind ev_cand)
  std::chrono::steady_clock::time_point t_begin;
};

extern "C" int vdo_orb_pyramid_launches(const vdo_orb* o) {
  if (!o) return set_error(VDO_ERR_INVALID, "null handle");
  return o->pyr.n_levels ? (o->pyr2.lv1 > o->pyr2.lv0 ? 2 : 1) : (int)o->levels.size();
}

extern "C" int vdo_orb_max_keypoints(const vdo_orb* o, int* n) {
  if (!o || !n) return set_error(VDO_ERR_INVALID, "vdo_orb_max_keypoints: null argument");
  *n = o->max_kp;
  return VDO_OK;
}

extern "C" int vdo_orb_last_keypoints(const vdo_orb* o, int* n) {
  if (!o || !n) return set_error(VDO_ERR_INVALID, "vdo_orb_last_keypoints: null argument");
  *n = (int)o->sel_dense.size();
  return VDO_OK;
}

extern "C" int vdo_orb_destroy(vdo_orb* o) {
  if (!o) return VDO_OK;
  if (o->ctx) ctx_bind(o->ctx);
  for (void* p : o->allocs) hipFree(p);
  if (o->h_pin) hipHostFree(o->h_pin);
  if (o->ev_cand) hipEventDestroy(o->ev_cand);
  if (o->ev_ang) hipEventDestroy(o->ev_ang);
  delete o;
  return VDO_OK;
}

extern "C" int vdo_orb_create(vdo_ctx* ctx, const vdo_orb_params* prm, int w, int h, vdo_orb** out) {
  if (!ctx || !prm || !out || w < 64 || h < 64 || prm->n_levels < 1 || prm->n_levels > 16 || !(prm->scale_factor > 1.f))
    return set_error(VDO_ERR_INVALID, "vdo_orb_create: bad argument");
  int rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  vdo_orb* o = new vdo_orb();
  o->ctx = ctx; o->prm = *prm; o->w = w; o->h = h;
  const int NL = prm->n_levels;
  // scale tables, level sizes (ORBextractor ctor :403-419, ComputePyramid :1116-1117)
  o->scale.resize(NL);
  o->scale[0] = 1.0f;
  for (int i = 1; i < NL; ++i) o->scale[i] = o->scale[i - 1] * prm->scale_factor;
  o->levels.resize(NL);
  int64_t off = 0, boff = 0;
  for (int l = 0; l < NL; ++l) {
    const float inv = 1.0f / o->scale[l];
    LevelDesc& L = o->levels[l];
    L.w = (int)lrintf((float)w * inv); L.h = (int)lrintf((float)h * inv);
    L.bw = L.w + 2 * kEdge; L.bh = L.h + 2 * kEdge;
    L.off = off; L.off_inner = off + (int64_t)kEdge * L.bw + kEdge; L.off_blur = boff;
    off += (int64_t)L.bw * L.bh;
    boff += (int64_t)L.w * L.h;
    if (L.w < 2 * kEdge + 8 || L.h < 2 * kEdge + 8) {        // (L lives in o: the message is formatted first)
      const int e = set_error(VDO_ERR_UNSUPPORTED, "pyramid level %d too small (%dx%d)", l, L.w, L.h);
      delete o;
      return e;
    }
  }
  o->pyr_bytes = off; o->blur_bytes = boff;
  // features per level (:424-435)
  o->nfeat.resize(NL);
  {
    float factor = 1.0f / prm->scale_factor;
    float nd = prm->n_features * (1 - factor) / (1 - (float)std::pow((double)factor, (double)NL));
    int sum = 0;
    for (int l = 0; l < NL - 1; ++l) { o->nfeat[l] = (int)lrintf(nd); sum += o->nfeat[l]; nd *= factor; }
    o->nfeat[NL - 1] = std::max(prm->n_features - sum, 0);
  }
  // FAST cells (:760-796)
  for (int l = 0; l < NL; ++l) {
    const int ncells_before = (int)o->cells.size();
    const LevelDesc& L = o->levels[l];
    const float W = 30;
    const int minBX = kEdge - 3, minBY = minBX, maxBX = L.w - kEdge + 3, maxBY = L.h - kEdge + 3;
    const float width = (float)(maxBX - minBX), height = (float)(maxBY - minBY);
    const int nCols = (int)(width / W), nRows = (int)(height / W);
    if (nCols <= 0 || nRows <= 0) continue;
    const int wCell = (int)std::ceil(width / nCols), hCell = (int)std::ceil(height / nRows);
    for (int i = 0; i < nRows; ++i) {
      const float iniY = (float)(minBY + i * hCell);
      float maxY = iniY + hCell + 6;
      if (iniY >= maxBY - 3) continue;
      if (maxY > maxBY) maxY = (float)maxBY;
      for (int j = 0; j < nCols; ++j) {
        const float iniX = (float)(minBX + j * wCell);
        float maxX = iniX + wCell + 6;
        if (iniX >= maxBX - 6) continue;
        if (maxX > maxBX) maxX = (float)maxBX;
        CellDesc c{l, (int)iniX, (int)iniY, (int)maxX, (int)maxY, j * wCell, i * hCell, 0};
        if (c.x1 - c.x0 > kMaxCellDim || c.y1 - c.y0 > kMaxCellDim) { delete o; return set_error(VDO_ERR_INTERNAL, "FAST cell larger than %d px", kMaxCellDim); }
        // FAST scores pixels 3 px inside the cell, and non-maximum suppression (strict > against all 8 neighbours) never keeps
        // two touching pixels: at most one candidate per 2x2 block of that interior (uniform noise: 184 in a 59x40 cell)
        o->cell_cap = std::max(o->cell_cap, std::max(0, c.x1 - c.x0 - 5) / 2 * (std::max(0, c.y1 - c.y0 - 5) / 2));
        o->cells.push_back(c);
        o->cell_level.push_back(l);
      }
    }
    if ((int)o->cells.size() == ncells_before) continue;      // no cells: no candidates, the level returns no keypoints
    // DistributeOctTree (:535-549) starts from nIni = round(region width / region height) columns, the same float arithmetic
    // as QuadTree::run.  nIni == 0 (a region less than half as wide as it is tall) leaves the reference indexing an empty
    // vector, undefined behaviour: such a level is refused.
    const int nIni = (int)std::round((float)(maxBX - minBX) / (maxBY - minBY));
    if (nIni < 1) {
      const int e = set_error(VDO_ERR_UNSUPPORTED, "vdo_orb_create: pyramid level %d (%dx%d): its keypoint region (%dx%d) is less than half "
                              "as wide as it is tall, the quadtree would start with no node", l, L.w, L.h, maxBX - minBX, maxBY - minBY);
      delete o;
      return e;
    }
    // Keypoints this level can return.  Each DistributeOctTree pass divides nodes (a node with k > 1 keys becomes at most 4
    // non-empty children: +3 at most) and stops as soon as the node count reaches N = nfeat[l]:
    //  - the first pass divides every initial node before it tests: at most 4 nIni nodes;
    //  - a later breadth pass runs only if count + 3 nToExpand <= N held after the pass before it, and it divides exactly
    //    those nToExpand nodes: at most N;
    //  - the "largest first" passes start below N and stop right after the division that reaches N: at most N - 1 + 3.
    // Hence max(4 nIni, N + 2) per level (the reference returns one keypoint per node).
    o->max_kp += std::max(4 * nIni, o->nfeat[l] + 2);
  }
  o->ncells = (int)o->cells.size();
  // fused pyramid: possible when there are at most 8 levels and every cascaded region fits the LDS buffers
  if (NL <= 8 && !std::getenv("VDO_ORB_PYRAMID_LAUNCHES")) {
    // Two cascades: levels [0, split] from the source image, levels (split, NL) from level `split` - a tile of the top level
    // would otherwise recompute a ~140 x 140 source window through seven levels (58 us for the one-launch form, 8 launches x
    // ~6 us level by level; two launches: the deepest cascade is four levels)
    const int split = NL > 5 ? 4 : NL - 1;
    PyrDesc& P = o->pyr;
    P.n_levels = NL; P.base = 0; P.lv0 = 0; P.lv1 = split + 1;
    for (int l = 0; l < NL; ++l) {
      P.w[l] = o->levels[l].w; P.h[l] = o->levels[l].h;
      P.sx[l] = l ? 1. / ((double)o->levels[l].w / o->levels[l - 1].w) : 1.0;
      P.sy[l] = l ? 1. / ((double)o->levels[l].h / o->levels[l - 1].h) : 1.0;
      P.tiles_x[l] = (P.w[l] + 31) / 32;
    }
    PyrDesc& Q = o->pyr2;
    Q = P;
    Q.base = split; Q.lv0 = split + 1; Q.lv1 = NL;
    for (PyrDesc* D : {&P, &Q}) {
      int tot = 0;
      for (int l = 0; l <= NL; ++l) D->tile_off[l] = 0;
      for (int l = D->lv0; l < D->lv1; ++l) { D->tile_off[l] = tot; tot += D->tiles_x[l] * ((D->h[l] + 31) / 32); }
      for (int l = D->lv1; l <= NL; ++l) D->tile_off[l] = tot;
    }
    // widest region any tile needs at any level below it: the kernel's own cascade (same arithmetic) over every tile column / row
    auto src_range = [](int d0, int d1, double scale, int slen, bool clamp_both, int& s0, int& s1) {
      auto tap = [&](int d, int& lo, int& hi) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int si = (int)std::floor(f);
        if (clamp_both) { lo = std::min(std::max(si, 0), slen - 1); hi = std::min(std::max(si + 1, 0), slen - 1); return; }
        if (si < 0) si = 0;
        if (si + 1 >= slen) { lo = hi = slen - 1; return; }
        lo = si; hi = si + 1;
      };
      int a, b;
      tap(d0, s0, a); tap(d1, b, s1);
    };
    int worst = 32;
    for (const PyrDesc* D : {&P, &Q}) {
      for (int l = std::max(D->lv0, D->base + 1); l < D->lv1; ++l) {
        for (int axis = 0; axis < 2; ++axis) {
          const int len = axis ? D->h[l] : D->w[l];
          for (int t0 = 0; t0 < len; t0 += 32) {
            int d0 = t0, d1 = std::min(t0 + 31, len - 1);
            for (int k = l; k > D->base; --k) {
              int s0, s1;
              src_range(d0, d1, axis ? D->sy[k] : D->sx[k], axis ? D->h[k - 1] : D->w[k - 1], axis == 1, s0, s1);
              d0 = s0; d1 = s1;
              worst = std::max(worst, d1 - d0 + 1);
            }
          }
        }
      }
    }
    if (worst > kPyrRegion) P.n_levels = 0;
  }
  // umax (:443-458)
  {
    int* umax = o->um.v;
    int v, v0;
    const int vmax = (int)std::floor(kHalfPatch * std::sqrt(2.f) / 2 + 1);
    const int vmin = (int)std::ceil(kHalfPatch * std::sqrt(2.f) / 2);
    const double hp2 = kHalfPatch * kHalfPatch;
    for (v = 0; v <= vmax; ++v) umax[v] = (int)lrint(std::sqrt(hp2 - v * v));
    for (v = kHalfPatch, v0 = 0; v >= vmin; --v) { while (umax[v0] == umax[v0 + 1]) ++v0; umax[v] = v0; ++v0; }
  }
  // Gaussian kernel 7, sigma 2 -> 8-bit fixed point
  {
    double kd[7], sum = 0;
    for (int i = 0; i < 7; ++i) { const double x = i - 3; kd[i] = std::exp(-0.5 / 4.0 * x * x); sum += kd[i]; }
    for (int i = 0; i < 7; ++i) o->blur.k[i] = (int)lrint((double)(float)(kd[i] / sum) * 256);
  }
  hipStream_t s = ctx->stream;
  auto dev = [&](size_t bytes) -> void* { void* p = nullptr; if (hipMalloc(&p, bytes ? bytes : 8) != hipSuccess) return nullptr; o->allocs.push_back(p); return p; };
  o->dense_cap = o->ncells * o->cell_cap;
  o->d_src = (uint8_t*)dev((size_t)w * h * 4);
  o->d_pyr = (uint8_t*)dev(o->pyr_bytes); o->d_blur = (uint8_t*)dev(o->blur_bytes);
  o->d_levels = (LevelDesc*)dev(sizeof(LevelDesc) * NL); o->d_cells = (CellDesc*)dev(sizeof(CellDesc) * o->ncells);
  o->d_cell_level = (int*)dev(4 * (size_t)o->ncells);
  o->d_pat = (OrbPattern*)dev(sizeof(OrbPattern));
  o->d_cnt = (int*)dev(4 * (size_t)o->ncells); o->d_offs = (int*)dev(4 * ((size_t)o->ncells + 1)); o->d_level_cnt = (int*)dev(4 * 32);
  o->d_pack = (uint32_t*)dev(4 * (size_t)o->dense_cap);
  o->d_x = (float*)dev(4 * (size_t)o->dense_cap * 5);       // x | y | resp | angle | level: rows of one allocation (single strided D2H)
  if (o->d_x) {
    o->d_y = o->d_x + (size_t)o->dense_cap; o->d_resp = o->d_x + 2 * (size_t)o->dense_cap; o->d_ang = o->d_x + 3 * (size_t)o->dense_cap;
    o->d_lvl = (int*)(o->d_x + 4 * (size_t)o->dense_cap);
  }
  o->fused_angle = std::getenv("VDO_ORB_FUSED_ANGLE") != nullptr;
  // K5 on the device unless VDO_ORB_HOST_TREE=1 (the A/B switch) or the fused path (its candidates reach the host by a copy).  A level takes the host
  // tree when its node bound N + 3 exceeds kQtMaxNodes (VDO_ORB_QT_NODE_CAP lowers that, for the tests), when it has more initial strips than that bound,
  // or when its region does not fit the 16-bit node coordinates.
  {
    const char* ht = std::getenv("VDO_ORB_HOST_TREE");
    o->dev_tree = !o->fused_angle && !(ht && ht[0] && std::strcmp(ht, "0") != 0);
    int node_cap_max = kQtMaxNodes;
    if (const char* e = std::getenv("VDO_ORB_QT_NODE_CAP")) node_cap_max = std::max(0, std::min(kQtMaxNodes, std::atoi(e)));
    int koff = 0, out_off = 0;
    bool any = false;
    for (int l = 0; l < 16; ++l) {
      QtDesc& D = o->qtd[l];
      D = QtDesc{};
      if (l >= NL) continue;
      const LevelDesc& L = o->levels[l];
      const int minB = kEdge - 3, maxBX = L.w - kEdge + 3, maxBY = L.h - kEdge + 3;
      int cells_l = 0;
      for (int c : o->cell_level) cells_l += c == l;
      D.N = o->nfeat[l]; D.H = maxBY - minB; D.nIni = 1; D.hX = 1.f; D.scale = o->scale[l];
      if (cells_l) {                                   // (the same float arithmetic as QuadTree::run)
        D.nIni = (int)std::round((float)(maxBX - minB) / (maxBY - minB));
        D.hX = (float)(maxBX - minB) / D.nIni;
      }
      D.node_cap = D.N + 3;
      D.cand_cap = (int)std::min<int64_t>((int64_t)cells_l * o->cell_cap, kQtMaxCand);
      D.koff = koff; D.out_off = out_off;
      D.on_device = o->dev_tree && D.node_cap <= node_cap_max && D.nIni <= D.node_cap && maxBX - minB < 65536 && maxBY - minB < 65536;
      if (!D.on_device) { D.cand_cap = 0; D.node_cap = 0; }
      any = any || D.on_device;
      koff += D.cand_cap; out_off += D.node_cap;
    }
    o->dev_tree = any;
    o->qt_out = out_off;
    if (o->dev_tree) {
      o->d_qtd = (QtDesc*)dev(sizeof(o->qtd));
      o->d_qt_i = (uint32_t*)dev(4 * 3 * (size_t)koff); o->d_qt_p = (qt_u64*)dev(8 * ((size_t)koff + 16));
      o->d_qsel = (int*)dev(4 * (size_t)out_off); o->d_qhdr = (int*)dev(4 * 32);
    }
  }
  if (hipHostMalloc((void**)&o->h_pin, 4 * (32 + 4 * (size_t)o->dense_cap + 32 + 5 * (size_t)o->qt_out), hipHostMallocMapped) != hipSuccess) o->h_pin = nullptr;
  if (o->h_pin && hipHostGetDevicePointer((void**)&o->d_pin, o->h_pin, 0) != hipSuccess) o->d_pin = nullptr;
  for (void* p : o->allocs) if (!p) { vdo_orb_destroy(o); return set_error(VDO_ERR_OOM, "hipMalloc failed"); }
  if (!o->d_lvl || !o->h_pin || !o->d_pin) { vdo_orb_destroy(o); return set_error(VDO_ERR_OOM, "hipMalloc failed"); }
  hipMemcpyAsync(o->d_levels, o->levels.data(), sizeof(LevelDesc) * NL, hipMemcpyHostToDevice, s);
  hipMemcpyAsync(o->d_cells, o->cells.data(), sizeof(CellDesc) * o->ncells, hipMemcpyHostToDevice, s);
  hipMemcpyAsync(o->d_cell_level, o->cell_level.data(), 4 * (size_t)o->ncells, hipMemcpyHostToDevice, s);
  static_assert(sizeof(kOrbPattern31) == sizeof(OrbPattern), "256 tests x 4 signed bytes");
  hipMemcpyAsync(o->d_pat, kOrbPattern31, sizeof(OrbPattern), hipMemcpyHostToDevice, s);
  if (o->dev_tree) hipMemcpyAsync(o->d_qtd, o->qtd, sizeof(o->qtd), hipMemcpyHostToDevice, s);
  if (hipStreamSynchronize(s) != hipSuccess) { vdo_orb_destroy(o); return set_error(VDO_ERR_NO_DEVICE, "orb upload failed"); }
  if (hipEventCreateWithFlags(&o->ev_cand, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&o->ev_ang, hipEventDisableTiming) != hipSuccess) {
    vdo_orb_destroy(o);
    return set_error(VDO_ERR_NO_DEVICE, "hipEventCreate failed");
  }
  if (!o->dev_tree) {
    const char* e = std::getenv("VDO_ORB_THREADS");
    const int nw = e ? std::atoi(e) : 3;
    if (nw > 0) o->pool.reset(new LevelPool(std::min(nw, 15)));
  }
  *out = o;
  return VDO_OK;
}

// K5 on the device: k_quadtree behind whatever has put the candidate lists of all levels into d_level_cnt / d_x / d_y / d_resp on the extractor's stream
// (k_compact; vdo_orb_tree_run).  Its counts, status words and ids land in the mapped block behind the four candidate rows and in d_qhdr / d_qsel.
static void orb_queue_tree(vdo_orb* o) {
  int* qh = (int*)(o->d_pin + 32 + 4 * (size_t)o->dense_cap);
  hipLaunchKernelGGL(k_quadtree, dim3(o->prm.n_levels), dim3(kQtThreads), 0, o->ctx->stream, (const QtDesc*)o->d_qtd, (const int*)o->d_level_cnt, (const float*)o->d_x,
                     (const float*)o->d_y, (const float*)o->d_resp, o->d_qt_i, o->d_qt_p, o->d_qsel, o->d_qhdr, qh + 32, qh);
}

// K5 of every level once the candidates (o->hx / hy / hresp, o->hlevel_cnt) and, with the device tree, k_quadtree's block are on the host: o->sel[l] = the
// level's keypoints as ids into its own list, in list order - the device's ids where its status is kQtOk, QuadTree::run otherwise.  on_dev[l] says which;
// returns whether every level ran on the device.
static bool orb_resolve_levels(vdo_orb* o, bool on_dev[16]) {
  const int NL = o->prm.n_levels;
  int lvl_pos[17];
  lvl_pos[0] = 0;
  for (int l = 0; l < NL; ++l) lvl_pos[l + 1] = lvl_pos[l] + o->hlevel_cnt[l];
  const int minB = kEdge - 3;
  const int* qh = (const int*)(o->h_pin + 32 + 4 * (size_t)o->dense_cap);     // device tree: [16 counts][16 status][ids]
  bool all_dev = o->dev_tree;
  for (int l = 0; l < NL; ++l) { on_dev[l] = o->dev_tree && qh[16 + l] == kQtOk && qh[l] >= 0 && qh[l] <= o->qtd[l].node_cap; all_dev = all_dev && on_dev[l]; }
  auto level_task = [&](int l) {
    const LevelDesc& L = o->levels[l];
    const int pos = lvl_pos[l];
    if (on_dev[l]) {
      const int* ids = qh + 32 + o->qtd[l].out_off;
      o->sel[l].assign(ids, ids + qh[l]);
      return;
    }
    o->qt[l].run(o->hx + pos, o->hy + pos, o->hresp + pos, o->hlevel_cnt[l], minB, L.w - kEdge + 3, minB, L.h - kEdge + 3, o->nfeat[l], o->sel[l]);
  };
  if (o->pool) o->pool->run(NL, level_task);
  else for (int l = 0; l < NL; ++l) level_task(l);
  return all_dev;
}

// Device part of operator(): pyramid, blur, FAST cells, compaction + angles.  gray_dev: device, row stride `stride`.
static int orb_device_stage(vdo_orb* o, const uint8_t* gray_dev, int stride) {
  hipStream_t s = o->ctx->stream;
  const int NL = o->prm.n_levels;
  const dim3 tb(32, 8);
  if (o->pyr.n_levels) {
    hipLaunchKernelGGL(k_pyramid_all, dim3(o->pyr.tile_off[o->pyr.n_levels]), dim3(256), 0, s, gray_dev, stride, o->pyr, (const LevelDesc*)o->d_levels, o->d_pyr);
    if (o->pyr2.lv1 > o->pyr2.lv0) {
      const LevelDesc& B = o->levels[o->pyr2.base];
      hipLaunchKernelGGL(k_pyramid_all, dim3(o->pyr2.tile_off[o->pyr2.n_levels]), dim3(256), 0, s, (const uint8_t*)(o->d_pyr + B.off_inner), B.bw, o->pyr2, (const LevelDesc*)o->d_levels, o->d_pyr);
    }
  } else {
    {
      const LevelDesc& L = o->levels[0];
      hipLaunchKernelGGL(k_border_copy, dim3((L.bw + 31) / 32, (L.bh + 7) / 8), tb, 0, s, gray_dev, L.w, L.h, stride, o->d_pyr + L.off, L.bw, L.bh);
    }
    for (int l = 1; l < NL; ++l) {
      const LevelDesc &P = o->levels[l - 1], &L = o->levels[l];
      const double sx = 1. / ((double)L.w / P.w), sy = 1. / ((double)L.h / P.h);
      hipLaunchKernelGGL(k_resize_border, dim3((L.bw + 31) / 32, (L.bh + 7) / 8), tb, 0, s, (const uint8_t*)(o->d_pyr + P.off_inner), P.w, P.h, P.bw,
                         o->d_pyr + L.off, L.w, L.h, sx, sy);
    }
  }
  hipLaunchKernelGGL(k_fast_cells, dim3(o->ncells), dim3(256), 0, s, (const uint8_t*)o->d_pyr, (const LevelDesc*)o->d_levels, (const CellDesc*)o->d_cells,
                     o->prm.ini_th, o->prm.min_th, o->cell_cap, o->d_cnt, o->d_pack);
  if (o->fused_angle) {
    hipLaunchKernelGGL(k_compact_angle, dim3(o->ncells), dim3(256), 0, s, (const uint8_t*)o->d_pyr, (const LevelDesc*)o->d_levels, (const CellDesc*)o->d_cells,
                       (const int*)o->d_cnt, (const int*)o->d_cell_level, o->d_level_cnt, (const uint32_t*)o->d_pack, o->ncells, o->cell_cap, o->um, o->d_x, o->d_y, o->d_resp, o->d_ang, o->d_lvl);
  } else {
    float* rows = o->d_pin + 32;
    const size_t pitch = (size_t)o->dense_cap;
    hipLaunchKernelGGL(k_compact, dim3(o->ncells), dim3(256), 0, s, (const CellDesc*)o->d_cells, (const int*)o->d_cnt, (const int*)o->d_cell_level, o->d_level_cnt,
                       (const uint32_t*)o->d_pack, o->ncells, o->cell_cap, o->d_x, o->d_y, o->d_resp, o->d_lvl, (int*)o->d_pin, rows, rows + pitch, rows + 2 * pitch);
    if (o->dev_tree) {
      int* qh = (int*)(rows + 4 * pitch);
      orb_queue_tree(o);
      hipLaunchKernelGGL(k_qt_rows, dim3((o->qt_out + 7) / 8), dim3(256), 0, s, (const QtDesc*)o->d_qtd, NL, (const int*)o->d_qhdr, (const int*)o->d_qsel, (const float*)o->d_x,
                         (const float*)o->d_y, (const float*)o->d_resp, (const uint8_t*)o->d_pyr, (const LevelDesc*)o->d_levels, o->um, (float*)(qh + 32 + o->qt_out), o->qt_out);
    }
  }
  return VDO_OK;
}

// Split path: K6 behind the event the host waits for; the angle row arrives under the quadtrees and is closed by ev_ang.
static void orb_angle_stage(vdo_orb* o) {
  hipStream_t s = o->ctx->stream;
  // grid-stride over chunks of kAngChunk candidates per wave: 1024 workgroups take 32 k candidates per pass (a KITTI frame has 10-15 k)
  const int chunks = (o->dense_cap + kAngChunk - 1) / kAngChunk;
  hipLaunchKernelGGL(k_angle, dim3(std::max(1, std::min(1024, (chunks + 3) / 4))), dim3(256), 0, s, (const uint8_t*)o->d_pyr, (const LevelDesc*)o->d_levels,
                     (const int*)o->d_level_cnt, o->um, (const float*)o->d_x, (const float*)o->d_y, (const int*)o->d_lvl, o->d_ang, o->d_pin + 32 + 3 * (size_t)o->dense_cap);
  hipEventRecord(o->ev_ang, s);
}

// Device tree: no keypoint needs the angle row of all candidates (k_qt_rows computes the angles of the selected ones), and whatever the caller queues on the
// extractor's stream next would wait behind k_angle.  So it runs on demand: for a level that took the host tree, vdo_orb_get_candidates and the descriptors
// (k_orb_desc reads d_ang).  The pyramid and the dense candidate arrays stay resident until the next vdo_orb_extract_begin.
static void orb_ensure_angles(vdo_orb* o) {
  if (o->fused_angle || o->ang_queued) return;
  orb_angle_stage(o);
  o->ang_queued = true;
}

// K7: the reference blurs every non-empty level (result unused there since BRIEF is commented out, F1).  Nothing downstream
// waits for it, so it is queued BEHIND the copy of the candidates: the host starts the quadtrees ~45 us earlier.
static void orb_blur_stage(vdo_orb* o) {
  hipStream_t s = o->ctx->stream;
  BlurTiles bt{};
  int tot = 0;
  for (int l = 0; l < o->prm.n_levels; ++l) {
    const LevelDesc& L = o->levels[l];
    bt.off[l] = tot; bt.tiles_x[l] = (L.w + 31) / 32;
    tot += bt.tiles_x[l] * ((L.h + 31) / 32);
  }
  bt.off[o->prm.n_levels] = tot;
  hipLaunchKernelGGL(k_blur7_all, dim3(tot), dim3(256), 0, s, (const uint8_t*)o->d_pyr, (const LevelDesc*)o->d_levels, o->prm.n_levels, bt, o->blur, o->d_blur);
}

// operator() in two halves: _begin queues the device stage (pyramid, FAST cells, compaction + angles, blur) and the copy of the
// candidates on the extractor's stream and returns; _end waits for them and runs the quadtrees (K5).  vdo_orb_extract = both.
extern "C" int vdo_orb_extract_begin(vdo_orb* o, const uint8_t* gray, int stride, int src_is_device) {
  if (!o || !gray) return set_error(VDO_ERR_INVALID, "vdo_orb_extract_begin: null argument");
  int rc = ctx_bind(o->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = o->ctx->stream;
  const uint8_t* src = gray;
  int sstride = stride;
  if (!src_is_device) {
    // (a 2-D copy from pageable memory is executed row by row - 3 ms for a KITTI image; contiguous rows go up as one 1-D copy)
    if (stride == o->w) hipMemcpyAsync(o->d_src, gray, (size_t)o->w * o->h, hipMemcpyHostToDevice, s);
    else hipMemcpy2DAsync(o->d_src, o->w, gray, stride, o->w, o->h, hipMemcpyHostToDevice, s);
    src = o->d_src; sstride = o->w;
  }
  o->t_begin = std::chrono::steady_clock::now();
  o->desc_ready = o->pos_ready = false;             // (the dense candidate arrays are overwritten from here on)
  orb_device_stage(o, src, sstride);
  if (o->fused_angle) {
    // candidates -> host: header (level counts + total) and the first kSpecCand columns of the 4 candidate rows the host reads
    const int spec = std::min(kSpecCand, o->dense_cap);
    hipMemcpyAsync(o->h_pin, o->d_level_cnt, 4 * 32, hipMemcpyDeviceToHost, s);
    hipMemcpy2DAsync(o->h_pin + 32, 4 * (size_t)o->dense_cap, o->d_x, 4 * (size_t)o->dense_cap, 4 * (size_t)spec, 4, hipMemcpyDeviceToHost, s);
    hipEventRecord(o->ev_cand, s);
  } else {
    // k_compact has written the header and the x / y / resp rows to the host itself (and k_quadtree, with the device tree, the keypoint ids);
    // the angles of all candidates follow behind the event (device tree: on demand, orb_ensure_angles)
    hipEventRecord(o->ev_cand, s);
    o->ang_queued = false;
    if (!o->dev_tree) orb_ensure_angles(o);
  }
  orb_blur_stage(o);
  o->begun = true;
  return VDO_OK;
}

extern "C" int vdo_orb_extract(vdo_orb* o, const uint8_t* gray, int stride, int src_is_device, vdo_keypoints* out) {
  int rc = vdo_orb_extract_begin(o, gray, stride, src_is_device);
  return rc != VDO_OK ? rc : vdo_orb_extract_end(o, out);
}

extern "C" int vdo_orb_extract_end(vdo_orb* o, vdo_keypoints* out) {
  if (!o || !out) return set_error(VDO_ERR_INVALID, "vdo_orb_extract_end: null argument");
  if (!o->begun) return set_error(VDO_ERR_INVALID, "vdo_orb_extract_end without vdo_orb_extract_begin");
  o->begun = false;
  int rc = ctx_bind(o->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = o->ctx->stream;
  const auto t_begin = o->t_begin;
  int* hdr = (int*)o->h_pin;
  const float* rows = o->h_pin + 32;
  const size_t pitch = (size_t)o->dense_cap;
  if (hipEventSynchronize(o->ev_cand) != hipSuccess) return set_error(VDO_ERR_NO_DEVICE, "orb device stage failed: %s", hipGetErrorString(hipGetLastError()));
  if (hdr[17] > o->cell_cap) {   // cannot happen (vdo_orb_create); k_fast_cells would have dropped the excess without a word
    o->hlevel_cnt.clear(); o->sel_dense.clear();
    return set_error(VDO_ERR_UNSUPPORTED, "vdo_orb_extract: a FAST cell has %d candidates, more than the %d kept per cell", hdr[17], o->cell_cap);
  }
  const int total = hdr[16];
  o->n_cand = total;
  o->hlevel_cnt.assign(hdr, hdr + 16);
  if (o->fused_angle && total > kSpecCand) {           // rare: the speculative copy fell short, fetch all columns
    hipMemcpy2DAsync(o->h_pin + 32, 4 * pitch, o->d_x, 4 * pitch, 4 * (size_t)total, 4, hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess) return set_error(VDO_ERR_NO_DEVICE, "orb D2H failed");
  }
  o->hx = rows; o->hy = rows + pitch; o->hresp = rows + 2 * pitch; o->hang = rows + 3 * pitch;
  const auto t_dev = std::chrono::steady_clock::now();
  // K5 on the host: one quadtree per level (candidates of a level are contiguous: cells are level-major), levels in parallel
  const int NL = o->prm.n_levels;
  int lvl_pos[17];
  lvl_pos[0] = 0;
  for (int l = 0; l < NL; ++l) lvl_pos[l + 1] = lvl_pos[l] + o->hlevel_cnt[l];
  const int minB = kEdge - 3;
  const int* qh = (const int*)(rows + 4 * pitch);     // device tree: [16 counts][16 status][ids][rows of the keypoints]
  bool on_dev[16] = {};
  const bool all_dev = orb_resolve_levels(o, on_dev);
  // split path: the angle row was written under the quadtrees (o->hang and vdo_orb_get_candidates are valid from here on)
  // (device tree: k_qt_rows has written the rows of its keypoints, angle included; the angle row of all candidates is waited for only by a level
  //  that took the host tree, and by vdo_orb_get_candidates)
  if (!all_dev) orb_ensure_angles(o);
  if (!o->fused_angle && !all_dev && hipEventSynchronize(o->ev_ang) != hipSuccess) return set_error(VDO_ERR_NO_DEVICE, "orb angle stage failed: %s", hipGetErrorString(hipGetLastError()));
  int n = 0;
  o->sel_dense.clear();
  for (int l = 0; l < NL; ++l) {
    const int pos = lvl_pos[l];
    const float *cx = o->hx + pos, *cy = o->hy + pos, *cr = o->hresp + pos, *ca = o->hang + pos;
    const int patch = (int)(kPatch * o->scale[l]);
    if (on_dev[l]) {
      const int m = (int)o->sel[l].size();
      if (n + m > out->capacity) return set_error(VDO_ERR_INVALID, "vdo_orb_extract: keypoint capacity %d too small", out->capacity);
      const float* r = (const float*)(qh + 32 + o->qt_out) + o->qtd[l].out_off;
      std::memcpy(out->x + n, r, 4 * (size_t)m); std::memcpy(out->y + n, r + o->qt_out, 4 * (size_t)m);
      std::memcpy(out->response + n, r + 2 * (size_t)o->qt_out, 4 * (size_t)m); std::memcpy(out->angle + n, r + 3 * (size_t)o->qt_out, 4 * (size_t)m);
      for (int k = 0; k < m; ++k) { o->sel_dense.push_back(pos + o->sel[l][k]); out->octave[n + k] = l; out->size[n + k] = (float)patch; }
      n += m;
      continue;
    }
    for (int id : o->sel[l]) {
      o->sel_dense.push_back(pos + id);
      if (n >= out->capacity) return set_error(VDO_ERR_INVALID, "vdo_orb_extract: keypoint capacity %d too small", out->capacity);
      float x = cx[id] + minB, y = cy[id] + minB;
      if (l != 0) { x = x * o->scale[l]; y = y * o->scale[l]; }
      out->x[n] = x; out->y[n] = y; out->response[n] = cr[id]; out->angle[n] = ca[id];
      out->octave[n] = l; out->size[n] = (float)patch;
      ++n;
    }
  }
  out->n = n;
  const auto t_end = std::chrono::steady_clock::now();
  o->ms_device = std::chrono::duration<double, std::milli>(t_dev - t_begin).count();
  o->ms_tree = std::chrono::duration<double, std::milli>(t_end - t_dev).count();
  return VDO_OK;
}

// Queues K8 for the n keypoints of the last extraction on the extractor's stream: o->d_desc holds their descriptors once the stream gets there.
static int orb_queue_descriptors(vdo_orb* o, int n) {
  hipStream_t s = o->ctx->stream;
  if (n > o->desc_cap) {
    const int cap = std::max(n, 4096);
    int* ns = nullptr; uint8_t* nd = nullptr;
    if (hipMalloc((void**)&ns, 4 * (size_t)cap) != hipSuccess || hipMalloc((void**)&nd, 32 * (size_t)cap) != hipSuccess) { if (ns) hipFree(ns); return set_error(VDO_ERR_OOM, "hipMalloc failed"); }
    hipStreamSynchronize(s);
    auto drop = [&](void* p) { if (!p) return; hipFree(p); o->allocs.erase(std::remove(o->allocs.begin(), o->allocs.end(), p), o->allocs.end()); };
    drop(o->d_sel); drop(o->d_desc);
    o->d_sel = ns; o->d_desc = nd; o->desc_cap = cap;
    o->allocs.push_back(ns); o->allocs.push_back(nd);
  }
  // the blurred levels of this extraction are queued on the same stream (orb_blur_stage), the dense candidate arrays are still resident
  orb_ensure_angles(o);
  hipMemcpyAsync(o->d_sel, o->sel_dense.data(), 4 * (size_t)n, hipMemcpyHostToDevice, s);
  hipLaunchKernelGGL(k_orb_desc, dim3((n + 3) / 4), dim3(256), 0, s, (const uint8_t*)o->d_blur, (const LevelDesc*)o->d_levels, (const int*)o->d_sel, n,
                     (const float*)o->d_x, (const float*)o->d_y, (const float*)o->d_ang, (const int*)o->d_lvl, (const OrbPattern*)o->d_pat, o->d_desc);
  o->desc_ready = true;
  return VDO_OK;
}

// K8: descriptors of the keypoints of the last extraction, in their output order.  desc32: host, [n][32].
extern "C" int vdo_orb_descriptors(vdo_orb* o, uint8_t* desc32, int capacity_rows) {
  if (!o || !desc32) return set_error(VDO_ERR_INVALID, "vdo_orb_descriptors: null argument");
  const int n = (int)o->sel_dense.size();
  if (n > capacity_rows) return set_error(VDO_ERR_INVALID, "vdo_orb_descriptors: %d keypoints, room for %d", n, capacity_rows);
  if (n == 0) return VDO_OK;
  int rc = ctx_bind(o->ctx);
  if (rc != VDO_OK) return rc;
  rc = orb_queue_descriptors(o, n);
  if (rc != VDO_OK) return rc;
  hipStream_t s = o->ctx->stream;
  hipMemcpyAsync(desc32, o->d_desc, 32 * (size_t)n, hipMemcpyDeviceToHost, s);
  if (hipStreamSynchronize(s) != hipSuccess) return set_error(VDO_ERR_NO_DEVICE, "orb descriptors: %s", hipGetErrorString(hipGetLastError()));
  return VDO_OK;
}

// operator() with both of its outputs: keypoints and (desc32 != NULL) the 32-byte descriptors, [out->capacity][32]
extern "C" int vdo_orb_extract_desc(vdo_orb* o, const uint8_t* gray, int stride, int src_is_device, vdo_keypoints* out, uint8_t* desc32) {
  int rc = vdo_orb_extract(o, gray, stride, src_is_device, out);
  if (rc != VDO_OK || !desc32) return rc;
  return vdo_orb_descriptors(o, desc32, out->capacity);
}

// What vdo_orb_match_extractors reads (orb_match.hpp): descriptors, level-0 positions and octaves of the last extraction, resident and in output order.
// Everything is queued on the extractor's stream; nothing comes back to the host.
int vdo::orb_match_view(vdo_orb* o, OrbMatchView* v) {
  if (o->begun) return set_error(VDO_ERR_INVALID, "vdo_orb_match_extractors: an extraction is in flight (vdo_orb_extract_begin without _end)");
  int rc = ctx_bind(o->ctx);
  if (rc != VDO_OK) return rc;
  const int n = (int)o->sel_dense.size();
  v->ctx = o->ctx; v->n = n; v->desc = nullptr; v->x = v->y = nullptr; v->octave = nullptr;
  if (n == 0) return VDO_OK;
  hipStream_t s = o->ctx->stream;
  if (!o->desc_ready) {
    rc = orb_queue_descriptors(o, n);          // (also uploads d_sel, which the positions below go through)
    if (rc != VDO_OK) return rc;
  }
  if (!o->pos_ready) {
    if (n > o->match_cap) {
      const int cap = std::max(n, 4096);
      float* nx = nullptr;
      if (hipMalloc((void**)&nx, 12 * (size_t)cap) != hipSuccess) return set_error(VDO_ERR_OOM, "hipMalloc failed");
      hipStreamSynchronize(s);
      if (o->m_x) { hipFree(o->m_x); o->allocs.erase(std::remove(o->allocs.begin(), o->allocs.end(), (void*)o->m_x), o->allocs.end()); }
      o->m_x = nx; o->m_y = nx + cap; o->m_oct = (int32_t*)(nx + 2 * (size_t)cap); o->match_cap = cap;
      o->allocs.push_back(nx);
    }
    OrbScales sc{};
    for (int l = 0; l < o->prm.n_levels; ++l) sc.v[l] = o->scale[l];
    hipLaunchKernelGGL(k_orb_match_pos, dim3((n + 255) / 256), dim3(256), 0, s, (const int*)o->d_sel, n, (const float*)o->d_x, (const float*)o->d_y,
                       (const int*)o->d_lvl, sc, o->m_x, o->m_y, o->m_oct);
    o->pos_ready = true;
  }
  v->desc = o->d_desc; v->x = o->m_x; v->y = o->m_y; v->octave = o->m_oct;
  return VDO_OK;
}

// Wall time of the last vdo_orb_extract: [0] launch of the device stage .. candidates (device tree: and keypoint ids) on the host, [1] the rest of _end
extern "C" int vdo_orb_last_timing(vdo_orb* o, double ms[2]) {
  if (!o || !ms) return set_error(VDO_ERR_INVALID, "null argument");
  ms[0] = o->ms_device; ms[1] = o->ms_tree;
  return VDO_OK;
}

extern "C" int vdo_orb_tree_info(vdo_orb* o, int level, int* on_device, int* status) {
  if (!o || !on_device || !status || level < 0 || level >= o->prm.n_levels) return set_error(VDO_ERR_INVALID, "vdo_orb_tree_info: bad argument");
  if ((int)o->hlevel_cnt.size() != 16) return set_error(VDO_ERR_INVALID, "vdo_orb_tree_info: nothing extracted yet");
  const int st = o->dev_tree ? ((const int*)(o->h_pin + 32 + 4 * (size_t)o->dense_cap))[16 + level] : (int)kQtHostLevel;
  *on_device = st == kQtOk; *status = st;
  return VDO_OK;
}

// K5 alone on given candidate lists (diagnostic: the tests pin k_quadtree on lists no image produces).  The lists go where k_compact puts an image's
// candidates, then the extraction's own launch (orb_queue_tree) and the extraction's own resolution (orb_resolve_levels) run.  k_qt_rows is not queued: it
// reads a pyramid.  Everything is checked before anything is written.
extern "C" int vdo_orb_tree_run(vdo_orb* o, const int32_t* level_count, const float* x, const float* y, const float* resp,
                                int32_t* sel, int sel_capacity, int32_t* sel_count) {
  if (!o) return set_error(VDO_ERR_INVALID, "vdo_orb_tree_run: null argument orb");
  if (!level_count) return set_error(VDO_ERR_INVALID, "vdo_orb_tree_run: null argument level_count");
  if (!x) return set_error(VDO_ERR_INVALID, "vdo_orb_tree_run: null argument x");
  if (!y) return set_error(VDO_ERR_INVALID, "vdo_orb_tree_run: null argument y");
  if (!resp) return set_error(VDO_ERR_INVALID, "vdo_orb_tree_run: null argument resp");
  if (!sel) return set_error(VDO_ERR_INVALID, "vdo_orb_tree_run: null argument sel");
  if (!sel_count) return set_error(VDO_ERR_INVALID, "vdo_orb_tree_run: null argument sel_count");
  if (o->begun) return set_error(VDO_ERR_INVALID, "vdo_orb_tree_run: an extraction is in flight (vdo_orb_extract_begin without _end)");
  const int NL = o->prm.n_levels;
  int64_t total = 0, need = 0;
  for (int l = 0; l < NL; ++l) {
    if (level_count[l] < 0) return set_error(VDO_ERR_INVALID, "vdo_orb_tree_run: level_count[%d] = %d is negative", l, level_count[l]);
    total += level_count[l];
  }
  if (total > o->dense_cap) return set_error(VDO_ERR_INVALID, "vdo_orb_tree_run: level_count sums to %lld candidates, the extractor's dense capacity is %d", (long long)total, o->dense_cap);
  std::vector<int> lvl((size_t)total);
  {
    int64_t pos = 0;
    for (int l = 0; l < NL; ++l) {
      const int n = level_count[l];
      const int W = o->levels[l].w - 2 * kEdge + 6, H = o->levels[l].h - 2 * kEdge + 6;     // maxX - minX, maxY - minY
      bool cells = false;
      for (int c : o->cell_level) cells = cells || c == l;
      if (n > 0 && !cells) return set_error(VDO_ERR_INVALID, "vdo_orb_tree_run: level_count[%d] = %d, but level %d has no FAST cell and never has a candidate", l, n, l);
      // what a level can return: a keypoint per node (vdo_orb_create: max(4 nIni, N + 2)) and never more than it has candidates
      if (cells) need += std::min<int64_t>(n, std::max(4 * o->qtd[l].nIni, o->nfeat[l] + 2));
      for (int k = 0; k < n; ++k) {
        const float fx = x[pos + k], fy = y[pos + k], fr = resp[pos + k];
        if (!(fx >= 0.f && fx < (float)W && fx == std::floor(fx)))
          return set_error(VDO_ERR_INVALID, "vdo_orb_tree_run: x[%lld] = %g (level %d, key %d) is not an integer in [0, %d)", (long long)(pos + k), (double)fx, l, k, W);
        if (!(fy >= 0.f && fy < (float)H && fy == std::floor(fy)))
          return set_error(VDO_ERR_INVALID, "vdo_orb_tree_run: y[%lld] = %g (level %d, key %d) is not an integer in [0, %d)", (long long)(pos + k), (double)fy, l, k, H);
        if (!(fr >= 0.f && fr <= 255.f && fr == std::floor(fr)))
          return set_error(VDO_ERR_INVALID, "vdo_orb_tree_run: resp[%lld] = %g (level %d, key %d) is not an integer in [0, 255]", (long long)(pos + k), (double)fr, l, k);
        lvl[pos + k] = l;
      }
      pos += n;
    }
  }
  if (sel_capacity < need) return set_error(VDO_ERR_INVALID, "vdo_orb_tree_run: sel_capacity %d too small, these lists can return %lld keypoints", sel_capacity, (long long)need);
  int rc = ctx_bind(o->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = o->ctx->stream;
  if (hipStreamSynchronize(s) != hipSuccess) return set_error(VDO_ERR_NO_DEVICE, "vdo_orb_tree_run: %s", hipGetErrorString(hipGetLastError()));   // (the last extraction's blur / angle stages)
  // the lists where k_compact puts them: header and x / y / resp rows of the mapped block (what the host tree reads), the dense device rows and counts
  int* hdr = (int*)o->h_pin;
  float* rows = o->h_pin + 32;
  const size_t pitch = (size_t)o->dense_cap;
  for (int q = 0; q < 32; ++q) hdr[q] = 0;
  for (int l = 0; l < NL; ++l) hdr[l] = level_count[l];
  hdr[16] = (int)total;
  if (total) {
    std::memcpy(rows, x, 4 * (size_t)total); std::memcpy(rows + pitch, y, 4 * (size_t)total); std::memcpy(rows + 2 * pitch, resp, 4 * (size_t)total);
    hipMemcpyAsync(o->d_x, rows, 4 * (size_t)total, hipMemcpyHostToDevice, s);
    hipMemcpyAsync(o->d_y, rows + pitch, 4 * (size_t)total, hipMemcpyHostToDevice, s);
    hipMemcpyAsync(o->d_resp, rows + 2 * pitch, 4 * (size_t)total, hipMemcpyHostToDevice, s);
    hipMemcpyAsync(o->d_lvl, lvl.data(), 4 * (size_t)total, hipMemcpyHostToDevice, s);
  }
  hipMemcpyAsync(o->d_level_cnt, hdr, 4 * 32, hipMemcpyHostToDevice, s);
  if (o->dev_tree) orb_queue_tree(o);
  // no keypoints of an image from here on: nothing for the descriptors or the matcher (no pyramid stands behind these lists)
  o->desc_ready = o->pos_ready = false; o->ang_queued = false;
  o->sel_dense.clear();
  o->hlevel_cnt.assign(hdr, hdr + 16);
  o->n_cand = (int)total;
  o->hx = rows; o->hy = rows + pitch; o->hresp = rows + 2 * pitch; o->hang = rows + 3 * pitch;
  if (hipStreamSynchronize(s) != hipSuccess) return set_error(VDO_ERR_NO_DEVICE, "vdo_orb_tree_run: %s", hipGetErrorString(hipGetLastError()));
  bool on_dev[16] = {};
  orb_resolve_levels(o, on_dev);
  int64_t m = 0;
  for (int l = 0; l < NL; ++l) m += (int64_t)o->sel[l].size();
  if (m > sel_capacity) return set_error(VDO_ERR_INTERNAL, "vdo_orb_tree_run: %lld keypoints, more than the bound %lld", (long long)m, (long long)need);
  int n = 0;
  for (int l = 0; l < NL; ++l) {
    for (int id : o->sel[l]) sel[n++] = id;
    sel_count[l] = (int)o->sel[l].size();
  }
  return VDO_OK;
}

extern "C" int vdo_orb_level_info(vdo_orb* o, int level, int* w, int* h, int* n_features, int* n_candidates) {
  if (!o || level < 0 || level >= o->prm.n_levels) return set_error(VDO_ERR_INVALID, "bad level");
  if (w) *w = o->levels[level].w;
  if (h) *h = o->levels[level].h;
  if (n_features) *n_features = o->nfeat[level];
  if (n_candidates) *n_candidates = o->hlevel_cnt.empty() ? 0 : o->hlevel_cnt[level];
  return VDO_OK;
}

// mvImagePyramid[level] with its 19-px border: (w+38) x (h+38) bytes
extern "C" int vdo_orb_get_pyramid(vdo_orb* o, int level, uint8_t* out_bordered) {
  if (!o || !out_bordered || level < 0 || level >= o->prm.n_levels) return set_error(VDO_ERR_INVALID, "bad argument");
  int rc = ctx_bind(o->ctx);
  if (rc != VDO_OK) return rc;
  const LevelDesc& L = o->levels[level];
  if (hipMemcpy(out_bordered, o->d_pyr + L.off, (size_t)L.bw * L.bh, hipMemcpyDeviceToHost) != hipSuccess) return set_error(VDO_ERR_NO_DEVICE, "D2H failed");
  return VDO_OK;
}

extern "C" int vdo_orb_get_blurred(vdo_orb* o, int level, uint8_t* out) {
  if (!o || !out || level < 0 || level >= o->prm.n_levels) return set_error(VDO_ERR_INVALID, "bad argument");
  int rc = ctx_bind(o->ctx);
  if (rc != VDO_OK) return rc;
  int64_t boff = 0;
  for (int l = 0; l < level; ++l) boff += (int64_t)o->levels[l].w * o->levels[l].h;
  const LevelDesc& L = o->levels[level];
  hipStreamSynchronize(o->ctx->stream);                 // the blur stage runs behind the extraction's own synchronisation point
  if (hipMemcpy(out, o->d_blur + boff, (size_t)L.w * L.h, hipMemcpyDeviceToHost) != hipSuccess) return set_error(VDO_ERR_NO_DEVICE, "D2H failed");
  return VDO_OK;
}

// FAST candidates of the last extraction for one level (reference push order; relative to (16,16))
extern "C" int vdo_orb_get_candidates(vdo_orb* o, int level, float* x, float* y, float* resp, float* angle, int cap, int* n) {
  if (!o || !n || level < 0 || level >= o->prm.n_levels || o->hlevel_cnt.empty()) return set_error(VDO_ERR_INVALID, "bad argument / no extraction yet");
  int pos = 0;
  for (int l = 0; l < level; ++l) pos += o->hlevel_cnt[l];
  const int cnt = o->hlevel_cnt[level];
  *n = cnt;
  // (device tree: vdo_orb_extract_end has not waited for the angle row of all candidates)
  if (angle && !o->fused_angle && !o->begun) {
    const int rc = ctx_bind(o->ctx);
    if (rc != VDO_OK) return rc;
    orb_ensure_angles(o);
  }
  if (angle && !o->fused_angle && !o->begun && hipEventSynchronize(o->ev_ang) != hipSuccess) return set_error(VDO_ERR_NO_DEVICE, "orb angle stage failed: %s", hipGetErrorString(hipGetLastError()));
  for (int k = 0; k < cnt && k < cap; ++k) {
    if (x) x[k] = o->hx[pos + k];
    if (y) y[k] = o->hy[pos + k];
    if (resp) resp[k] = o->hresp[pos + k];
    if (angle) angle[k] = o->hang[pos + k];
  }
  return VDO_OK;
}

extern "C" int vdo_depth_preprocess(vdo_ctx* ctx, float* depth, int64_t n, float bf, float factor, int is_device) {
  if (!ctx || !depth || n <= 0) return set_error(VDO_ERR_INVALID, "bad argument");
  int rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = ctx->stream;
  float* d = depth;
  if (!is_device) {
    if (hipMalloc((void**)&d, 4 * (size_t)n) != hipSuccess) return set_error(VDO_ERR_OOM, "hipMalloc failed");
    hipMemcpyAsync(d, depth, 4 * (size_t)n, hipMemcpyHostToDevice, s);
  }
  hipLaunchKernelGGL(k_depth_preprocess, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, n, bf, factor);
  if (!is_device) {
    hipMemcpyAsync(depth, d, 4 * (size_t)n, hipMemcpyDeviceToHost, s);
    hipStreamSynchronize(s);
    hipFree(d);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(VDO_ERR_NO_DEVICE, "depth preprocess: %s", hipGetErrorString(e));
  return VDO_OK;
}

extern "C" int vdo_rgb2gray(vdo_ctx* ctx, const uint8_t* rgb, int64_t n_pixels, int channels, int rgb_order, uint8_t* gray) {
  if (!ctx || !rgb || !gray || n_pixels <= 0 || (channels != 3 && channels != 4)) return set_error(VDO_ERR_INVALID, "bad argument");
  int rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = ctx->stream;
  uint8_t *ds = nullptr, *dd = nullptr;
  if (hipMalloc((void**)&ds, (size_t)n_pixels * channels) != hipSuccess || hipMalloc((void**)&dd, (size_t)n_pixels) != hipSuccess) { if (ds) hipFree(ds); return set_error(VDO_ERR_OOM, "hipMalloc failed"); }
  hipMemcpyAsync(ds, rgb, (size_t)n_pixels * channels, hipMemcpyHostToDevice, s);
  hipLaunchKernelGGL(k_rgb2gray, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, s, (const uint8_t*)ds, n_pixels, channels, rgb_order, dd);
  hipMemcpyAsync(gray, dd, (size_t)n_pixels, hipMemcpyDeviceToHost, s);
  hipError_t e = hipStreamSynchronize(s);
  hipFree(ds); hipFree(dd);
  if (e != hipSuccess) return set_error(VDO_ERR_NO_DEVICE, "rgb2gray: %s", hipGetErrorString(e));
  return VDO_OK;
}
