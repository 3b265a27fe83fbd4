// Instance labeller: connected components of a class image, cut where the disparity jumps, small components dropped, numbered in raster order into
// the int32 mask image FramePipeline::Step takes; and the same engine as a speckle filter on a disparity image.  The reference takes its masks from
// an offline instance-segmentation network; the semantics are this library's own, stated in include/vdo_slam_hip.h (vdo_labels_compute) and
// restated in NumPy by tests/labels_ref.py.  Integer arithmetic end to end; no result depends on workgroup shape or order.
//
//   k_lab_links     one byte per pixel: the two or four forward links and a member bit.  Computed once, read by everything after; the instance and the
//                   speckle rule are one template flag.  Also clears the per-pixel area and rank and the handle's counters.
//   k_lab_local     one workgroup per 64 x 16 tile, one thread per pixel: union-find in LDS with integer atomicMin, then parent[i] = the GLOBAL raster
//                   index of the local root.  Local and global raster order agree inside a tile, so the local minimum is the global one.
//   k_lab_border    one thread per pixel that has a link across a tile edge: lock-free union on the global parent array.
//   k_lab_flatten   every pixel walks to its root and stores it; areas go to the root with one integer atomic per run of lanes that share a root.
//   k_lab_hist / k_lab_pick   three 9-bit radix passes that find the (max_labels + 1)-th largest area; all but the first return at once unless
//                   more than max_labels components pass min_area.  The launch count is fixed; nothing is read back to choose a path.
//   k_lab_count / k_lab_scan / k_lab_number   ordered compaction of the kept roots (the pattern of frame.hip's K10): rank[root] = 1..n in raster order.
//   k_lab_write     mask[i] = rank[root(i)]; the speckle variant zeroes the pixels of components with area <= max_size and counts them.
//
// INVARIANT, everywhere below: parent[i] <= i at all times (a link is only ever lowered, by atomicMin, to a member of the same component), so every
// walk strictly descends, ends after at most W * H steps, and the final root is the component's smallest raster index whatever the schedule.  Each
// loop still carries that bound as an explicit cap: on overrun the kernel raises a flag and returns, and the call answers VDO_ERR_INTERNAL.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"
#include "scan.hpp"
#include "stage.hpp"

namespace vdo {

constexpr int kLabTW = 64, kLabTH = 16, kLabTile = kLabTW * kLabTH;       // one thread per pixel of a tile: 16 waves, 5 KB of LDS
constexpr int64_t kLabMaxPixels = int64_t(1) << 26;
constexpr int kLabRight = 1, kLabDown = 2, kLabDownRight = 4, kLabDownLeft = 8, kLabMember = 16;
constexpr int kLabBins = 512;                                             // 9 bits per radix pass; 3 passes cover areas up to 2^27 - 1
// the handle's counters (int32 each), cleared by k_lab_links
enum { kSelComponents = 0, kSelPassMin, kSelOverrun, kSelLabels, kSelThreshold, kSelK, kSelPrefix, kSelRemoved, kSelMinKept, kSelReport, kSelHist, kSelSize = kSelHist + 3 * kLabBins };

}  // namespace vdo

struct vdo_labels {
  vdo_ctx* ctx = nullptr;
  int W = 0, H = 0;
  vdo_labels_params p{};
  uint8_t* d_cls = nullptr;                               // [H][W] staged class image
  float* d_disp = nullptr;                                // [H][W] staged disparity
  uint8_t* d_links = nullptr;                             // [H][W]
  int32_t* d_parent = nullptr;                            // [H][W]: after the flatten the root, -1 where the pixel is in no component
  int32_t* d_area = nullptr;                              // [H][W]: the area at each root
  int32_t* d_rank = nullptr;                              // [H][W]: the label at each kept root
  int32_t* d_mask = nullptr;                              // [H][W]
  int32_t* d_blk = nullptr;                               // per 256 pixels: kept roots, then their exclusive scan
  int32_t* d_sel = nullptr;                               // [kSelSize]
  int32_t* h_sel = nullptr;                               // pinned, the first kSelHist of them
  vdo::StageTimer tm;
  bool computed = false;
};

namespace vdo {

__device__ __forceinline__ int lab_disp(float v) { return (v >= 0.f && v < 16777216.f) ? (int)v : 0; }       // NaN, negative, too large: 0 = unknown

template <bool SPECKLE>
__device__ __forceinline__ bool lab_linked(int ca, int cb, int da, int db, int max_diff) {
  if (SPECKLE) return db != 0 && abs(da - db) <= max_diff;                 // (da != 0: the caller is a member)
  return ca == cb && (max_diff < 0 || da == 0 || db == 0 || abs(da - db) <= max_diff);
}

template <bool SPECKLE>
__global__ __launch_bounds__(256) void k_lab_links(const uint8_t* __restrict__ cls, const float* __restrict__ disp, int W, int H, int conn, int max_diff,
                                                   uint8_t* __restrict__ links, int32_t* __restrict__ area, int32_t* __restrict__ rank, int32_t* __restrict__ sel) {
  if (blockIdx.x == 0) for (int k = threadIdx.x; k < kSelSize; k += 256) sel[k] = 0;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W * H) return;
  const int y = i / W, x = i - y * W;
  const bool use_d = SPECKLE || max_diff >= 0;
  const int c = SPECKLE ? 0 : cls[i];
  const int d = use_d ? lab_disp(disp[i]) : 0;
  int bits = 0;
  if (SPECKLE ? d != 0 : c != 0) {
    bits = kLabMember;
    auto link = [&](int dx, int dy) {
      const int xx = x + dx, yy = y + dy;
      if (xx < 0 || xx >= W || yy >= H) return false;
      const int j = yy * W + xx;
      return lab_linked<SPECKLE>(c, SPECKLE ? 0 : cls[j], d, use_d ? lab_disp(disp[j]) : 0, max_diff);
    };
    if (link(1, 0)) bits |= kLabRight;
    if (link(0, 1)) bits |= kLabDown;
    if (conn == 8) {
      if (link(1, 1)) bits |= kLabDownRight;
      if (link(-1, 1)) bits |= kLabDownLeft;
    }
  }
  links[i] = (uint8_t)bits;
  area[i] = 0; rank[i] = 0;
}

// ---- union-find on an array of links with p[i] <= i; `cap` bounds every loop (the invariant above), *overrun is raised when it is passed ---------
template <int SCOPE>
__device__ __forceinline__ int lab_load(const int* p, int i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, SCOPE); }

template <int SCOPE>
__device__ __forceinline__ int lab_find(int* p, int i, int cap, int* overrun) {
  int a = i;
  for (int steps = 0;; ++steps) {
    const int q = lab_load<SCOPE>(p, a);
    if (q == a) break;
    if (steps >= cap) { *overrun = 1; return -1; }
    a = q;                                                // q < a: the walk descends
  }
  if (a != i) __hip_atomic_fetch_min(p + i, a, __ATOMIC_RELAXED, SCOPE);     // shortens later walks; a root is a member below i, so p[i] <= i holds
  return a;
}

// attaches the larger root to the smaller; a lost race continues from the value the atomic returned
template <int SCOPE>
__device__ __forceinline__ void lab_union(int* p, int a, int b, int cap, int* overrun) {
  for (int steps = 0;; ++steps) {
    a = lab_find<SCOPE>(p, a, cap, overrun);
    b = lab_find<SCOPE>(p, b, cap, overrun);
    if (a < 0 || b < 0 || a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }         // a > b
    const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) return;                                 // a was a root and now hangs below b
    if (steps >= cap) { *overrun = 1; return; }
    a = old;                                              // somebody hung a below old < a first (and p[a] is now min(old, b)): old and b remain to be joined
  }
}

__global__ __launch_bounds__(kLabTile) void k_lab_local(const uint8_t* __restrict__ links, int W, int H, int tiles_x, int32_t* __restrict__ parent, int32_t* __restrict__ sel) {
  __shared__ int lab[kLabTile];
  const int l = threadIdx.x, lx = l % kLabTW, ly = l / kLabTW;
  const int x0 = (blockIdx.x % tiles_x) * kLabTW, y0 = (blockIdx.x / tiles_x) * kLabTH;
  const int x = x0 + lx, y = y0 + ly;
  const bool in = x < W && y < H;
  const int bits = in ? links[y * W + x] : 0;             // a link never leaves the image, so a member's partner inside the tile is inside the image
  lab[l] = l;
  __syncthreads();
  constexpr int S = __HIP_MEMORY_SCOPE_WORKGROUP;
  int* overrun = sel + kSelOverrun;
  const bool right = lx + 1 < kLabTW, down = ly + 1 < kLabTH;
  if ((bits & kLabRight) && right) lab_union<S>(lab, l, l + 1, kLabTile, overrun);
  if ((bits & kLabDown) && down) lab_union<S>(lab, l, l + kLabTW, kLabTile, overrun);
  if ((bits & kLabDownRight) && right && down) lab_union<S>(lab, l, l + kLabTW + 1, kLabTile, overrun);
  if ((bits & kLabDownLeft) && lx > 0 && down) lab_union<S>(lab, l, l + kLabTW - 1, kLabTile, overrun);
  __syncthreads();
  if (!in) return;
  int r = -1;
  if (bits & kLabMember) {
    const int lr = lab_find<S>(lab, l, kLabTile, overrun);
    if (lr >= 0) r = (y0 + lr / kLabTW) * W + x0 + lr % kLabTW;       // lr <= l in the tile's raster order, so r <= i in the image's
    else r = y * W + x;
  }
  parent[y * W + x] = r;
}

// Threads 0 .. rows_b * W - 1: the pixels of the last row of a tile row that has a row below it; all their down links cross the edge.  The rest, two
// per tile-column edge and image row: the pixel left of the edge (right and down-right link) and the pixel right of it (down-left link); the diagonal
// ones of a tile's last row were taken by the first group.
__global__ __launch_bounds__(256) void k_lab_border(const uint8_t* __restrict__ links, int W, int H, int rows_b, int cols_b, int32_t* __restrict__ parent, int32_t* __restrict__ sel) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int n_row = rows_b * W;
  constexpr int S = __HIP_MEMORY_SCOPE_AGENT;
  const int cap = W * H;
  int* overrun = sel + kSelOverrun;
  if (t < n_row) {
    const int y = (t / W + 1) * kLabTH - 1, x = t % W, i = y * W + x;
    const int bits = links[i];
    if (bits & kLabDown) lab_union<S>(parent, i, i + W, cap, overrun);
    if (bits & kLabDownRight) lab_union<S>(parent, i, i + W + 1, cap, overrun);
    if (bits & kLabDownLeft) lab_union<S>(parent, i, i + W - 1, cap, overrun);
    return;
  }
  const int u = t - n_row;
  if (u >= 2 * cols_b * H) return;
  const int side = u & 1, e = (u >> 1) % cols_b, y = (u >> 1) / cols_b;
  const int x = (e + 1) * kLabTW - 1 + side, i = y * W + x;
  const bool last_row = y % kLabTH == kLabTH - 1;
  const int bits = links[i];
  if (side == 0) {
    if (bits & kLabRight) lab_union<S>(parent, i, i + 1, cap, overrun);
    if ((bits & kLabDownRight) && !last_row) lab_union<S>(parent, i, i + W + 1, cap, overrun);
  } else if ((bits & kLabDownLeft) && !last_row) {
    lab_union<S>(parent, i, i + W - 1, cap, overrun);
  }
}

// No union runs beside this kernel, so every store writes the component's final root.  Areas are integer sums: the order of the atomics is immaterial.
__global__ __launch_bounds__(256) void k_lab_flatten(int n, int32_t* __restrict__ parent, int32_t* __restrict__ area, int32_t* __restrict__ sel) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  constexpr int S = __HIP_MEMORY_SCOPE_AGENT;
  int r = -1;
  if (i < n) {
    const int p = lab_load<S>(parent, i);
    if (p >= 0) {
      r = lab_find<S>(parent, p, n, sel + kSelOverrun);   // (its min on parent[p] lets the tile's other pixels stop after one step)
      if (r >= 0) __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, S);
    }
  }
  // neighbours in raster order mostly share a root: one atomic per run of equal roots in the wave
  const int lane = threadIdx.x & 63;
  const int prev = __shfl_up(r, 1, 64);
  const bool head = lane == 0 || prev != r;
  const uint64_t heads = __ballot(head);
  if (head && r >= 0) {
    const uint64_t above = lane == 63 ? 0 : heads >> (lane + 1);
    const int len = above ? __ffsll((unsigned long long)above) : 64 - lane;
    atomicAdd(area + r, len);
  }
}

// Radix pass PASS (bits 26..18, 17..9, 8..0) of the areas at the roots.  Pass 0 also counts the components and those of at least min_area.
template <int PASS>
__global__ __launch_bounds__(256) void k_lab_hist(int n, const int32_t* __restrict__ parent, const int32_t* __restrict__ area, int min_area, int max_labels, int32_t* __restrict__ sel) {
  __shared__ int hist[kLabBins];
  __shared__ int cnt[2];
  if (PASS > 0 && sel[kSelPassMin] <= max_labels) return;                   // (uniform over the launch: pass 0 has ended)
  for (int k = threadIdx.x; k < kLabBins; k += 256) hist[k] = 0;
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && parent[i] == i) {
    const int a = area[i];
    constexpr int shift = 18 - 9 * PASS;
    if (PASS == 0) { atomicAdd(&cnt[0], 1); if (a >= min_area) atomicAdd(&cnt[1], 1); }
    if (PASS == 0 || (a >> (shift + 9)) == sel[kSelPrefix]) atomicAdd(&hist[(a >> shift) & (kLabBins - 1)], 1);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kLabBins; k += 256) if (hist[k]) atomicAdd(sel + kSelHist + PASS * kLabBins + k, hist[k]);
  if (PASS == 0 && threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(sel + (threadIdx.x ? kSelPassMin : kSelComponents), cnt[threadIdx.x]);
}

// One workgroup, one thread per bin from the largest down: the bin in which the K-th largest area lies.  After pass 2 the threshold: with
// v the (max_labels + 1)-th largest area, more than max_labels components have area >= v and at most max_labels have area >= v + 1.
template <int PASS>
__global__ __launch_bounds__(kLabBins) void k_lab_pick(int min_area, int max_labels, int32_t* __restrict__ sel) {
  __shared__ int lds[17];
  if (PASS == 2 && threadIdx.x == 0) sel[kSelMinKept] = INT32_MAX;
  if (sel[kSelPassMin] <= max_labels) {
    if (PASS == 2 && threadIdx.x == 0) sel[kSelThreshold] = min_area;
    return;
  }
  const int K = PASS == 0 ? max_labels + 1 : sel[kSelK];
  const int prefix = PASS == 0 ? 0 : sel[kSelPrefix];
  const int bin = kLabBins - 1 - threadIdx.x;
  const int v = sel[kSelHist + PASS * kLabBins + bin];
  int total;
  const int ex = block_excl_scan(v, lds, &total);
  if (ex < K && K <= ex + v) {                            // exactly one thread
    const int value = (prefix << 9) | bin;
    sel[kSelPrefix] = value; sel[kSelK] = K - ex;
    if (PASS == 2) sel[kSelThreshold] = value + 1;
  }
}

__device__ __forceinline__ int lab_kept(int i, int n, const int32_t* __restrict__ parent, const int32_t* __restrict__ area, int threshold) {
  return i < n && parent[i] == i && area[i] >= threshold;
}

// also the smallest area kept (at most max_labels atomics in the whole launch)
__global__ __launch_bounds__(256) void k_lab_count(int n, const int32_t* __restrict__ parent, const int32_t* __restrict__ area, int32_t* __restrict__ sel, int32_t* __restrict__ blk_cnt) {
  __shared__ int lds[17];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int keep = lab_kept(i, n, parent, area, sel[kSelThreshold]);
  if (keep) atomicMin(sel + kSelMinKept, area[i]);
  int total;
  block_excl_scan(keep, lds, &total);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// exclusive scan of the workgroup counts (single workgroup), as frame.hip's k_scan_blocks; and the threshold as it is reported: min_area when
// nothing overflowed, else the smallest area kept, else (nothing kept) the working threshold
__global__ __launch_bounds__(1024) void k_lab_scan(int32_t* __restrict__ blk_cnt, int nblk, int min_area, int max_labels, int32_t* __restrict__ sel) {
  __shared__ int lds[17];
  int carry = 0;
  for (int base = 0; base < nblk; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < nblk ? blk_cnt[i] : 0;
    int total;
    const int ex = block_excl_scan(v, lds, &total);
    if (i < nblk) blk_cnt[i] = carry + ex;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    sel[kSelLabels] = carry;
    sel[kSelReport] = sel[kSelPassMin] <= max_labels ? min_area : carry > 0 ? sel[kSelMinKept] : sel[kSelThreshold];
  }
}

__global__ __launch_bounds__(256) void k_lab_number(int n, const int32_t* __restrict__ parent, const int32_t* __restrict__ area, const int32_t* __restrict__ sel,
                                                    const int32_t* __restrict__ blk_off, int32_t* __restrict__ rank) {
  __shared__ int lds[17];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int keep = lab_kept(i, n, parent, area, sel[kSelThreshold]);
  int total;
  const int pos = blk_off[blockIdx.x] + block_excl_scan(keep, lds, &total);
  if (keep) rank[i] = pos + 1;                            // <= max_labels <= 1023 by the choice of the threshold
}

template <bool SPECKLE>
__global__ __launch_bounds__(256) void k_lab_write(int n, const int32_t* __restrict__ parent, const int32_t* __restrict__ area, const int32_t* __restrict__ rank, int max_size,
                                                   int32_t* __restrict__ mask, float* __restrict__ disp, int32_t* __restrict__ sel) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int r = i < n ? parent[i] : -1;
  if (!SPECKLE) {
    if (i < n) mask[i] = r >= 0 ? rank[r] : 0;
    return;
  }
  const bool drop = r >= 0 && area[r] <= max_size;
  if (drop) disp[i] = 0.f;
  const int c = (int)__popcll(__ballot(drop));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(sel + kSelRemoved, c);
}

static void lab_free(vdo_labels* h) {
  hipFree(h->d_cls); hipFree(h->d_disp); hipFree(h->d_links); hipFree(h->d_parent); hipFree(h->d_area); hipFree(h->d_rank); hipFree(h->d_mask); hipFree(h->d_blk); hipFree(h->d_sel);
  if (h->h_sel) hipHostFree(h->h_sel);
  h->tm.destroy();
  delete h;
}

// links, local labelling, border merge, flatten and areas: the part the two consumers share.  cls / disp: packed device images.
template <bool SPECKLE>
static void lab_components(vdo_labels* h, hipStream_t s, const uint8_t* cls, const float* disp, int conn, int max_diff) {
  const int W = h->W, H = h->H, n = W * H, nblk = (n + 255) / 256;
  const int tiles_x = (W + kLabTW - 1) / kLabTW, tiles_y = (H + kLabTH - 1) / kLabTH;
  const int rows_b = (H - 1) / kLabTH, cols_b = (W - 1) / kLabTW;           // tile edges with pixels on both sides
  hipLaunchKernelGGL(k_lab_links<SPECKLE>, dim3(nblk), dim3(256), 0, s, cls, disp, W, H, conn, max_diff, h->d_links, h->d_area, h->d_rank, h->d_sel);
  hipLaunchKernelGGL(k_lab_local, dim3(tiles_x * tiles_y), dim3(kLabTile), 0, s, (const uint8_t*)h->d_links, W, H, tiles_x, h->d_parent, h->d_sel);
  const int n_border = rows_b * W + 2 * cols_b * H;
  if (n_border > 0)                                       // (a matter of the image's size, not of its content)
    hipLaunchKernelGGL(k_lab_border, dim3((n_border + 255) / 256), dim3(256), 0, s, (const uint8_t*)h->d_links, W, H, rows_b, cols_b, h->d_parent, h->d_sel);
  hipLaunchKernelGGL(k_lab_flatten, dim3(nblk), dim3(256), 0, s, n, h->d_parent, h->d_area, h->d_sel);
}

static int lab_finish(const char* who, vdo_labels* h, StageClock::time_point t0) {
  hipStream_t s = h->ctx->stream;
  hipMemcpyAsync(h->h_sel, h->d_sel, kSelHist * sizeof(int32_t), hipMemcpyDeviceToHost, s);
  const int rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  if (h->h_sel[kSelOverrun]) return set_error(VDO_ERR_INTERNAL, "%s: a union-find walk passed its step bound of width x height", who);
  h->tm.finish(t0);
  h->computed = true;
  return VDO_OK;
}

}  // namespace vdo

using namespace vdo;

extern "C" int vdo_labels_create(vdo_ctx* ctx, int width, int height, const vdo_labels_params* p, vdo_labels** out) {
  static const char* who = "vdo_labels_create";
  if (!ctx) return set_error(VDO_ERR_INVALID, "%s: ctx is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (!p) return set_error(VDO_ERR_INVALID, "%s: params is null", who);
  if (width < 1) return set_error(VDO_ERR_INVALID, "%s: width %d < 1", who, width);
  if (height < 1) return set_error(VDO_ERR_INVALID, "%s: height %d < 1", who, height);
  if (p->connectivity != 4 && p->connectivity != 8) return set_error(VDO_ERR_INVALID, "%s: connectivity %d is neither 4 nor 8", who, p->connectivity);
  if (p->max_disp_diff < -1) return set_error(VDO_ERR_INVALID, "%s: max_disp_diff %d below -1", who, p->max_disp_diff);
  if (p->min_area < 1) return set_error(VDO_ERR_INVALID, "%s: min_area %d < 1", who, p->min_area);
  if (p->max_labels < 1 || p->max_labels > 1023) return set_error(VDO_ERR_INVALID, "%s: max_labels %d outside 1..1023", who, p->max_labels);
  if ((int64_t)width * height > kLabMaxPixels) return set_error(VDO_ERR_UNSUPPORTED, "%s: width x height = %d x %d exceeds 2^26 pixels", who, width, height);
  int rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  vdo_labels* h = new vdo_labels;
  h->ctx = ctx; h->W = width; h->H = height; h->p = *p;
  const size_t n = (size_t)width * height, nblk = (n + 255) / 256;
  const bool ok = hipMalloc((void**)&h->d_cls, n) == hipSuccess && hipMalloc((void**)&h->d_disp, n * sizeof(float)) == hipSuccess && hipMalloc((void**)&h->d_links, n) == hipSuccess &&
                  hipMalloc((void**)&h->d_parent, n * sizeof(int32_t)) == hipSuccess && hipMalloc((void**)&h->d_area, n * sizeof(int32_t)) == hipSuccess &&
                  hipMalloc((void**)&h->d_rank, n * sizeof(int32_t)) == hipSuccess && hipMalloc((void**)&h->d_mask, n * sizeof(int32_t)) == hipSuccess &&
                  hipMalloc((void**)&h->d_blk, nblk * sizeof(int32_t)) == hipSuccess && hipMalloc((void**)&h->d_sel, kSelSize * sizeof(int32_t)) == hipSuccess &&
                  hipHostMalloc((void**)&h->h_sel, kSelHist * sizeof(int32_t), hipHostMallocDefault) == hipSuccess && h->tm.create();
  if (!ok) {
    (void)hipGetLastError();
    lab_free(h);
    return set_error(VDO_ERR_OOM, "%s: device allocation failed for %d x %d", who, width, height);
  }
  *out = h;
  return VDO_OK;
}

extern "C" int vdo_labels_destroy(vdo_labels* h) {
  if (!h) return VDO_OK;
  if (ctx_bind(h->ctx) == VDO_OK) hipStreamSynchronize(h->ctx->stream);
  lab_free(h);
  return VDO_OK;
}

extern "C" int vdo_labels_compute(vdo_labels* h, const uint8_t* cls, int64_t cls_stride, const float* disp, int64_t disp_stride_floats, int src_is_device, int32_t* mask,
                                  int out_is_device, int32_t out[3]) {
  static const char* who = "vdo_labels_compute";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!cls) return set_error(VDO_ERR_INVALID, "%s: cls is null", who);
  if (cls_stride < h->W) return set_error(VDO_ERR_INVALID, "%s: cls_stride %lld smaller than the width %d", who, (long long)cls_stride, h->W);
  const bool gate = h->p.max_disp_diff >= 0;
  if (gate && !disp) return set_error(VDO_ERR_INVALID, "%s: disp is null with max_disp_diff %d (only -1 needs no disparity)", who, h->p.max_disp_diff);
  if (gate && disp_stride_floats < h->W) return set_error(VDO_ERR_INVALID, "%s: disp_stride_floats %lld smaller than the width %d", who, (long long)disp_stride_floats, h->W);
  if (!mask) return set_error(VDO_ERR_INVALID, "%s: mask is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const int W = h->W, H = h->H, n = W * H, nblk = (n + 255) / 256;
  const auto t0 = h->tm.begin(s);
  // packed device images are read where they lie; anything else is brought to the handle's staging images
  const uint8_t* d_cls = stage_rows(s, h->d_cls, cls, cls_stride, W, H, src_is_device);
  const float* d_disp = gate ? stage_rows(s, h->d_disp, disp, disp_stride_floats, W, H, src_is_device) : nullptr;
  int32_t* d_mask = out_is_device ? mask : h->d_mask;
  lab_components<false>(h, s, d_cls, d_disp, h->p.connectivity, h->p.max_disp_diff);
  const int32_t *par = h->d_parent, *area = h->d_area;
  const int mn = h->p.min_area, mx = h->p.max_labels;
  hipLaunchKernelGGL(k_lab_hist<0>, dim3(nblk), dim3(256), 0, s, n, par, area, mn, mx, h->d_sel);
  hipLaunchKernelGGL(k_lab_pick<0>, dim3(1), dim3(kLabBins), 0, s, mn, mx, h->d_sel);
  hipLaunchKernelGGL(k_lab_hist<1>, dim3(nblk), dim3(256), 0, s, n, par, area, mn, mx, h->d_sel);
  hipLaunchKernelGGL(k_lab_pick<1>, dim3(1), dim3(kLabBins), 0, s, mn, mx, h->d_sel);
  hipLaunchKernelGGL(k_lab_hist<2>, dim3(nblk), dim3(256), 0, s, n, par, area, mn, mx, h->d_sel);
  hipLaunchKernelGGL(k_lab_pick<2>, dim3(1), dim3(kLabBins), 0, s, mn, mx, h->d_sel);
  hipLaunchKernelGGL(k_lab_count, dim3(nblk), dim3(256), 0, s, n, par, area, h->d_sel, h->d_blk);
  hipLaunchKernelGGL(k_lab_scan, dim3(1), dim3(1024), 0, s, h->d_blk, nblk, mn, mx, h->d_sel);
  hipLaunchKernelGGL(k_lab_number, dim3(nblk), dim3(256), 0, s, n, par, area, (const int32_t*)h->d_sel, (const int32_t*)h->d_blk, h->d_rank);
  hipLaunchKernelGGL(k_lab_write<false>, dim3(nblk), dim3(256), 0, s, n, par, area, (const int32_t*)h->d_rank, 0, d_mask, (float*)nullptr, h->d_sel);
  h->tm.mark_end(s);
  // the mask travels before the verdict is known; a walk past its bound (VDO_ERR_INTERNAL) cannot happen while the invariant holds
  if (!out_is_device) hipMemcpyAsync(mask, h->d_mask, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s);
  rc = lab_finish(who, h, t0);
  if (rc != VDO_OK) return rc;
  out[0] = h->h_sel[kSelLabels]; out[1] = h->h_sel[kSelComponents]; out[2] = h->h_sel[kSelReport];
  return VDO_OK;
}

extern "C" int vdo_labels_filter_speckles(vdo_labels* h, float* disparity256, int is_device, int max_diff, int max_size, int32_t* n_removed) {
  static const char* who = "vdo_labels_filter_speckles";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!disparity256) return set_error(VDO_ERR_INVALID, "%s: disparity256 is null", who);
  if (max_diff < 0) return set_error(VDO_ERR_INVALID, "%s: max_diff %d < 0", who, max_diff);
  if (max_size < 0) return set_error(VDO_ERR_INVALID, "%s: max_size %d < 0", who, max_size);
  if (!n_removed) return set_error(VDO_ERR_INVALID, "%s: n_removed is null", who);
  int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const int n = h->W * h->H, nblk = (n + 255) / 256;
  const auto t0 = h->tm.begin(s);
  float* d = is_device ? disparity256 : h->d_disp;
  if (!is_device) hipMemcpyAsync(h->d_disp, disparity256, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s);
  lab_components<true>(h, s, nullptr, d, 4, max_diff);
  hipLaunchKernelGGL(k_lab_write<true>, dim3(nblk), dim3(256), 0, s, n, (const int32_t*)h->d_parent, (const int32_t*)h->d_area, (const int32_t*)h->d_rank, max_size,
                     (int32_t*)nullptr, d, h->d_sel);
  h->tm.mark_end(s);
  if (!is_device) hipMemcpyAsync(disparity256, h->d_disp, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s);
  rc = lab_finish(who, h, t0);
  if (rc != VDO_OK) return rc;
  *n_removed = h->h_sel[kSelRemoved];
  return VDO_OK;
}

static int lab_fetch(const char* who, vdo_labels* h, const int32_t* dev, int32_t* out) {
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (!h->computed) return set_error(VDO_ERR_INVALID, "%s: no vdo_labels_compute or vdo_labels_filter_speckles on this handle yet", who);
  const int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipMemcpyAsync(out, dev, (size_t)h->W * h->H * sizeof(int32_t), hipMemcpyDeviceToHost, h->ctx->stream);
  return check_hip(who, hipStreamSynchronize(h->ctx->stream));
}

extern "C" int vdo_labels_get_roots(vdo_labels* h, int32_t* out) { return lab_fetch("vdo_labels_get_roots", h, h ? h->d_parent : nullptr, out); }

extern "C" int vdo_labels_get_areas(vdo_labels* h, int32_t* out) { return lab_fetch("vdo_labels_get_areas", h, h ? h->d_area : nullptr, out); }

extern "C" int vdo_labels_last_timing(vdo_labels* h, double ms[2]) {
  return last_timing("vdo_labels_last_timing", h ? &h->tm : nullptr, ms);
}

extern "C" int vdo_labels_device_images(vdo_labels* h, uint8_t** cls, int32_t** mask) {
  if (!h) return set_error(VDO_ERR_INVALID, "vdo_labels_device_images: handle is null");
  if (cls) *cls = h->d_cls;
  if (mask) *mask = h->d_mask;
  return VDO_OK;
}

extern "C" int vdo_labels_stage_classes(vdo_labels* h, const uint8_t* cls, int64_t cls_stride, uint8_t** cls_dev) {
  static const char* who = "vdo_labels_stage_classes";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!cls || !cls_dev) return set_error(VDO_ERR_INVALID, "%s: %s is null", who, !cls ? "cls" : "cls_dev");
  if (cls_stride < h->W) return set_error(VDO_ERR_INVALID, "%s: cls_stride %lld smaller than the width %d", who, (long long)cls_stride, h->W);
  const int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  stage_rows(h->ctx->stream, h->d_cls, cls, cls_stride, h->W, h->H, 0);
  const int rs = check_hip(who, hipStreamSynchronize(h->ctx->stream));
  if (rs != VDO_OK) return rs;
  *cls_dev = h->d_cls;
  return VDO_OK;
}
