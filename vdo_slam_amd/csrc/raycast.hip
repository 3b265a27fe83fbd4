// Raycaster: what the dense mapper's TSDF volume (dense.hip) predicts a camera at pose T would see - a depth, an unnormalised surface gradient and a
// weight per pixel, from a per-pixel march through the cyclic volume with trilinear sampling.  The semantics are this library's own, stated in
// include/vdo_slam_hip.h ("Raycaster") and restated in NumPy by tests/raycast_ref.py.  fp32 with one rounded operation per step in the header's order
// (the library is built with -ffp-contract=off; / and floorf are correctly rounded); every sample is computed from its integer k, nothing is stepped
// along a ray: no result depends on workgroup shape, on the schedule or on the empty-space skipping.
//
//   k_rc_grid<V> x on the lanes, V words of a row per thread (one 16-byte load where nx is a multiple of 4, else single words): a non-zero word at slot s
//                sets the flag of the 8 x 8 x 8-slot bricks that hold s and s - 1 (cyclic) on every axis - a brick's flag is set iff any word of the
//                brick dilated by one slot towards +x, +y, +z is non-zero, which is the slot set a sample with its base cell in the brick can touch.
//                Every writer stores the same byte 1: no atomic, no order.
//   k_rc_march   one thread per pixel, one wave per 8 x 8 pixel tile, 2 x 2 tiles per workgroup: the lanes of a wave walk neighbouring rays and their
//                eight-word gathers fall into the same few lines.  The two x-neighbours of a corner pair are read from one row pointer (adjacent words
//                except at the seam).  The crossing search keeps (valid, F) of the previous sample; a sample whose base brick is clear is invalid without
//                touching the volume.  After the march a hit pixel reads the 32 distinct words of its six gradient samples once.  The three counts by wave
//                ballot, summed over the workgroup in LDS, one 64-bit atomic per workgroup and counter on one of 256 copies, which the host adds up.
//
// NO OUT-OF-RANGE ACCESS: a base cell is turned into slots only after its float compares against (float)o and (float)(o + n - 2) held (a NaN fails them),
// so that every slot lies in [0, n); the gradient's cells b - 1 .. b + 2 are tested the same way before any of the 32 words is read; a brick index is
// slot >> 3; a pixel is written only inside the image.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"
#include "stage.hpp"
#include "dense.hpp"

namespace vdo {

constexpr int kRcMaxSteps = 1 << 16;                                       // (float)k is exact
constexpr int kRcBrick = 3;                                                // log2 of the brick edge in slots
constexpr int kRcSlots = 256;                                              // copies of the counters, 32 bytes apart
constexpr int kRcCounters = 4;                                             // hit, missed, no valid sample, (unused)

// what the kernels take by value
struct RcArgs {
  float fx, fy, cx, cy, near, step, voxel;
  int n_steps, min_w, W, H, tiles_x;
  float c[3], R[9];                                                        // the camera centre; R[3 * i + a] = T(i, a)
  float lo[3], hi[3];                                                      // (float)o, (float)(o + n - 2): the bounds of a base cell
  int n[3], o[3], om[3], nb[3];                                            // size, origin, origin mod size, bricks per axis
};

__device__ __forceinline__ float rc_lerp(float u, float v, float f) { return u + f * (v - u); }

// four lerps along x, two along y, one along z; tijk is the corner at (x, y, z) = (i, j, k)
__device__ __forceinline__ float rc_tri(float t000, float t100, float t010, float t110, float t001, float t101, float t011, float t111, const float f[3]) {
  const float a00 = rc_lerp(t000, t100, f[0]), a10 = rc_lerp(t010, t110, f[0]), a01 = rc_lerp(t001, t101, f[0]), a11 = rc_lerp(t011, t111, f[0]);
  const float b0 = rc_lerp(a00, a10, f[1]), b1 = rc_lerp(a01, a11, f[1]);
  return rc_lerp(b0, b1, f[2]);
}

// the point at depth lam on the ray: its voxel coordinate's base cell b and fractions f.  True iff every g is finite and b lies inside the bounds.
__device__ __forceinline__ bool rc_cell(const RcArgs& a, float lam, const float r[3], float b[3], float f[3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float p = a.c[k] + lam * r[k];
    const float g = p / a.voxel - 0.5f;
    b[k] = floorf(g);
    f[k] = g - b[k];
    ok = ok && dn_finite(g) && a.lo[k] <= b[k] && b[k] <= a.hi[k];
  }
  return ok;
}

// the slot of the base cell b on axis k (b passed rc_cell: o <= b <= o + n - 2)
__device__ __forceinline__ int rc_base(const RcArgs& a, const float b[3], int k) { return dn_slot((int)b[k] - a.o[k], a.om[k], a.n[k]); }

// sample at depth lam: true iff VALID; *F its value and *wmin the smallest corner weight (both meaningful only when the words were read)
__device__ __forceinline__ bool rc_sample(const RcArgs& a, const uint32_t* __restrict__ vol, const uint8_t* __restrict__ grid, float lam, const float r[3], float* F, int* wmin) {
  float b[3], f[3];
  if (!rc_cell(a, lam, r, b, f)) return false;
  const int x0 = rc_base(a, b, 0), y0 = rc_base(a, b, 1), z0 = rc_base(a, b, 2);
  if (grid && !grid[((z0 >> kRcBrick) * a.nb[1] + (y0 >> kRcBrick)) * a.nb[0] + (x0 >> kRcBrick)]) return false;      // all eight words are 0: weight 0 < min_weight
  const int y1 = dn_next(y0, a.n[1]), z1 = dn_next(z0, a.n[2]);
  const int dx1 = x0 + 1 == a.n[0] ? -x0 : 1;                                // the x-neighbour is the next word except at the seam
  const uint32_t* r00 = vol + ((size_t)z0 * a.n[1] + y0) * a.n[0] + x0;
  const uint32_t* r10 = vol + ((size_t)z0 * a.n[1] + y1) * a.n[0] + x0;
  const uint32_t* r01 = vol + ((size_t)z1 * a.n[1] + y0) * a.n[0] + x0;
  const uint32_t* r11 = vol + ((size_t)z1 * a.n[1] + y1) * a.n[0] + x0;
  const uint32_t w000 = r00[0], w100 = r00[dx1], w010 = r10[0], w110 = r10[dx1], w001 = r01[0], w101 = r01[dx1], w011 = r11[0], w111 = r11[dx1];
  const int m = min(min(min(dn_weight(w000), dn_weight(w100)), min(dn_weight(w010), dn_weight(w110))), min(min(dn_weight(w001), dn_weight(w101)), min(dn_weight(w011), dn_weight(w111))));
  *wmin = m;
  *F = rc_tri(dn_tsdf_f(w000), dn_tsdf_f(w100), dn_tsdf_f(w010), dn_tsdf_f(w110), dn_tsdf_f(w001), dn_tsdf_f(w101), dn_tsdf_f(w011), dn_tsdf_f(w111), f);
  return m >= a.min_w;
}

// the gradient at the hit point: central differences of the trilinear form at the base cells b +- e_a with the fractions of b; 0 unless all six are valid
__device__ __forceinline__ void rc_gradient(const RcArgs& a, const uint32_t* __restrict__ vol, float lam, const float r[3], float g[3]) {
  g[0] = g[1] = g[2] = 0.f;
  float b[3], f[3];
  bool ok = rc_cell(a, lam, r, b, f);
#pragma unroll
  for (int k = 0; k < 3; ++k) ok = ok && a.lo[k] <= b[k] - 1.0f && b[k] + 1.0f <= a.hi[k];
  if (!ok) return;
  // slots of the cells b - 1, b, b + 1, b + 2 per axis: all inside the volume, n >= 4
  int sx[4], sy[4], sz[4];
  sx[1] = rc_base(a, b, 0); sy[1] = rc_base(a, b, 1); sz[1] = rc_base(a, b, 2);
  sx[0] = sx[1] == 0 ? a.n[0] - 1 : sx[1] - 1; sy[0] = sy[1] == 0 ? a.n[1] - 1 : sy[1] - 1; sz[0] = sz[1] == 0 ? a.n[2] - 1 : sz[1] - 1;
  sx[2] = dn_next(sx[1], a.n[0]); sy[2] = dn_next(sy[1], a.n[1]); sz[2] = dn_next(sz[1], a.n[2]);
  sx[3] = dn_next(sx[2], a.n[0]); sy[3] = dn_next(sy[2], a.n[1]); sz[3] = dn_next(sz[2], a.n[2]);
  const size_t nx = (size_t)a.n[0], nxy = nx * (size_t)a.n[1];
  uint32_t c[2][2][2], xm[2][2], xp[2][2], ym[2][2], yp[2][2], zm[2][2], zp[2][2];      // c[z][y][x]; xm, xp [z][y]; ym, yp [z][x]; zm, zp [y][x]
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint32_t* row = vol + sz[1 + k] * nxy + sy[1 + j] * nx;
      xm[k][j] = row[sx[0]]; c[k][j][0] = row[sx[1]]; c[k][j][1] = row[sx[2]]; xp[k][j] = row[sx[3]];
    }
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ym[k][i] = vol[sz[1 + k] * nxy + sy[0] * nx + sx[1 + i]];
      yp[k][i] = vol[sz[1 + k] * nxy + sy[3] * nx + sx[1 + i]];
    }
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      zm[j][i] = vol[sz[0] * nxy + sy[1 + j] * nx + sx[1 + i]];
      zp[j][i] = vol[sz[3] * nxy + sy[1 + j] * nx + sx[1 + i]];
    }
  int m = 1 << 20;
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      m = min(m, min(dn_weight(c[k][j][0]), dn_weight(c[k][j][1])));
      m = min(m, min(min(dn_weight(xm[k][j]), dn_weight(xp[k][j])), min(dn_weight(ym[k][j]), dn_weight(yp[k][j]))));
      m = min(m, min(dn_weight(zm[k][j]), dn_weight(zp[k][j])));
    }
  if (m < a.min_w) return;
  const float xa = rc_tri(dn_tsdf_f(c[0][0][1]), dn_tsdf_f(xp[0][0]), dn_tsdf_f(c[0][1][1]), dn_tsdf_f(xp[0][1]), dn_tsdf_f(c[1][0][1]), dn_tsdf_f(xp[1][0]), dn_tsdf_f(c[1][1][1]), dn_tsdf_f(xp[1][1]), f);
  const float xb = rc_tri(dn_tsdf_f(xm[0][0]), dn_tsdf_f(c[0][0][0]), dn_tsdf_f(xm[0][1]), dn_tsdf_f(c[0][1][0]), dn_tsdf_f(xm[1][0]), dn_tsdf_f(c[1][0][0]), dn_tsdf_f(xm[1][1]), dn_tsdf_f(c[1][1][0]), f);
  const float ya = rc_tri(dn_tsdf_f(c[0][1][0]), dn_tsdf_f(c[0][1][1]), dn_tsdf_f(yp[0][0]), dn_tsdf_f(yp[0][1]), dn_tsdf_f(c[1][1][0]), dn_tsdf_f(c[1][1][1]), dn_tsdf_f(yp[1][0]), dn_tsdf_f(yp[1][1]), f);
  const float yb = rc_tri(dn_tsdf_f(ym[0][0]), dn_tsdf_f(ym[0][1]), dn_tsdf_f(c[0][0][0]), dn_tsdf_f(c[0][0][1]), dn_tsdf_f(ym[1][0]), dn_tsdf_f(ym[1][1]), dn_tsdf_f(c[1][0][0]), dn_tsdf_f(c[1][0][1]), f);
  const float za = rc_tri(dn_tsdf_f(c[1][0][0]), dn_tsdf_f(c[1][0][1]), dn_tsdf_f(c[1][1][0]), dn_tsdf_f(c[1][1][1]), dn_tsdf_f(zp[0][0]), dn_tsdf_f(zp[0][1]), dn_tsdf_f(zp[1][0]), dn_tsdf_f(zp[1][1]), f);
  const float zb = rc_tri(dn_tsdf_f(zm[0][0]), dn_tsdf_f(zm[0][1]), dn_tsdf_f(zm[1][0]), dn_tsdf_f(zm[1][1]), dn_tsdf_f(c[0][0][0]), dn_tsdf_f(c[0][0][1]), dn_tsdf_f(c[0][1][0]), dn_tsdf_f(c[0][1][1]), f);
  g[0] = xa - xb; g[1] = ya - yb; g[2] = za - zb;
}

// V consecutive words of a row per thread: 4 (one 16-byte load; nx % 4 == 0, so that a thread's words are aligned and share a brick) or 1.  The words' own
// brick, and the brick of the slot before the FIRST word (the slots before the others are the thread's own), on y and z the bricks of the slot and of
// the slot before it.  nquads = (nx / V) * ny * nz.
template <int V>
__global__ __launch_bounds__(256) void k_rc_grid(const uint32_t* __restrict__ vol, int nx, int ny, int nz, int nbx, int nby, long long nquads, uint8_t* __restrict__ grid) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nquads) return;
  const int qx = nx / V;
  const int x = (int)(i % qx) * V, y = (int)((i / qx) % ny), z = (int)(i / ((long long)qx * ny));
  const uint32_t* p = vol + ((size_t)z * ny + y) * nx + x;
  bool first, some;
  if (V == 4) {
    const uint4 w = *reinterpret_cast<const uint4*>(p);
    first = w.x != 0u; some = (w.x | w.y | w.z | w.w) != 0u;
  } else {
    first = some = p[0] != 0u;
  }
  if (!some) return;
  const int bx = x >> kRcBrick, bxm = (x == 0 ? nx - 1 : x - 1) >> kRcBrick;
  const int by[2] = {y >> kRcBrick, (y == 0 ? ny - 1 : y - 1) >> kRcBrick}, bz[2] = {z >> kRcBrick, (z == 0 ? nz - 1 : z - 1) >> kRcBrick};
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      uint8_t* row = grid + ((size_t)bz[k] * nby + by[j]) * nbx;
      row[bx] = 1;
      if (first) row[bxm] = 1;
    }
}

__global__ __launch_bounds__(256) void k_rc_march(RcArgs a, const uint32_t* __restrict__ vol, const uint8_t* __restrict__ grid, float* __restrict__ depth, float* __restrict__ grad,
                                                  int32_t* __restrict__ weight, unsigned long long* __restrict__ cnt) {
  const int wave = threadIdx.y, lane = threadIdx.x;
  const int tx = (int)(blockIdx.x % (unsigned)a.tiles_x), ty = (int)(blockIdx.x / (unsigned)a.tiles_x);
  const int x = tx * 16 + (wave & 1) * 8 + (lane & 7), y = ty * 16 + (wave >> 1) * 8 + (lane >> 3);
  const bool in = x < a.W && y < a.H;
  bool hit = false, any = false;
  if (in) {
    float r[3];
    dn_ray((float)x, (float)y, a.fx, a.fy, a.cx, a.cy, a.R, r);
    float d_out = 0.f, pF = 0.f;
    int w_out = 0;
    bool pv = false;
    for (int k = 0; k < a.n_steps; ++k) {
      const float lam = a.near + (float)k * a.step;
      float Fk = 0.f;
      int wm = 0;
      const bool v = rc_sample(a, vol, grid, lam, r, &Fk, &wm);
      any = any || v;
      if (v && pv && pF > 0.f && Fk <= 0.f) {
        const float lam0 = a.near + (float)(k - 1) * a.step;
        d_out = lam0 + a.step * (pF / (pF - Fk));
        w_out = wm;
        hit = true;
        break;
      }
      pv = v; pF = Fk;
    }
    const int j = y * a.W + x;
    if (depth) depth[j] = d_out;
    if (weight) weight[j] = w_out;
    if (grad) {
      float g[3] = {0.f, 0.f, 0.f};
      if (hit) rc_gradient(a, vol, d_out, r, g);
      grad[3 * (size_t)j] = g[0]; grad[3 * (size_t)j + 1] = g[1]; grad[3 * (size_t)j + 2] = g[2];
    }
  }
  const int n_hit = (int)__popcll(__ballot(hit)), n_miss = (int)__popcll(__ballot(in && !hit && any)), n_none = (int)__popcll(__ballot(in && !any));
  __shared__ int red[4][3];
  if (lane == 0) { red[wave][0] = n_hit; red[wave][1] = n_miss; red[wave][2] = n_none; }
  __syncthreads();
  if (lane < 3 && wave == 0) {
    const int sum = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    if (sum) atomicAdd(cnt + (blockIdx.x & (unsigned)(kRcSlots - 1)) * kRcCounters + lane, (unsigned long long)sum);
  }
}

}  // namespace vdo

struct vdo_raycast {
  vdo_dense* map = nullptr;                               // borrowed
  vdo::RcArgs a{};
  int skip = 1;
  size_t npix = 0, grid_bytes = 0;
  float* d_stage = nullptr;                               // [H][W] depth, [H][W][3] gradient, [H][W] weight: staging of host outputs
  uint8_t* d_grid = nullptr;                              // one byte per brick
  vdo::SlotCounts cnt;                                    // [kRcSlots][kRcCounters]
  vdo::StageTimer tm;
  hipEvent_t evg = nullptr;                               // between the brick grid and the march
  double grid_ms = 0;
};

using namespace vdo;

void vdo::rc_view_info(const vdo_raycast* view, int* W, int* H, float K[4], vdo_ctx** ctx) {
  *W = view->a.W; *H = view->a.H; *ctx = view->map->ctx;
  K[0] = view->a.fx; K[1] = view->a.fy; K[2] = view->a.cx; K[3] = view->a.cy;
}

static void rc_free(vdo_raycast* h) {
  hipFree(h->d_stage); hipFree(h->d_grid);
  h->cnt.destroy();
  h->tm.destroy();
  if (h->evg) hipEventDestroy(h->evg);
  delete h;
}

extern "C" int vdo_raycast_create(vdo_dense* map, int width, int height, const vdo_raycast_params* p, vdo_raycast** out) {
  static const char* who = "vdo_raycast_create";
  if (!map) return set_error(VDO_ERR_INVALID, "%s: map is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  if (!p) return set_error(VDO_ERR_INVALID, "%s: params is null", who);
  if (width < 1) return set_error(VDO_ERR_INVALID, "%s: width %d < 1", who, width);
  if (height < 1) return set_error(VDO_ERR_INVALID, "%s: height %d < 1", who, height);
  int rc = check_intrinsics(who, "K", p->K);
  if (rc != VDO_OK) return rc;
  if (!is_finite(p->near) || !(p->near >= 0.f)) return set_error(VDO_ERR_INVALID, "%s: near %g must be finite and >= 0", who, (double)p->near);
  if (!is_finite(p->step) || !(p->step > 0.f)) return set_error(VDO_ERR_INVALID, "%s: step %g must be positive and finite", who, (double)p->step);
  if (p->n_steps < 1 || p->n_steps > kRcMaxSteps) return set_error(VDO_ERR_INVALID, "%s: n_steps %d outside 1..65536", who, p->n_steps);
  if (p->min_weight < 1 || p->min_weight > 255) return set_error(VDO_ERR_INVALID, "%s: min_weight %d outside 1..255", who, p->min_weight);
  rc = check_image_size(who, "width x height =", width, height);
  if (rc == VDO_OK) rc = ctx_bind(map->ctx);
  if (rc != VDO_OK) return rc;
  vdo_raycast* h = new vdo_raycast;
  h->map = map;
  RcArgs& a = h->a;
  a.fx = p->K[0]; a.fy = p->K[1]; a.cx = p->K[2]; a.cy = p->K[3]; a.near = p->near; a.step = p->step; a.voxel = map->a.voxel;
  a.n_steps = p->n_steps; a.min_w = p->min_weight; a.W = width; a.H = height; a.tiles_x = (width + 15) / 16;
  h->grid_bytes = 1;
  for (int k = 0; k < 3; ++k) { a.n[k] = map->a.n[k]; a.nb[k] = (a.n[k] + (1 << kRcBrick) - 1) >> kRcBrick; h->grid_bytes *= (size_t)a.nb[k]; }
  h->npix = (size_t)width * height;
  const bool ok = hipMalloc((void**)&h->d_stage, h->npix * 5 * sizeof(float)) == hipSuccess && hipMalloc((void**)&h->d_grid, h->grid_bytes) == hipSuccess &&
                  h->cnt.create(kRcSlots, kRcCounters) && h->tm.create() &&
                  hipEventCreate(&h->evg) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    rc_free(h);
    return set_error(VDO_ERR_OOM, "%s: device allocation failed for a %d x %d view", who, width, height);
  }
  *out = h;
  return VDO_OK;
}

extern "C" int vdo_raycast_destroy(vdo_raycast* h) {
  if (!h) return VDO_OK;
  if (ctx_bind(h->map->ctx) == VDO_OK) hipStreamSynchronize(h->map->ctx->stream);
  rc_free(h);
  return VDO_OK;
}

extern "C" int vdo_raycast_set_skip(vdo_raycast* h, int on) {
  if (!h) return set_error(VDO_ERR_INVALID, "vdo_raycast_set_skip: handle is null");
  h->skip = on ? 1 : 0;
  return VDO_OK;
}

extern "C" int vdo_raycast_render(vdo_raycast* h, const float T[16], float* depth, float* grad, int32_t* weight, int out_is_device, int64_t out[3]) {
  static const char* who = "vdo_raycast_render";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!T) return set_error(VDO_ERR_INVALID, "%s: T is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  int rc = ctx_bind(h->map->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->map->ctx->stream;
  RcArgs a = h->a;
  dn_centre(T, a.c);
  for (int k = 0; k < 3; ++k) {
    a.R[k] = T[k]; a.R[3 + k] = T[4 + k]; a.R[6 + k] = T[8 + k];
    a.o[k] = h->map->a.o[k]; a.om[k] = h->map->a.om[k];
    a.lo[k] = (float)a.o[k]; a.hi[k] = (float)(a.o[k] + a.n[k] - 2);
  }
  const size_t np = h->npix;
  float* o_depth = depth ? (out_is_device ? depth : h->d_stage) : nullptr;
  float* o_grad = grad ? (out_is_device ? grad : h->d_stage + np) : nullptr;
  int32_t* o_wgt = weight ? (out_is_device ? weight : (int32_t*)(h->d_stage + 4 * np)) : nullptr;
  const auto t0 = h->tm.begin(s);
  h->cnt.zero(s);
  if (h->skip) {
    hipMemsetAsync(h->d_grid, 0, h->grid_bytes, s);
    const int v = a.n[0] % 4 == 0 ? 4 : 1;                                   // (the volume is a hipMalloc of its own: its rows are then 16-byte aligned)
    const long long nquads = (long long)(a.n[0] / v) * a.n[1] * a.n[2];
    const dim3 blocks((unsigned)((nquads + 255) / 256));
    if (v == 4) hipLaunchKernelGGL(k_rc_grid<4>, blocks, dim3(256), 0, s, (const uint32_t*)h->map->d_vol, a.n[0], a.n[1], a.n[2], a.nb[0], a.nb[1], nquads, h->d_grid);
    else hipLaunchKernelGGL(k_rc_grid<1>, blocks, dim3(256), 0, s, (const uint32_t*)h->map->d_vol, a.n[0], a.n[1], a.n[2], a.nb[0], a.nb[1], nquads, h->d_grid);
  }
  hipEventRecord(h->evg, s);
  const unsigned tiles = (unsigned)a.tiles_x * (unsigned)((a.H + 15) / 16);
  hipLaunchKernelGGL(k_rc_march, dim3(tiles), dim3(64, 4), 0, s, a, (const uint32_t*)h->map->d_vol, (const uint8_t*)(h->skip ? h->d_grid : nullptr), o_depth, o_grad, o_wgt, h->cnt.d);
  h->tm.mark_end(s);
  h->cnt.download(s);
  if (!out_is_device) {
    if (depth) hipMemcpyAsync(depth, o_depth, np * sizeof(float), hipMemcpyDeviceToHost, s);
    if (grad) hipMemcpyAsync(grad, o_grad, np * 3 * sizeof(float), hipMemcpyDeviceToHost, s);
    if (weight) hipMemcpyAsync(weight, o_wgt, np * sizeof(int32_t), hipMemcpyDeviceToHost, s);
  }
  rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  for (int k = 0; k < 3; ++k) out[k] = h->cnt.sum(k);
  h->tm.finish(t0);
  h->grid_ms = h->skip ? elapsed_ms(h->tm.ev0, h->evg) : 0.0;
  return VDO_OK;
}

extern "C" int vdo_raycast_last_timing(vdo_raycast* h, double ms[2]) {
  return last_timing("vdo_raycast_last_timing", h ? &h->tm : nullptr, ms);
}

extern "C" int vdo_raycast_grid_timing(vdo_raycast* h, double* ms) {
  if (!h || !ms) return set_error(VDO_ERR_INVALID, "vdo_raycast_grid_timing: %s is null", !h ? "handle" : "ms");
  *ms = h->grid_ms;
  return VDO_OK;
}
