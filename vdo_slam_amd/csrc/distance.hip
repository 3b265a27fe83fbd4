// Distance field: the exact squared Euclidean distance, in voxels, from every voxel of a box of a dense mapper's TSDF volume (the static map or an
// object's volume) to the nearest SITE - a valid voxel at an end of a sign-changing lattice edge - and the voxel's state (unknown, free, inside).
// The reference keeps no dense map; the semantics are this library's own, stated in include/vdo_slam_hip.h ("Distance field") and restated in NumPy
// by tests/distance_ref.py.  Everything up to the sample's floor is integer, and every thread works from its own integer index: no result depends on
// launch shape, method, schedule or the slot alignment of the cyclic volume.
//
// The field is separable: d2(p) = min_z (dz^2 + min_y (dy^2 + min_x dx^2)).  One uint32 per voxel of the box in BOX order (x fastest), the state in
// bits 28-29 from the first kernel on, the running minimum in bits 0-27, capped to FAR as soon as it passes R^2 (an axis offset above R, or a partial
// sum above R^2, cannot end at or below R^2):
//   k_dt_sites          thread i = box voxel i: its word and its six neighbours through the cyclic slots (a neighbour outside the volume does not
//                       exist), the site bit as a wave ballot, 1 bit per voxel at bit i of the bit array, the state into the field.
//   k_dt_x              the nearest set bit to the left and to the right inside the voxel's own row, from the ballot words with clz / ctz.
//   k_dt_axis_win<LDS>  method 1, y then z: out(p) = min over |q - p| <= R of f(q) + (p - q)^2, the columns on the lanes (adjacent lanes read adjacent
//                       x: coalesced).  LDS: from a tile of up to 64 rows of 64 columns with an R-row halo; !LDS (the window does not fit): from memory.
//   k_dt_axis_env       method 2: the lower envelope of the parabolas of a column (Meijster), one thread per column, integers only - the abscissa
//                       where a parabola takes over is an exact floor division.  The stack of a column (s, t packed in one word) lives in the
//                       column's own OUTPUT words: the backward scan at u reads entry q <= t[q] <= u before it writes word u, so no entry still
//                       needed is overwritten and no third buffer exists.
//   k_dt_sample         one thread per point: the float compares, then the index.
// The three counts are integer atomics (order-free), kDtSlots copies 32 bytes apart that the host adds up.
//
// NO OUT-OF-RANGE ACCESS: a voxel is read only at local coordinates tested against n; a field word only at a column index tested against `inner` and a
// position tested against L; a bit word only at indices inside the row's own words; a sampled word only after the point's voxel lay in the box.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"
#include "stage.hpp"
#include "dense.hpp"

namespace vdo {

constexpr uint32_t kDtFar = VDO_DISTANCE_FAR, kDtState = 0x30000000u;
constexpr int kDtRows = 192;                                               // the most rows of the LDS tile of k_dt_axis_win: 48 KiB
constexpr int kDtMinTile = 32;                                             // the fewest rows of a tile that are not halo
constexpr int kDtWinMax = (kDtRows - kDtMinTile) / 2;                       // method 0: the window while min(R, L - 1) <= 80, where its tile fits the LDS; else the envelope
constexpr int kDtSlots = 64, kDtCounters = 4;                              // sites, voxels in reach, points inside
constexpr long long kDtMaxWindow = 1LL << 30;                              // points per launch of k_dt_sample on device points

struct DtArgs {
  int n[3], om[3];                                                         // the map's size and origin mod size
  int blo[3], b[3];                                                        // the clipped box: its lower corner in LOCAL voxels, its size
  int min_w, R;
  unsigned nbox;
};

struct DtSnap {
  int lo[3], hi[3];                                                        // global voxels; all 0 when empty
  float voxel;
};

// adds v (summed over the wave; every lane of the wave calls) to counter `which`
__device__ __forceinline__ void dt_count(int v, int which, u64* __restrict__ cnt) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63u) == 0 && v) {
    const unsigned slot = (blockIdx.x + blockIdx.y + blockIdx.z + (threadIdx.x >> 6)) & (unsigned)(kDtSlots - 1);
    atomicAdd(cnt + slot * kDtCounters + which, (u64)v);
  }
}

__global__ __launch_bounds__(256) void k_dt_sites(DtArgs a, const uint32_t* __restrict__ vol, u64* __restrict__ bits, uint32_t* __restrict__ field, u64* __restrict__ cnt) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  bool site = false;
  if (i < a.nbox) {
    const unsigned bx = (unsigned)a.b[0], by = (unsigned)a.b[1], r = i / bx, z = r / by;
    const int l[3] = {a.blo[0] + (int)(i - r * bx), a.blo[1] + (int)(r - z * by), a.blo[2] + (int)z};
    const uint32_t v = dn_word(vol, a.n, a.om, l[0], l[1], l[2]);
    uint32_t state = 0u;
    if (dn_weight(v) >= a.min_w) {
      const bool neg = (int16_t)(v & 0xffffu) < 0;                           // dn_tsdf(v) < 0, spelled out here and below: the call moves the kernel's registers
      state = neg ? 2u : 1u;
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int d = -1; d <= 1; d += 2) {
          int m[3] = {l[0], l[1], l[2]};
          m[k] += d;
          if (m[k] < 0 || m[k] >= a.n[k]) continue;
          const uint32_t q = dn_word(vol, a.n, a.om, m[0], m[1], m[2]);
          site = site || (dn_weight(q) >= a.min_w && ((int16_t)(q & 0xffffu) < 0) != neg);
        }
    }
    field[i] = state << 28;
  }
  const u64 bal = __ballot(site);
  if ((threadIdx.x & 63u) == 0 && i < a.nbox) bits[i >> 6] = bal;
  dt_count(site ? 1 : 0, 0, cnt);
}

__global__ __launch_bounds__(256) void k_dt_x(DtArgs a, const u64* __restrict__ bits, uint32_t* __restrict__ field) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.nbox) return;
  const unsigned bx = (unsigned)a.b[0], x = i % bx, R = (unsigned)a.R;
  const unsigned first = i - (x < R ? x : R), last = i + (bx - 1u - x < R ? bx - 1u - x : R);      // the bits of the row within reach
  unsigned d = R + 1u;
  unsigned w = i >> 6;
  u64 m = bits[w] & (~0ull >> (63u - (i & 63u)));                           // bits at or below i
  for (;;) {
    if (m) {
      const unsigned pos = (w << 6) + 63u - (unsigned)__clzll((long long)m);
      if (pos >= first) d = i - pos;
      break;
    }
    if ((w << 6) <= first) break;
    m = bits[--w];
  }
  w = i >> 6;
  m = bits[w] & (~0ull << (i & 63u));                                       // bits at or above i
  for (;;) {
    if (m) {
      const unsigned pos = (w << 6) + (unsigned)__ffsll((long long)m) - 1u;
      if (pos <= last && pos - i < d) d = pos - i;
      break;
    }
    if ((w << 6) + 63u >= last) break;
    m = bits[++w];
  }
  field[i] = (field[i] & kDtState) | (d <= R ? d * d : kDtFar);
}

// Method 1.  Workgroup (x, y, z) takes the 64 columns from 64 x, the positions [T y, T y + T) of them, of outer index z; wave v the positions v, v + 4, ...
template <bool LDS>
__global__ __launch_bounds__(256) void k_dt_axis_win(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t inner, int L, int R, uint32_t cap, int T, u64* __restrict__ cnt) {
  extern __shared__ uint32_t tile[];                                         // LDS: [T + 2 R][64]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, p0 = (int)blockIdx.y * T;
  const size_t c = (size_t)blockIdx.x * 64u + lane, base = (size_t)blockIdx.z * L * inner + c;
  const bool col = c < inner;
  if (LDS) {
    for (int r = wv; r < T + 2 * R; r += 4) {
      const int q = p0 - R + r;
      tile[r * 64 + lane] = col && q >= 0 && q < L ? in[base + (size_t)q * inner] : kDtFar;
    }
    __syncthreads();
  }
  int reach = 0;
  for (int pl = wv; pl < T; pl += 4) {
    const int p = p0 + pl;
    if (p >= L || !col) continue;
    uint32_t m = kDtFar, self;
    if (LDS) {
      self = tile[(pl + R) * 64 + lane];
      for (int d = -R; d <= R; ++d) {
        const uint32_t v = (tile[(pl + R + d) * 64 + lane] & kDtFar) + (uint32_t)(d * d);
        m = v < m ? v : m;
      }
    } else {
      self = in[base + (size_t)p * inner];
      const int q0 = p - R > 0 ? p - R : 0, q1 = p + R < L - 1 ? p + R : L - 1;
      for (int q = q0; q <= q1; ++q) {
        const uint32_t v = (in[base + (size_t)q * inner] & kDtFar) + (uint32_t)((q - p) * (q - p));
        m = v < m ? v : m;
      }
    }
    if (m > cap) m = kDtFar;
    reach += m != kDtFar;
    out[base + (size_t)p * inner] = (self & kDtState) | m;
  }
  if (cnt) dt_count(reach, 1, cnt);
}

// Method 2.  Thread = column.  Stack entry q in out[q]: s | t << 16 - the parabola of s is the lowest from t on.  The top entry stays in registers.
__global__ __launch_bounds__(256) void k_dt_axis_env(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t inner, int L, size_t ncol, uint32_t cap, u64* __restrict__ cnt) {
  const size_t col = (size_t)blockIdx.x * 256u + threadIdx.x;
  int reach = 0;
  if (col < ncol) {
    const size_t o = col / inner, base = o * L * inner + (col - o * inner);
    int q = 0, ss = 0, tt = 0, fs = (int)(in[base] & kDtFar);
    out[base] = 0u;
    for (int u = 1; u < L; ++u) {
      const int fu = (int)(in[base + (size_t)u * inner] & kDtFar);
      while (fs + (tt - ss) * (tt - ss) > fu + (tt - u) * (tt - u)) {         // at t the new parabola is lower: the top never shows
        if (--q < 0) break;
        const uint32_t e = out[base + (size_t)q * inner];
        ss = (int)(e & 0xffffu); tt = (int)(e >> 16); fs = (int)(in[base + (size_t)ss * inner] & kDtFar);
      }
      if (q < 0) {
        q = 0; ss = u; tt = 0; fs = fu;
        out[base] = (uint32_t)u;
      } else {
        const int w = 1 + dn_floor_div(((u * u - ss * ss) + fu) - fs, 2 * (u - ss));      // the first abscissa at which u is lower; sums below 2^31
        if (w < L) {
          ++q; ss = u; tt = w; fs = fu;
          out[base + (size_t)q * inner] = (uint32_t)u | (uint32_t)w << 16;
        }
      }
    }
    for (int u = L - 1; u >= 0; --u) {
      uint32_t m = (uint32_t)(fs + (u - ss) * (u - ss));
      if (m > cap) m = kDtFar;
      reach += m != kDtFar;
      const bool pop = u == tt && q > 0;
      uint32_t e = 0u;
      if (pop) e = out[base + (size_t)(q - 1) * inner];                     // q - 1 < t[q] = u: read before word u is written
      out[base + (size_t)u * inner] = (in[base + (size_t)u * inner] & kDtState) | m;
      if (pop) { --q; ss = (int)(e & 0xffffu); tt = (int)(e >> 16); fs = (int)(in[base + (size_t)ss * inner] & kDtFar); }
    }
  }
  if (cnt) dt_count(reach, 1, cnt);
}

// points [0, n) of a window
__global__ __launch_bounds__(256) void k_dt_sample(DtSnap sn, const uint32_t* __restrict__ field, long long n, const float* __restrict__ xyz, uint32_t* __restrict__ words,
                                                   u64* __restrict__ cnt) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  bool in = false;
  if (i < n) {
    int g[3] = {0, 0, 0};
    in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float p = xyz[3 * i + k], u = p / sn.voxel, b = floorf(u);
      const bool ok = dn_indexable(p, b);
      if (ok) g[k] = (int)b;
      in = in && ok && g[k] >= sn.lo[k] && g[k] < sn.hi[k];
    }
    uint32_t w = VDO_DISTANCE_OUTSIDE;
    if (in) w = field[((size_t)(g[2] - sn.lo[2]) * (size_t)(sn.hi[1] - sn.lo[1]) + (size_t)(g[1] - sn.lo[1])) * (size_t)(sn.hi[0] - sn.lo[0]) + (size_t)(g[0] - sn.lo[0])];
    words[i] = w;
  }
  dt_count(in ? 1 : 0, 2, cnt);
}

}  // namespace vdo

struct vdo_distance {
  vdo_ctx* ctx = nullptr;
  int64_t nvox = 0;
  int method = 0;
  bool has = false;                                                          // a snapshot exists
  int64_t nbox = 0;
  vdo::DtSnap snap{};
  uint32_t* d_field = nullptr; uint32_t* d_tmp = nullptr;                    // [nvox] the snapshot; the other side of the passes
  vdo::u64* d_bits = nullptr;                                                // [(nvox + 63) / 64] site bits in box order
  vdo::SlotCounts cnt;                                                       // [kDtSlots][kDtCounters]
  float* d_xyz = nullptr; uint32_t* d_words = nullptr;                       // [VDO_DISTANCE_WINDOW][3], [VDO_DISTANCE_WINDOW]: a window of host points
  vdo::StageTimer tm;
};

using namespace vdo;

static void dt_free(vdo_distance* h) {
  hipFree(h->d_field); hipFree(h->d_tmp); hipFree(h->d_bits); hipFree(h->d_xyz); hipFree(h->d_words);
  h->cnt.destroy();
  h->tm.destroy();
  delete h;
}

extern "C" int vdo_distance_create(vdo_ctx* ctx, const vdo_distance_params* p, vdo_distance** out) {
  static const char* who = "vdo_distance_create";
  if (!ctx) return set_error(VDO_ERR_INVALID, "%s: ctx is null", who);
  if (!p) return set_error(VDO_ERR_INVALID, "%s: params is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  int64_t nvox;
  int rc = dn_check_sides(who, p->n);
  if (rc == VDO_OK) rc = dn_check_size(who, p->n, &nvox);
  if (rc == VDO_OK) rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  vdo_distance* h = new vdo_distance;
  h->ctx = ctx; h->nvox = nvox;
  const size_t nv = (size_t)nvox;
  const bool ok = hipMalloc((void**)&h->d_field, nv * sizeof(uint32_t)) == hipSuccess && hipMalloc((void**)&h->d_tmp, nv * sizeof(uint32_t)) == hipSuccess &&
                  hipMalloc((void**)&h->d_bits, (nv + 63) / 64 * sizeof(u64)) == hipSuccess && h->cnt.create(kDtSlots, kDtCounters) &&
                  hipMalloc((void**)&h->d_xyz, (size_t)VDO_DISTANCE_WINDOW * 3 * sizeof(float)) == hipSuccess &&
                  hipMalloc((void**)&h->d_words, (size_t)VDO_DISTANCE_WINDOW * sizeof(uint32_t)) == hipSuccess && h->tm.create();
  if (!ok) {
    (void)hipGetLastError();
    dt_free(h);
    return set_error(VDO_ERR_OOM, "%s: device allocation failed for %d x %d x %d voxels", who, p->n[0], p->n[1], p->n[2]);
  }
  *out = h;
  return VDO_OK;
}

extern "C" int vdo_distance_destroy(vdo_distance* h) {
  if (!h) return VDO_OK;
  if (ctx_bind(h->ctx) == VDO_OK) hipStreamSynchronize(h->ctx->stream);
  dt_free(h);
  return VDO_OK;
}

// one axis pass over [outer][L][inner]; cnt non-null on the last one
static void dt_axis(const vdo_distance* h, hipStream_t s, const uint32_t* in, uint32_t* out, size_t inner, int L, size_t outer, int R, u64* cnt) {
  const int Re = R < L - 1 ? R : L - 1;                                      // no offset along the column is longer
  const uint32_t cap = (uint32_t)R * (uint32_t)R;
  const int method = h->method ? h->method : (Re <= kDtWinMax ? 1 : 2);
  if (method == 2) {
    const size_t ncol = inner * outer;
    hipLaunchKernelGGL(k_dt_axis_env, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, s, in, out, inner, L, ncol, cap, cnt);
    return;
  }
  const bool lds = 2 * Re + kDtMinTile <= kDtRows;
  int T = lds && kDtRows - 2 * Re < 64 ? kDtRows - 2 * Re : 64;
  if (T > L) T = (L + 3) / 4 * 4;
  const size_t tile = lds ? (size_t)(T + 2 * Re) * 64 * sizeof(uint32_t) : 0;
  const dim3 grid((unsigned)((inner + 63) / 64), (unsigned)((L + T - 1) / T), (unsigned)outer);
  if (lds) hipLaunchKernelGGL(k_dt_axis_win<true>, grid, dim3(256), tile, s, in, out, inner, L, Re, cap, T, cnt);
  else hipLaunchKernelGGL(k_dt_axis_win<false>, grid, dim3(256), 0, s, in, out, inner, L, Re, cap, T, cnt);
}

extern "C" int vdo_distance_compute(vdo_distance* h, vdo_dense* map, const int32_t lo[3], const int32_t hi[3], int min_weight, int radius, int64_t counts[3]) {
  static const char* who = "vdo_distance_compute";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!map) return set_error(VDO_ERR_INVALID, "%s: map is null", who);
  if (!lo) return set_error(VDO_ERR_INVALID, "%s: lo is null", who);
  if (!hi) return set_error(VDO_ERR_INVALID, "%s: hi is null", who);
  if (min_weight < 1 || min_weight > 255) return set_error(VDO_ERR_INVALID, "%s: min_weight %d outside 1..255", who, min_weight);
  if (radius < 1 || radius > 8191) return set_error(VDO_ERR_INVALID, "%s: radius %d outside 1..8191", who, radius);
  if (!counts) return set_error(VDO_ERR_INVALID, "%s: counts is null", who);
  if (map->ctx != h->ctx) return set_error(VDO_ERR_INVALID, "%s: map belongs to another context", who);
  DtArgs a;
  DtSnap sn;
  const DnClip clip = dn_clip(map, lo, hi);
  const int64_t nbox = clip.voxels();
  for (int k = 0; k < 3; ++k) {
    a.n[k] = map->a.n[k]; a.om[k] = map->a.om[k];
    a.blo[k] = clip.empty ? 0 : clip.box.lo[k] - map->a.o[k]; a.b[k] = clip.box.b[k];
    sn.lo[k] = clip.box.lo[k]; sn.hi[k] = clip.box.lo[k] + clip.box.b[k];
  }
  if (nbox > h->nvox)
    return set_error(VDO_ERR_INVALID, "%s: the clipped box of %d x %d x %d voxels is larger than the handle's %lld", who, a.b[0], a.b[1], a.b[2], (long long)h->nvox);
  sn.voxel = map->a.voxel;
  a.min_w = min_weight; a.R = radius; a.nbox = (unsigned)nbox;                // (2^31 voxels fit an unsigned index)
  int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const auto t0 = h->tm.begin(s);
  h->tm.ms[0] = h->tm.ms[1] = 0;
  if (nbox > 0) {
    const dim3 grid((unsigned)((nbox + 255) / 256)), block(256);
    h->cnt.zero(s);
    hipLaunchKernelGGL(k_dt_sites, grid, block, 0, s, a, (const uint32_t*)map->d_vol, h->d_bits, h->d_field, h->cnt.d);
    hipLaunchKernelGGL(k_dt_x, grid, block, 0, s, a, (const u64*)h->d_bits, h->d_field);
    dt_axis(h, s, h->d_field, h->d_tmp, (size_t)a.b[0], a.b[1], (size_t)a.b[2], radius, nullptr);
    dt_axis(h, s, h->d_tmp, h->d_field, (size_t)a.b[0] * a.b[1], a.b[2], 1, radius, h->cnt.d);
    h->tm.mark_end(s);
    h->cnt.download(s);
  } else {
    h->tm.mark_end(s);
  }
  h->has = true; h->nbox = nbox; h->snap = sn;                                // (the field's words are the new box's from the first kernel on)
  rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  counts[0] = nbox ? h->cnt.sum(0) : 0; counts[1] = nbox ? h->cnt.sum(1) : 0; counts[2] = nbox;
  h->tm.finish(t0);
  return VDO_OK;
}

extern "C" int vdo_distance_get(vdo_distance* h, uint32_t* words, int out_is_device, int32_t lo[3], int32_t hi[3]) {
  static const char* who = "vdo_distance_get";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!h->has) return set_error(VDO_ERR_INVALID, "%s: no field was computed yet", who);
  if (words && h->nbox > 0) {
    int rc = ctx_bind(h->ctx);
    if (rc != VDO_OK) return rc;
    hipStream_t s = h->ctx->stream;
    rc = check_hip(who, hipMemcpyAsync(words, h->d_field, (size_t)h->nbox * sizeof(uint32_t), out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (rc == VDO_OK) rc = sync_check(who, s);
    if (rc != VDO_OK) return rc;
  }
  for (int k = 0; k < 3; ++k) {
    if (lo) lo[k] = h->snap.lo[k];
    if (hi) hi[k] = h->snap.hi[k];
  }
  return VDO_OK;
}

extern "C" int vdo_distance_sample(vdo_distance* h, int64_t n, const float* xyz, uint32_t* words, int is_device, int64_t* n_inside) {
  static const char* who = "vdo_distance_sample";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (n < 0) return set_error(VDO_ERR_INVALID, "%s: n %lld < 0", who, (long long)n);
  if (n > 0 && !xyz) return set_error(VDO_ERR_INVALID, "%s: xyz is null", who);
  if (n > 0 && !words) return set_error(VDO_ERR_INVALID, "%s: words is null", who);
  if (!n_inside) return set_error(VDO_ERR_INVALID, "%s: n_inside is null", who);
  int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  const auto t0 = h->tm.begin(s);
  DtSnap sn = h->snap;
  if (!h->has) { for (int k = 0; k < 3; ++k) sn.lo[k] = sn.hi[k] = 0; sn.voxel = 1.f; }
  h->cnt.zero(s);
  // device points in windows of 2^30, host points through the staging lists, VDO_DISTANCE_WINDOW at a time
  const long long window = is_device ? kDtMaxWindow : (long long)VDO_DISTANCE_WINDOW;
  for (long long base = 0; base < n; base += window) {
    const long long cap = n - base < window ? n - base : window;
    const float* i_xyz = xyz + 3 * base;
    uint32_t* o_words = words + base;
    if (!is_device) {
      hipMemcpyAsync(h->d_xyz, xyz + 3 * base, (size_t)cap * 3 * sizeof(float), hipMemcpyHostToDevice, s);
      i_xyz = h->d_xyz; o_words = h->d_words;
    }
    hipLaunchKernelGGL(k_dt_sample, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, sn, (const uint32_t*)h->d_field, cap, i_xyz, o_words, h->cnt.d);
    if (!is_device) {
      hipMemcpyAsync(words + base, h->d_words, (size_t)cap * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
      rc = check_hip(who, hipStreamSynchronize(s));                          // the staging lists are free for the next window
      if (rc != VDO_OK) return rc;
    }
  }
  h->tm.mark_end(s);
  h->cnt.download(s);
  rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  *n_inside = h->cnt.sum(2);
  h->tm.finish(t0);
  return VDO_OK;
}

extern "C" int vdo_distance_device_field(vdo_distance* h, uint32_t** words) {
  static const char* who = "vdo_distance_device_field";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!words) return set_error(VDO_ERR_INVALID, "%s: words is null", who);
  *words = h->d_field;
  return VDO_OK;
}

extern "C" int vdo_distance_set_method(vdo_distance* h, int method) {
  static const char* who = "vdo_distance_set_method";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (method < 0 || method > 2) return set_error(VDO_ERR_INVALID, "%s: method %d is not 0, 1 or 2", who, method);
  h->method = method;
  return VDO_OK;
}

extern "C" int vdo_distance_last_timing(vdo_distance* h, double ms[2]) {
  return last_timing("vdo_distance_last_timing", h ? &h->tm : nullptr, ms);
}
