// Mesher: surface-nets triangles from a dense mapper's TSDF volume (the static map or an object's volume) - one vertex per active cell at the mean of
// its edge crossings, one quad (two triangles) per sign-changing lattice edge whose four cells are valid, vertices and quads in a fixed order.  The
// reference keeps no dense map; the semantics are this library's own, stated in include/vdo_slam_hip.h ("Mesher") and restated in NumPy by
// tests/mesh_ref.py.  A vertex is fp32 with one rounded operation per step (-ffp-contract=off), everything else is integer, and every thread works
// from its own integer index: no result depends on launch shape, schedule or the slot alignment of the cyclic volume.
//
// Thread i of every kernel stands for the voxel at LOCAL index l = g - o (x fastest) of the volume, 256 per workgroup, one wave = one 64-bit word of
// the two bit arrays:
//   k_ms_cells          the cell whose lower corner is the voxel: `valid` (8 corners inside the volume, w >= min_weight) and `emit` (active and selected
//                       by the box rule) as wave ballots, 1 bit per cell; the workgroup's emit count.
//   k_counts_scan       (scan.hpp) the exclusive scan of the workgroup counts, 64-bit carry, the total.
//   k_ms_verts          an emitting cell recomputes its vertex and writes it at blk[workgroup] + popcounts of the workgroup's earlier words + of the
//                       lanes below in its own word (ms_vnum), when that place lies in the window [base, base + cap).
//   k_ms_edges<FILL>    the lattice edges (voxel, k = 0, 1, 2): the four cells' validity from the `valid` bits, count per workgroup, scan, then the
//                       two triangles per quad, the vertex numbers by ms_vnum from the `emit` bits.
// There is no atomic and no 4-byte-per-cell index map: the order is the visiting order by construction.
//
// NO OUT-OF-RANGE ACCESS: a voxel is read only at local coordinates tested against n (its slot is then inside the volume); a bit of a neighbouring
// cell only after its local coordinates were tested against 0; an output only inside its window.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vdo_slam_hip.h"
#include "ctx.hpp"
#include "stage.hpp"
#include "dense.hpp"
#include "scan.hpp"

namespace vdo {

struct MsArgs {
  int n[3], om[3], o[3];                                                   // the map's size, origin mod size, origin
  int lo[3], hi[3];                                                        // the box clipped to the volume, LOCAL voxels; all 0 when it is empty
  int outside, min_w;
  unsigned nvox;
  float voxel;
};

__device__ __forceinline__ void ms_local(const MsArgs& a, unsigned i, int l[3]) {
  const unsigned nx = (unsigned)a.n[0], ny = (unsigned)a.n[1], r = i / nx;
  l[0] = (int)(i - r * nx); l[2] = (int)(r / ny); l[1] = (int)(r - (unsigned)l[2] * ny);
}

// the 8 corners of the cell at l (corner dx + 2 dy + 4 dz); false, nothing read, unless all of them are inside the volume
__device__ __forceinline__ bool ms_corners(const MsArgs& a, const uint32_t* __restrict__ vol, const int l[3], int t[8], int w[8]) {
  if (l[0] + 1 >= a.n[0] || l[1] + 1 >= a.n[1] || l[2] + 1 >= a.n[2]) return false;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const uint32_t v = dn_word(vol, a.n, a.om, l[0] + (c & 1), l[1] + (c >> 1 & 1), l[2] + (c >> 2));
    t[c] = dn_tsdf(v); w[c] = dn_weight(v);
  }
  return true;
}

// the cell's 8 corners inside the box shrunk by `shrink` voxels on every side
__device__ __forceinline__ bool ms_cell_in(const MsArgs& a, const int l[3], int shrink) {
  bool in = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) in = in && l[c] >= a.lo[c] + shrink && l[c] + 1 < a.hi[c] - shrink;
  return in;
}

// the number of the vertex of cell ci (whose emit bit is set) among the emitted ones
__device__ __forceinline__ long long ms_vnum(const u64* __restrict__ emit, const long long* __restrict__ blkv, unsigned ci) {
  const unsigned wd = ci >> 6;
  long long v = blkv[ci >> 8];
  for (unsigned q = wd & ~3u; q < wd; ++q) v += __popcll(emit[q]);
  return v + __popcll(emit[wd] & ((1ull << (ci & 63u)) - 1ull));
}

__global__ __launch_bounds__(256) void k_ms_cells(MsArgs a, const uint32_t* __restrict__ vol, u64* __restrict__ valid, u64* __restrict__ emit, long long* __restrict__ blkv) {
  __shared__ int cnt[4];
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  bool ok = false, em = false;
  if (i < a.nvox) {
    int l[3], t[8], w[8];
    ms_local(a, i, l);
    if (ms_corners(a, vol, l, t, w)) {
      int wmin = w[0], neg = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) { wmin = w[c] < wmin ? w[c] : wmin; neg += t[c] < 0; }
      ok = wmin >= a.min_w;
      em = ok && neg != 0 && neg != 8 && (a.outside ? !ms_cell_in(a, l, 1) : ms_cell_in(a, l, 0));
    }
  }
  const u64 bv = __ballot(ok), be = __ballot(em);
  const unsigned wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) { valid[i >> 6] = bv; emit[i >> 6] = be; cnt[wave] = (int)__popcll(be); }
  __syncthreads();
  if (threadIdx.x == 0) blkv[blockIdx.x] = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
}

__global__ __launch_bounds__(256) void k_ms_verts(MsArgs a, const uint32_t* __restrict__ vol, const u64* __restrict__ emit, const long long* __restrict__ blkv, long long base,
                                                  long long cap, float* __restrict__ xyz, int32_t* __restrict__ grad, int32_t* __restrict__ wgt) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.nvox || !(emit[i >> 6] >> (i & 63u) & 1ull)) return;
  const long long pos = ms_vnum(emit, blkv, i);
  if (pos < base || pos >= base + cap) return;
  int l[3], t[8], w[8];
  ms_local(a, i, l);
  if (!ms_corners(a, vol, l, t, w)) return;                                  // (an emitting cell has its corners inside)
  float s[3] = {0.f, 0.f, 0.f};
  int m = 0, g[3] = {0, 0, 0}, wmin = w[0];
#pragma unroll
  for (int c = 0; c < 8; ++c) wmin = w[c] < wmin ? w[c] : wmin;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int ai = (k + 1) % 3, aj = (k + 2) % 3;
#pragma unroll
    for (int dj = 0; dj < 2; ++dj)
#pragma unroll
      for (int di = 0; di < 2; ++di) {
        const int ca = (di << ai) | (dj << aj), ta = t[ca], tb = t[ca | (1 << k)];
        g[k] += tb - ta;
        if ((ta < 0) != (tb < 0)) {
          const float frac = (float)ta / (float)(ta - tb);
          float p[3];
          p[ai] = (float)di; p[aj] = (float)dj; p[k] = 0.f + frac;
          s[0] += p[0]; s[1] += p[1]; s[2] += p[2];
          ++m;
        }
      }
  }
  const long long r = pos - base;
  const float fm = (float)m;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float mean = s[c] / fm;
    xyz[3 * r + c] = (((float)(a.o[c] + l[c]) + 0.5f) + mean) * a.voxel;
    grad[3 * r + c] = g[c];
  }
  wgt[r] = wmin;
}

// Voxel i as the lower end a of its three lattice edges.  !FILL: the workgroup's number of quads.  FILL: the triangles whose place lies in
// [base, base + cap) are written at place - base.
template <bool FILL>
__global__ __launch_bounds__(256) void k_ms_edges(MsArgs a, const uint32_t* __restrict__ vol, const u64* __restrict__ valid, const u64* __restrict__ emit,
                                                  const long long* __restrict__ blkv, long long* __restrict__ blke, long long base, long long cap, int32_t* __restrict__ tri) {
  __shared__ int lds[17];
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const unsigned st[3] = {1u, (unsigned)a.n[0], (unsigned)a.n[0] * (unsigned)a.n[1]};
  int cross = 0, l[3] = {0, 0, 0}, ta = 0;
  // every quad of a uses the cell at a itself: nothing to do unless that cell is valid, and then a and a + e_k are inside with w >= min_weight
  if (i < a.nvox && (valid[i >> 6] >> (i & 63u) & 1ull)) {
    ms_local(a, i, l);
    ta = (int)(int16_t)(dn_word(vol, a.n, a.om, l[0], l[1], l[2]) & 0xffffu);   // dn_tsdf, spelled out here and for tb: the call costs k_ms_edges<true> two instructions
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int ai = (k + 1) % 3, aj = (k + 2) % 3;
      if (l[ai] < 1 || l[aj] < 1) continue;
      const unsigned c1 = i - st[ai], c2 = i - st[aj], c3 = i - st[ai] - st[aj];
      if (!((valid[c1 >> 6] >> (c1 & 63u)) & (valid[c2 >> 6] >> (c2 & 63u)) & (valid[c3 >> 6] >> (c3 & 63u)) & 1ull)) continue;
      int b[3] = {l[0], l[1], l[2]};
      b[k] += 1;
      const int tb = (int)(int16_t)(dn_word(vol, a.n, a.om, b[0], b[1], b[2]) & 0xffffu);
      if ((ta < 0) == (tb < 0)) continue;
      // the 3 x 3 x 2 corner block inside the box
      const bool in = l[ai] - 1 >= a.lo[ai] && l[ai] + 1 < a.hi[ai] && l[aj] - 1 >= a.lo[aj] && l[aj] + 1 < a.hi[aj] && l[k] >= a.lo[k] && l[k] + 1 < a.hi[k];
      if (a.outside ? !in : in) cross |= 1 << k;
    }
  }
  int total;
  const int ex = block_excl_scan(__popc(cross), lds, &total);
  if (!FILL) {
    if (threadIdx.x == 0) blke[blockIdx.x] = total;
    return;
  }
  long long pos = 2 * (blke[blockIdx.x] + ex);                              // in triangles
  if (pos >= base + cap) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!(cross >> k & 1)) continue;
    if (pos + 2 > base && pos < base + cap) {
      const int ai = (k + 1) % 3, aj = (k + 2) % 3;
      // (d_i, d_j) = (1, 1), (0, 1), (0, 0), (1, 0), reversed when ta >= 0
      int v[4];
      v[0] = (int)ms_vnum(emit, blkv, i - st[ai] - st[aj]); v[1] = (int)ms_vnum(emit, blkv, i - st[aj]);
      v[2] = (int)ms_vnum(emit, blkv, i); v[3] = (int)ms_vnum(emit, blkv, i - st[ai]);
      if (ta >= 0) { int q = v[0]; v[0] = v[3]; v[3] = q; q = v[1]; v[1] = v[2]; v[2] = q; }
      if (pos >= base) { int32_t* o = tri + 3 * (pos - base); o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; }
      if (pos + 1 < base + cap) { int32_t* o = tri + 3 * (pos + 1 - base); o[0] = v[0]; o[1] = v[2]; o[2] = v[3]; }
    }
    pos += 2;
  }
}

}  // namespace vdo

struct vdo_mesh {
  vdo_ctx* ctx = nullptr;
  int64_t nvox = 0, nblk = 0, stage_v = 0, stage_t = 0;
  vdo::u64* d_valid = nullptr; vdo::u64* d_emit = nullptr;                   // [4 * nblk] words: 1 bit per cell
  long long* d_blkv = nullptr; long long* d_blke = nullptr;                  // [nblk] per workgroup: emitted cells, quads; then their exclusive scans
  unsigned long long* d_tot = nullptr;                                       // vertices, quads
  unsigned long long* h_tot = nullptr;                                       // pinned
  float* d_xyz = nullptr; int32_t* d_grad = nullptr; int32_t* d_wgt = nullptr;      // [stage_v] staging of host outputs
  int32_t* d_tri = nullptr;                                                  // [stage_t][3]
  vdo::StageTimer tm;
};

using namespace vdo;

static void ms_free(vdo_mesh* h) {
  hipFree(h->d_valid); hipFree(h->d_emit); hipFree(h->d_blkv); hipFree(h->d_blke); hipFree(h->d_tot); hipFree(h->d_xyz); hipFree(h->d_grad); hipFree(h->d_wgt); hipFree(h->d_tri);
  if (h->h_tot) hipHostFree(h->h_tot);
  h->tm.destroy();
  delete h;
}

extern "C" int vdo_mesh_create(vdo_ctx* ctx, const vdo_mesh_params* p, vdo_mesh** out) {
  static const char* who = "vdo_mesh_create";
  if (!ctx) return set_error(VDO_ERR_INVALID, "%s: ctx is null", who);
  if (!p) return set_error(VDO_ERR_INVALID, "%s: params is null", who);
  if (!out) return set_error(VDO_ERR_INVALID, "%s: out is null", who);
  int rc = dn_check_sides(who, p->n);
  if (rc != VDO_OK) return rc;
  if (p->stage_vertices < 1) return set_error(VDO_ERR_INVALID, "%s: stage_vertices %d < 1", who, p->stage_vertices);
  if (p->stage_triangles < 1) return set_error(VDO_ERR_INVALID, "%s: stage_triangles %d < 1", who, p->stage_triangles);
  int64_t nvox;
  rc = dn_check_size(who, p->n, &nvox);
  if (rc == VDO_OK) rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  vdo_mesh* h = new vdo_mesh;
  h->ctx = ctx; h->nvox = nvox; h->nblk = (nvox + 255) / 256; h->stage_v = p->stage_vertices; h->stage_t = p->stage_triangles;
  const size_t nb = (size_t)h->nblk, sv = (size_t)h->stage_v, stt = (size_t)h->stage_t;
  const bool ok = hipMalloc((void**)&h->d_valid, nb * 4 * sizeof(u64)) == hipSuccess && hipMalloc((void**)&h->d_emit, nb * 4 * sizeof(u64)) == hipSuccess &&
                  hipMalloc((void**)&h->d_blkv, nb * sizeof(long long)) == hipSuccess && hipMalloc((void**)&h->d_blke, nb * sizeof(long long)) == hipSuccess &&
                  hipMalloc((void**)&h->d_tot, 2 * sizeof(unsigned long long)) == hipSuccess && hipMalloc((void**)&h->d_xyz, sv * 3 * sizeof(float)) == hipSuccess &&
                  hipMalloc((void**)&h->d_grad, sv * 3 * sizeof(int32_t)) == hipSuccess && hipMalloc((void**)&h->d_wgt, sv * sizeof(int32_t)) == hipSuccess &&
                  hipMalloc((void**)&h->d_tri, stt * 3 * sizeof(int32_t)) == hipSuccess &&
                  hipHostMalloc((void**)&h->h_tot, 2 * sizeof(unsigned long long), hipHostMallocDefault) == hipSuccess && h->tm.create();
  if (!ok) {
    (void)hipGetLastError();
    ms_free(h);
    return set_error(VDO_ERR_OOM, "%s: device allocation failed for %d x %d x %d cells", who, p->n[0], p->n[1], p->n[2]);
  }
  *out = h;
  return VDO_OK;
}

extern "C" int vdo_mesh_destroy(vdo_mesh* h) {
  if (!h) return VDO_OK;
  if (ctx_bind(h->ctx) == VDO_OK) hipStreamSynchronize(h->ctx->stream);
  ms_free(h);
  return VDO_OK;
}

extern "C" int vdo_mesh_extract(vdo_mesh* h, vdo_dense* map, const int32_t lo[3], const int32_t hi[3], int outside, int min_weight, int64_t vertex_capacity, float* xyz, int32_t* grad,
                                int32_t* weight, int64_t triangle_capacity, int32_t* tri, int out_is_device, int64_t counts[2]) {
  static const char* who = "vdo_mesh_extract";
  if (!h) return set_error(VDO_ERR_INVALID, "%s: handle is null", who);
  if (!map) return set_error(VDO_ERR_INVALID, "%s: map is null", who);
  if (!lo) return set_error(VDO_ERR_INVALID, "%s: lo is null", who);
  if (!hi) return set_error(VDO_ERR_INVALID, "%s: hi is null", who);
  if (min_weight < 1) return set_error(VDO_ERR_INVALID, "%s: min_weight %d < 1", who, min_weight);
  if (vertex_capacity < 0) return set_error(VDO_ERR_INVALID, "%s: vertex_capacity %lld < 0", who, (long long)vertex_capacity);
  if (triangle_capacity < 0) return set_error(VDO_ERR_INVALID, "%s: triangle_capacity %lld < 0", who, (long long)triangle_capacity);
  if (vertex_capacity > 0 && !xyz) return set_error(VDO_ERR_INVALID, "%s: xyz is null", who);
  if (vertex_capacity > 0 && !grad) return set_error(VDO_ERR_INVALID, "%s: grad is null", who);
  if (vertex_capacity > 0 && !weight) return set_error(VDO_ERR_INVALID, "%s: weight is null", who);
  if (triangle_capacity > 0 && !tri) return set_error(VDO_ERR_INVALID, "%s: tri is null", who);
  if (!counts) return set_error(VDO_ERR_INVALID, "%s: counts is null", who);
  if (map->ctx != h->ctx) return set_error(VDO_ERR_INVALID, "%s: map belongs to another context", who);
  if (map->nvox > h->nvox)
    return set_error(VDO_ERR_INVALID, "%s: map of %d x %d x %d voxels is larger than the mesher's %lld", who, map->a.n[0], map->a.n[1], map->a.n[2], (long long)h->nvox);
  int rc = ctx_bind(h->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = h->ctx->stream;
  MsArgs a;
  const DnClip clip = dn_clip(map, lo, hi);
  for (int k = 0; k < 3; ++k) {
    a.n[k] = map->a.n[k]; a.o[k] = map->a.o[k]; a.om[k] = map->a.om[k];
    a.lo[k] = clip.empty ? 0 : clip.box.lo[k] - a.o[k]; a.hi[k] = a.lo[k] + clip.box.b[k];
  }
  a.outside = outside ? 1 : 0; a.min_w = min_weight; a.nvox = (unsigned)map->nvox; a.voxel = map->a.voxel;   // (2^31 voxels fit an unsigned index)
  const uint32_t* vol = map->d_vol;
  const long long nblk = (map->nvox + 255) / 256;
  const dim3 grid((unsigned)nblk), block(256);
  const auto t0 = h->tm.begin(s);
  h->tm.ms[0] = h->tm.ms[1] = 0;                                             // a call that ends in an error reports 0, 0, not the last call's times
  hipLaunchKernelGGL(k_ms_cells, grid, block, 0, s, a, vol, h->d_valid, h->d_emit, h->d_blkv);
  hipLaunchKernelGGL(k_counts_scan<1024>, dim3(1), dim3(1024), 0, s, h->d_blkv, nblk, h->d_tot);
  hipLaunchKernelGGL(k_ms_edges<false>, grid, block, 0, s, a, vol, (const u64*)h->d_valid, (const u64*)h->d_emit, (const long long*)h->d_blkv, h->d_blke, 0LL, 0LL, (int32_t*)nullptr);
  hipLaunchKernelGGL(k_counts_scan<1024>, dim3(1), dim3(1024), 0, s, h->d_blke, nblk, h->d_tot + 1);
  hipMemcpyAsync(h->h_tot, h->d_tot, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
  rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  const long long nv = (long long)h->h_tot[0], nt = 2 * (long long)h->h_tot[1];
  if (nv > INT32_MAX || nt > INT32_MAX) return set_error(VDO_ERR_UNSUPPORTED, "%s: %lld vertices, %lld triangles: a count passes 2^31 - 1", who, nv, nt);
  const long long want_v = nv < vertex_capacity ? nv : vertex_capacity, want_t = nt < triangle_capacity ? nt : triangle_capacity;
  // a device output is one window; a host output goes through the staging lists, stage_vertices / stage_triangles at a time
  for (long long base = 0; base < want_v; base += out_is_device ? want_v : h->stage_v) {
    const long long cap = out_is_device ? want_v : (want_v - base < h->stage_v ? want_v - base : h->stage_v);
    hipLaunchKernelGGL(k_ms_verts, grid, block, 0, s, a, vol, (const u64*)h->d_emit, (const long long*)h->d_blkv, base, cap, out_is_device ? xyz : h->d_xyz,
                       out_is_device ? grad : h->d_grad, out_is_device ? weight : h->d_wgt);
    if (!out_is_device) {
      hipMemcpyAsync(xyz + 3 * base, h->d_xyz, (size_t)cap * 3 * sizeof(float), hipMemcpyDeviceToHost, s);
      hipMemcpyAsync(grad + 3 * base, h->d_grad, (size_t)cap * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s);
      hipMemcpyAsync(weight + base, h->d_wgt, (size_t)cap * sizeof(int32_t), hipMemcpyDeviceToHost, s);
      rc = check_hip(who, hipStreamSynchronize(s));                          // the staging lists are free for the next window
      if (rc != VDO_OK) return rc;
    }
  }
  for (long long base = 0; base < want_t; base += out_is_device ? want_t : h->stage_t) {
    const long long cap = out_is_device ? want_t : (want_t - base < h->stage_t ? want_t - base : h->stage_t);
    hipLaunchKernelGGL(k_ms_edges<true>, grid, block, 0, s, a, vol, (const u64*)h->d_valid, (const u64*)h->d_emit, (const long long*)h->d_blkv, h->d_blke, base, cap,
                       out_is_device ? tri : h->d_tri);
    if (!out_is_device) {
      hipMemcpyAsync(tri + 3 * base, h->d_tri, (size_t)cap * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s);
      rc = check_hip(who, hipStreamSynchronize(s));
      if (rc != VDO_OK) return rc;
    }
  }
  h->tm.mark_end(s);
  rc = sync_check(who, s);
  if (rc != VDO_OK) return rc;
  counts[0] = nv; counts[1] = nt;
  h->tm.finish(t0);
  return VDO_OK;
}

extern "C" int vdo_mesh_last_timing(vdo_mesh* h, double ms[2]) {
  return last_timing("vdo_mesh_last_timing", h ? &h->tm : nullptr, ms);
}
