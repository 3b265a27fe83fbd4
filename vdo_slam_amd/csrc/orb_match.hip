// ORB descriptor matcher: gated brute-force Hamming search over two sets of 256-bit rotated-BRIEF rows (the consumer of K8, orb.hip).
// The reference carries the ORB-SLAM2 skeleton such a matcher plugs into (mDescriptors, mvKeysUn, the feature grid) but no matcher; the
// semantics are this library's own, stated in include/vdo_slam_hip.h (vdo_orb_match) and restated in NumPy by tests/matching_ref.py.
// Integer arithmetic end to end: the only fp32 operations are the window gate (one subtraction per axis) and the ratio test (one multiply).
//
//   k_match_partial   grid (ceil(nQ/256), n_chunks), one query per thread: descriptor, position and octave in registers; the chunk's train
//                     rows go through LDS in tiles of 256 (11 KB) and every lane reads the SAME row (a broadcast: no bank conflict); per pair
//                     4 XOR + 4 popcounts.  The running best is the packed key (dist << 32) | j kept by min - the lowest index wins ties
//                     without a compare of its own - with the second-smallest distance beside it.  Writes (key, second) to [chunk][nQ].
//   k_match_finalize  one thread per query folds the chunks (best = min key, second = min(max(b1, b2), s1, s2)), applies the distance,
//                     ratio and cross-check filters, writes the three outputs and counts the matches (wave ballot, one atomicAdd per wave).
//   cross-check       the reverse bests are a second k_match_partial launch with the roles swapped, folded to rev_best[nT] by k_match_rev_merge.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/vdo_slam_hip.h"
#include "arena.hpp"
#include "ctx.hpp"
#include "orb_match.hpp"

namespace vdo {

constexpr int kMatchThreads = 256;          // queries per workgroup
constexpr int kMatchTile = 256;             // train rows staged in LDS at a time
constexpr uint64_t kNoKey = ~uint64_t(0);   // no candidate yet (larger than every (dist << 32) | j)
constexpr uint32_t kNoDist = ~uint32_t(0);  // no second candidate yet; also the distance half of kNoKey
constexpr int kMatchMaxRows = 1 << 24;
constexpr size_t kMatchMaxScratch = size_t(1) << 30;

struct MatchSet { int n; const uint64_t* desc; const float *x, *y; const int32_t* oct; };

// GATED = false: every train row is a candidate (no position / octave is read).  use_window / max_oct < 0 switch the two gates singly.
template <bool GATED>
__global__ __launch_bounds__(kMatchThreads) void k_match_partial(MatchSet Q, MatchSet T, int chunk_rows, float window, int use_window, long long max_oct,
                                                                 uint64_t* __restrict__ pkey, uint32_t* __restrict__ psec) {
  __shared__ uint64_t s_desc[kMatchTile][4];
  __shared__ float s_x[kMatchTile], s_y[kMatchTile];
  __shared__ int32_t s_o[kMatchTile];
  const int i = blockIdx.x * kMatchThreads + threadIdx.x;
  const bool live = i < Q.n;
  uint64_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;
  float qx = 0.f, qy = 0.f;
  long long qo = 0;
  if (live) {
    const uint64_t* d = Q.desc + (size_t)i * 4;
    q0 = d[0]; q1 = d[1]; q2 = d[2]; q3 = d[3];
    if (GATED) {
      if (use_window) { qx = Q.x[i]; qy = Q.y[i]; }
      if (max_oct >= 0) qo = Q.oct[i];
    }
  }
  const long long c0 = (long long)blockIdx.y * chunk_rows;
  const int c1 = c0 + chunk_rows < T.n ? (int)(c0 + chunk_rows) : T.n;
  uint64_t best = kNoKey;
  uint32_t second = kNoDist;
  for (int t0 = (int)c0; t0 < c1; t0 += kMatchTile) {
    const int rows = min(kMatchTile, c1 - t0);
    __syncthreads();                                  // the tile before this one has been read by every lane
    if ((int)threadIdx.x < rows) {
      const int j = t0 + threadIdx.x;
      const uint64_t* d = T.desc + (size_t)j * 4;
      s_desc[threadIdx.x][0] = d[0]; s_desc[threadIdx.x][1] = d[1]; s_desc[threadIdx.x][2] = d[2]; s_desc[threadIdx.x][3] = d[3];
      if (GATED) {
        if (use_window) { s_x[threadIdx.x] = T.x[j]; s_y[threadIdx.x] = T.y[j]; }
        if (max_oct >= 0) s_o[threadIdx.x] = T.oct[j];
      }
    }
    __syncthreads();
    if (!live) continue;
#pragma unroll 4
    for (int r = 0; r < rows; ++r) {
      if (GATED) {
        // one fp32 subtraction, fabsf and compare per axis (a NaN position fails the compare); octave difference in 64 bits (no int32 wrap)
        if (use_window && !(fabsf(s_x[r] - qx) <= window && fabsf(s_y[r] - qy) <= window)) continue;
        if (max_oct >= 0) { long long dd = (long long)s_o[r] - qo; if (dd < 0) dd = -dd; if (dd > max_oct) continue; }
      }
      const uint32_t d = (uint32_t)(__popcll(q0 ^ s_desc[r][0]) + __popcll(q1 ^ s_desc[r][1]) + __popcll(q2 ^ s_desc[r][2]) + __popcll(q3 ^ s_desc[r][3]));
      const uint64_t key = ((uint64_t)d << 32) | (uint32_t)(t0 + r);
      second = min(second, max(d, (uint32_t)(best >> 32)));     // the larger of (this, best so far) is a runner-up; kNoDist while there is no best
      best = min(best, key);
    }
  }
  if (live) {
    const size_t o = (size_t)blockIdx.y * Q.n + i;
    pkey[o] = best; psec[o] = second;
  }
}

// Fold of the chunk partials of one row, in chunk order
__device__ __forceinline__ void match_fold(const uint64_t* __restrict__ pkey, const uint32_t* __restrict__ psec, int n, int n_chunks, int i, uint64_t* best_out,
                                           uint32_t* second_out) {
  uint64_t best = kNoKey;
  uint32_t second = kNoDist;
  for (int c = 0; c < n_chunks; ++c) {
    const uint64_t k = pkey[(size_t)c * n + i];
    const uint32_t s = psec[(size_t)c * n + i];
    second = min(min(second, s), max((uint32_t)(best >> 32), (uint32_t)(k >> 32)));
    best = min(best, k);
  }
  *best_out = best; *second_out = second;
}

// rev_best[j]: the query a train row is closest to (lowest index on ties), -1 without a candidate
__global__ __launch_bounds__(256) void k_match_rev_merge(int nT, int n_chunks, const uint64_t* __restrict__ pkey, const uint32_t* __restrict__ psec,
                                                         int32_t* __restrict__ rev_best) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nT) return;
  uint64_t best; uint32_t second;
  match_fold(pkey, psec, nT, n_chunks, j, &best, &second);
  rev_best[j] = best == kNoKey ? -1 : (int32_t)(uint32_t)best;
}

__global__ __launch_bounds__(256) void k_match_finalize(int nQ, int n_chunks, const uint64_t* __restrict__ pkey, const uint32_t* __restrict__ psec,
                                                        const int32_t* __restrict__ rev_best, int max_distance, float ratio, int use_ratio,
                                                        int32_t* __restrict__ train_idx, int32_t* __restrict__ best_dist, int32_t* __restrict__ second_dist,
                                                        int* __restrict__ n_matches) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool ok = false;
  if (i < nQ) {
    uint64_t best; uint32_t second;
    match_fold(pkey, psec, nQ, n_chunks, i, &best, &second);
    int32_t j = -1, bd = -1, sd = -1;
    if (best != kNoKey) {
      j = (int32_t)(uint32_t)best; bd = (int32_t)(best >> 32);
      if (second != kNoDist) sd = (int32_t)second;
      ok = bd <= max_distance;
      if (ok && use_ratio && sd >= 0) ok = (float)bd < ratio * (float)sd;     // one fp32 multiply, strict
      if (ok && rev_best) ok = rev_best[j] == i;
    }
    train_idx[i] = ok ? j : -1; best_dist[i] = bd; second_dist[i] = sd;
  }
  const unsigned long long m = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_matches, (int)__popcll(m));
}

struct MatchPlan { int chunk_rows, n_chunks; };

// Train rows per chunk.  asked >= 1: exactly that.  0: enough chunks that the grid has about two workgroups for each of the 256 CUs (10 query blocks x 52
// chunks of 49 rows at 2 500 x 2 500), but no chunk shorter than 32 rows - below that a workgroup stages more than it compares.
static MatchPlan match_plan(int nQ, int nT, int asked) {
  MatchPlan p;
  if (asked >= 1) p.chunk_rows = asked;
  else {
    const int qb = (nQ + kMatchThreads - 1) / kMatchThreads;
    const int want = (2 * 256 + qb - 1) / qb;
    p.chunk_rows = std::max((nT + want - 1) / want, 32);
  }
  p.n_chunks = (int)(((long long)nT + p.chunk_rows - 1) / p.chunk_rows);
  return p;
}

static size_t pad256(size_t b) { return (b + 255) & ~size_t(255); }

static int match_check_params(const char* who, const vdo_match_params* p) {
  if (!p) return set_error(VDO_ERR_INVALID, "%s: params is null", who);
  if (p->max_distance < 0 || p->max_distance > 256) return set_error(VDO_ERR_INVALID, "%s: max_distance %d outside 0..256", who, p->max_distance);
  if (std::isnan(p->ratio)) return set_error(VDO_ERR_INVALID, "%s: ratio is NaN", who);
  if (std::isnan(p->window)) return set_error(VDO_ERR_INVALID, "%s: window is NaN", who);
  if (p->chunk_rows < 0) return set_error(VDO_ERR_INVALID, "%s: chunk_rows %d is negative", who, p->chunk_rows);
  return VDO_OK;
}

static int match_check_outputs(const char* who, const int32_t* train_idx, const int32_t* best_dist, const int32_t* second_dist, const int32_t* n_matches) {
  if (!train_idx) return set_error(VDO_ERR_INVALID, "%s: train_idx is null", who);
  if (!best_dist) return set_error(VDO_ERR_INVALID, "%s: best_dist is null", who);
  if (!second_dist) return set_error(VDO_ERR_INVALID, "%s: second_dist is null", who);
  if (!n_matches) return set_error(VDO_ERR_INVALID, "%s: n_matches is null", who);
  return VDO_OK;
}

static void match_fill_none(int n, int32_t* train_idx, int32_t* best_dist, int32_t* second_dist, int32_t* n_matches) {
  std::fill(train_idx, train_idx + n, -1); std::fill(best_dist, best_dist + n, -1); std::fill(second_dist, second_dist + n, -1);
  *n_matches = 0;
}

// Scratch one match takes from the context's arena besides its staged inputs: both partial stores, rev_best, the outputs and the count
static size_t match_scratch_bytes(int nQ, int nT, const MatchPlan& f, const MatchPlan& r, bool cross) {
  size_t b = pad256(8 * (size_t)f.n_chunks * nQ) + pad256(4 * (size_t)f.n_chunks * nQ) + 3 * pad256(4 * (size_t)nQ) + 256;
  if (cross) b += pad256(8 * (size_t)r.n_chunks * nT) + pad256(4 * (size_t)r.n_chunks * nT) + pad256(4 * (size_t)nT);
  return b;
}

static int match_check_plan(const char* who, int nQ, int nT, const MatchPlan& f, const MatchPlan& r, bool cross) {
  if (f.n_chunks > 65535 || (cross && r.n_chunks > 65535) || match_scratch_bytes(nQ, nT, f, r, cross) > kMatchMaxScratch)
    return set_error(VDO_ERR_UNSUPPORTED, "%s: chunk_rows too small for %d x %d rows (more than 65535 chunks or 1 GiB of partial results)", who, nQ, nT);
  return VDO_OK;
}

// The launches of one match on the arena's stream, inputs resident (Q, T: device pointers).  Queues the downloads; the caller finishes the arena.
static int match_launch(const char* who, Arena& A, const MatchSet& Q, const MatchSet& T, const vdo_match_params& p, const MatchPlan& f, const MatchPlan& r,
                        int32_t* train_idx, int32_t* best_dist, int32_t* second_dist, int32_t* n_matches) {
  const int nQ = Q.n, nT = T.n;
  const bool cross = p.cross_check != 0;
  const int use_window = p.window >= 0.f;
  const long long max_oct = p.max_octave_diff >= 0 ? p.max_octave_diff : -1;
  const bool gated = use_window || max_oct >= 0;
  uint64_t* fkey = A.up<uint64_t>(nullptr, (size_t)f.n_chunks * nQ);
  uint32_t* fsec = A.up<uint32_t>(nullptr, (size_t)f.n_chunks * nQ);
  uint64_t* rkey = nullptr; uint32_t* rsec = nullptr; int32_t* rev = nullptr;
  if (cross) {
    rkey = A.up<uint64_t>(nullptr, (size_t)r.n_chunks * nT);
    rsec = A.up<uint32_t>(nullptr, (size_t)r.n_chunks * nT);
    rev = A.up<int32_t>(nullptr, (size_t)nT);
  }
  int32_t* d_idx = A.up<int32_t>(nullptr, nQ);
  int32_t* d_best = A.up<int32_t>(nullptr, nQ);
  int32_t* d_second = A.up<int32_t>(nullptr, nQ);
  int* d_count = A.up<int>(nullptr, 1);
  if (!fkey || !fsec || !d_idx || !d_best || !d_second || !d_count || (cross && (!rkey || !rsec || !rev))) return set_error(VDO_ERR_OOM, "%s: scratch arena exhausted", who);
  hipStream_t s = A.stream();
  hipMemsetAsync(d_count, 0, sizeof(int), s);
  const dim3 gf((nQ + kMatchThreads - 1) / kMatchThreads, f.n_chunks), gr((nT + kMatchThreads - 1) / kMatchThreads, r.n_chunks);
  if (gated) {
    hipLaunchKernelGGL(k_match_partial<true>, gf, dim3(kMatchThreads), 0, s, Q, T, f.chunk_rows, p.window, use_window, max_oct, fkey, fsec);
    if (cross) hipLaunchKernelGGL(k_match_partial<true>, gr, dim3(kMatchThreads), 0, s, T, Q, r.chunk_rows, p.window, use_window, max_oct, rkey, rsec);
  } else {
    hipLaunchKernelGGL(k_match_partial<false>, gf, dim3(kMatchThreads), 0, s, Q, T, f.chunk_rows, 0.f, 0, -1LL, fkey, fsec);
    if (cross) hipLaunchKernelGGL(k_match_partial<false>, gr, dim3(kMatchThreads), 0, s, T, Q, r.chunk_rows, 0.f, 0, -1LL, rkey, rsec);
  }
  if (cross) hipLaunchKernelGGL(k_match_rev_merge, dim3((nT + 255) / 256), dim3(256), 0, s, nT, r.n_chunks, (const uint64_t*)rkey, (const uint32_t*)rsec, rev);
  const int use_ratio = p.ratio > 0.f && p.ratio < 1.f;
  hipLaunchKernelGGL(k_match_finalize, dim3((nQ + 255) / 256), dim3(256), 0, s, nQ, f.n_chunks, (const uint64_t*)fkey, (const uint32_t*)fsec, (const int32_t*)rev,
                     p.max_distance, p.ratio, use_ratio, d_idx, d_best, d_second, d_count);
  A.down(train_idx, d_idx, nQ); A.down(best_dist, d_best, nQ); A.down(second_dist, d_second, nQ); A.down(n_matches, d_count, 1);
  return VDO_OK;
}

static int match_check_set(const char* who, const char* name, const vdo_match_set* m) {
  if (!m) return set_error(VDO_ERR_INVALID, "%s: %s is null", who, name);
  if (m->n < 0 || m->n > kMatchMaxRows) return set_error(VDO_ERR_INVALID, "%s: %s->n %d outside 0..%d", who, name, m->n, kMatchMaxRows);
  if (!m->desc) return set_error(VDO_ERR_INVALID, "%s: %s->desc is null", who, name);
  if (m->is_device && ((uintptr_t)m->desc & 7)) return set_error(VDO_ERR_INVALID, "%s: %s->desc: a device pointer must be 8-byte aligned", who, name);
  return VDO_OK;
}

}  // namespace vdo

using namespace vdo;

extern "C" int vdo_orb_match(vdo_ctx* ctx, const vdo_match_set* query, const vdo_match_set* train, const vdo_match_params* prm, int32_t* train_idx,
                             int32_t* best_dist, int32_t* second_dist, int32_t* n_matches) {
  static const char* who = "vdo_orb_match";
  if (!ctx) return set_error(VDO_ERR_INVALID, "%s: ctx is null", who);
  int rc = match_check_set(who, "query", query);
  if (rc == VDO_OK) rc = match_check_set(who, "train", train);
  if (rc == VDO_OK) rc = match_check_params(who, prm);
  if (rc == VDO_OK) rc = match_check_outputs(who, train_idx, best_dist, second_dist, n_matches);
  if (rc != VDO_OK) return rc;
  if (prm->window >= 0.f && !(query->x && query->y && train->x && train->y))
    return set_error(VDO_ERR_INVALID, "%s: window >= 0 needs x and y on both sets (%s is null)", who,
                     !query->x ? "query->x" : !query->y ? "query->y" : !train->x ? "train->x" : "train->y");
  if (prm->max_octave_diff >= 0 && !(query->octave && train->octave))
    return set_error(VDO_ERR_INVALID, "%s: max_octave_diff >= 0 needs octave on both sets (%s is null)", who, !query->octave ? "query->octave" : "train->octave");
  const int nQ = query->n, nT = train->n;
  if (nQ == 0 || nT == 0) { match_fill_none(nQ, train_idx, best_dist, second_dist, n_matches); return VDO_OK; }
  const bool cross = prm->cross_check != 0;
  const MatchPlan f = match_plan(nQ, nT, prm->chunk_rows), r = match_plan(nT, nQ, prm->chunk_rows);
  rc = match_check_plan(who, nQ, nT, f, r, cross);
  if (rc != VDO_OK) return rc;
  rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  const bool use_pos = prm->window >= 0.f, use_oct = prm->max_octave_diff >= 0;
  size_t bytes = match_scratch_bytes(nQ, nT, f, r, cross) + 4096;
  for (const vdo_match_set* m : {query, train})
    if (!m->is_device) bytes += pad256(32 * (size_t)m->n) + (use_pos ? 2 * pad256(4 * (size_t)m->n) : 0) + (use_oct ? pad256(4 * (size_t)m->n) : 0);
  Arena A(ctx);
  if (!A.reserve(bytes)) return set_error(VDO_ERR_OOM, "%s: scratch arena: allocation failed, or an open object chain holds it", who);
  MatchSet dev[2];
  const vdo_match_set* in[2] = {query, train};
  for (int k = 0; k < 2; ++k) {
    const vdo_match_set* m = in[k];
    MatchSet& D = dev[k];
    D.n = m->n; D.x = D.y = nullptr; D.oct = nullptr;
    if (m->is_device) {
      D.desc = (const uint64_t*)m->desc;
      if (use_pos) { D.x = m->x; D.y = m->y; }
      if (use_oct) D.oct = m->octave;
    } else {
      D.desc = (const uint64_t*)A.up(m->desc, 32 * (size_t)m->n);
      if (use_pos) { D.x = A.up(m->x, m->n); D.y = A.up(m->y, m->n); }
      if (use_oct) D.oct = A.up(m->octave, m->n);
      if (!D.desc || (use_pos && (!D.x || !D.y)) || (use_oct && !D.oct)) return set_error(VDO_ERR_OOM, "%s: scratch arena exhausted", who);
    }
  }
  rc = match_launch(who, A, dev[0], dev[1], *prm, f, r, train_idx, best_dist, second_dist, n_matches);
  if (rc != VDO_OK) return rc;
  return A.finish(who);
}

extern "C" int vdo_orb_match_extractors(vdo_orb* query, vdo_orb* train, const vdo_match_params* prm, int32_t* train_idx, int32_t* best_dist,
                                        int32_t* second_dist, int32_t* n_matches, int32_t capacity) {
  static const char* who = "vdo_orb_match_extractors";
  if (!query) return set_error(VDO_ERR_INVALID, "%s: query is null", who);
  if (!train) return set_error(VDO_ERR_INVALID, "%s: train is null", who);
  int rc = match_check_params(who, prm);
  if (rc == VDO_OK) rc = match_check_outputs(who, train_idx, best_dist, second_dist, n_matches);
  if (rc != VDO_OK) return rc;
  // (one object on both sides is safe: its view is made resident once and the match only reads it)
  OrbMatchView vq, vt;
  rc = orb_match_view(query, &vq);
  if (rc != VDO_OK) return rc;
  if (vq.n > capacity) return set_error(VDO_ERR_INVALID, "%s: capacity %d smaller than the query extractor's %d keypoints", who, capacity, vq.n);
  rc = orb_match_view(train, &vt);
  if (rc != VDO_OK) return rc;
  if (vq.ctx->device != vt.ctx->device) return set_error(VDO_ERR_INVALID, "%s: query and train live on different devices (%d, %d)", who, vq.ctx->device, vt.ctx->device);
  const int nQ = vq.n, nT = vt.n;
  if (nQ == 0 || nT == 0) { match_fill_none(nQ, train_idx, best_dist, second_dist, n_matches); return VDO_OK; }
  const bool cross = prm->cross_check != 0;
  const MatchPlan f = match_plan(nQ, nT, prm->chunk_rows), r = match_plan(nT, nQ, prm->chunk_rows);
  rc = match_check_plan(who, nQ, nT, f, r, cross);
  if (rc != VDO_OK) return rc;
  vdo_ctx* ctx = vq.ctx;                       // the match runs on the query extractor's stream
  rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  Arena A(ctx);
  if (!A.reserve(match_scratch_bytes(nQ, nT, f, r, cross) + 4096)) return set_error(VDO_ERR_OOM, "%s: scratch arena: allocation failed, or an open object chain holds it", who);
  hipEvent_t ev = nullptr;
  if (vt.ctx->stream != ctx->stream) {         // the train extractor's view is produced on ITS stream: order the match behind it with an event
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return set_error(VDO_ERR_NO_DEVICE, "%s: hipEventCreate failed", who);
    hipEventRecord(ev, vt.ctx->stream);
    hipStreamWaitEvent(ctx->stream, ev, 0);
  }
  const MatchSet Q{nQ, (const uint64_t*)vq.desc, vq.x, vq.y, vq.octave}, T{nT, (const uint64_t*)vt.desc, vt.x, vt.y, vt.octave};
  rc = match_launch(who, A, Q, T, *prm, f, r, train_idx, best_dist, second_dist, n_matches);
  if (rc == VDO_OK) rc = A.finish(who);        // waits for the match, hence for everything it read: either extractor may extract again
  else hipStreamSynchronize(ctx->stream);
  if (ev) hipEventDestroy(ev);
  return rc;
}
