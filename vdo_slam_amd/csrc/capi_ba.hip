// C-ABI entry points (include/vdo_slam_hip.h) of the batch-BA path: upload of a graph in the layout its plan decides
// (ba_plan.hpp: the host-side re-ordering into tiles), linearisation, system download, estimates.
// The Levenberg–Marquardt driver is in ba_lm.hip.
#include <algorithm>
#include <cstdlib>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include <chrono>

#include "ba_host.hpp"
#include "ba_plan.hpp"

namespace vdo {
constexpr size_t kBaSlabBytes = (size_t)48 << 20;      // the context's slab for small batch handles (a 20-frame window of KITTI takes ~6 MB)

// device memory of a handle: from the context's slab while the handle owns the pool and the block fits, else hipMalloc (freed by vdo_ba_destroy)
void* ba_device_alloc(vdo_ba* ba, size_t bytes) {
  vdo_ctx* c = ba->ctx;
  const size_t need = (bytes + 255) & ~(size_t)255;
  if (ba->pooled && c->ba_slab && c->ba_slab_used + need <= c->ba_slab_cap) {
    void* p = c->ba_slab + c->ba_slab_used;
    c->ba_slab_used += need;
    return p;
  }
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
  ba->allocs.push_back(p);
  return p;
}
}  // namespace vdo

using namespace vdo;

namespace {

template <class T>
int upload(vdo_ba* ba, T** dst, const T* src, size_t n, hipStream_t s) {
  if (n == 0) { *dst = nullptr; return VDO_OK; }
  *dst = (T*)ba_device_alloc(ba, n * sizeof(T));
  if (!*dst) return set_error(VDO_ERR_OOM, "hipMalloc(%zu) failed", n * sizeof(T));
  if (src) {
    if (hipMemcpyAsync(*dst, src, n * sizeof(T), hipMemcpyHostToDevice, s) != hipSuccess) return set_error(VDO_ERR_NO_DEVICE, "H2D copy failed");
  } else {
    hipMemsetAsync(*dst, 0, n * sizeof(T), s);
  }
  return VDO_OK;
}

// the switches of the upload half, read once per call
struct UploadOptions {
  bool chain_global = false;    // VDO_BA_CHAIN_GLOBAL: the pose chains' strips in HBM, not in LDS
  bool pchain_closed = false;   // VDO_BA_PCHAIN_CLOSED: the closed-form block inverse in k_pchain_factor
  int chain_waves = 0;          // VDO_BA_CHAIN_WAVES: segments per pose chain (0: by the longest chain)
  static UploadOptions from_env() {
    UploadOptions o;
    o.chain_global = std::getenv("VDO_BA_CHAIN_GLOBAL") != nullptr;
    o.pchain_closed = std::getenv("VDO_BA_PCHAIN_CLOSED") != nullptr;
    if (const char* e = std::getenv("VDO_BA_CHAIN_WAVES")) o.chain_waves = std::min(16, std::max(1, std::atoi(e)));
    return o;
  }
};

// the plan's sizes, and what follows from them, as the kernels see them
BADev device_dims(const vdo_ba_graph& g, const BaPlan& plan, const UploadOptions& opt) {
  BADev d;
  d.P = plan.P; d.L = plan.L; d.Eb = plan.Ebp(); d.Et = plan.Et; d.Ep = plan.Ep; d.Npr = plan.Npr; d.Ninc = plan.Ebp() + 2 * plan.Et;
  d.n_tiles = plan.n_tiles(); d.NPS = plan.NPS; d.n_chains = plan.n_chains(); d.max_slots = plan.max_slots; d.n_dyn_tiles = plan.n_dyn_tiles;
  d.ps_stride = plan.ps_stride;
  d.n_hubs = plan.n_hubs(); d.n_hub_edges = plan.n_hub_edges();
  d.n_pchains = plan.n_pchains();
  // LDS strip of a pose chain's workgroup (ba_solve.hip pchain_solve_partitioned): [len][6] doubles, <= 144 KB
  d.pc_maxlen = plan.pc_maxlen;
  d.pc_lds = !opt.chain_global && 48 * (size_t)plan.pc_maxlen <= (size_t)(144 * 1024) ? 1 : 0;     // (up to 144 of the 160 KB of a CU: launch_pcg_* raise the kernels' dynamic-LDS limit)
  d.pc_closed = opt.pchain_closed ? 1 : 0;
  d.pc_nwave = opt.chain_waves ? opt.chain_waves : d.pc_lds ? std::min(16, std::max(1, (plan.pc_maxlen + 7) / 8)) : 1;      // segments of >= 8 positions, one wave each
  d.huber_eb = g.huber_eb; d.huber_et = g.huber_et; d.huber_ep = g.huber_ep;
  d.dsqr_eb = (double)(float)(g.huber_eb * g.huber_eb);   // float member, robust_kernel_impl.h:84
  d.dsqr_et = (double)(float)(g.huber_et * g.huber_et);
  d.dsqr_ep = (double)(float)(g.huber_ep * g.huber_ep);
  return d;
}

}  // namespace

#define UP(field, src, n)                                                          \
  do {                                                                             \
    int rc_ = upload(ba, &ba->d.field, src, (size_t)(n), s);                       \
    if (rc_ != VDO_OK) { vdo_ba_destroy(ba); return rc_; }                          \
  } while (0)

// validate the arguments, bind, plan (ba_plan.hip: every decision about the layout, on the host alone), check the plan against the tile kernels' LDS, take the
// context's pool, upload.  Every refusal returns before a handle exists, with the context untouched.
extern "C" int vdo_ba_create(vdo_ctx* ctx, const vdo_ba_graph* g, vdo_ba** out) {
  if (!ctx || !g || !out) return set_error(VDO_ERR_INVALID, "vdo_ba_create: null argument");
  if (g->n_pose <= 0 || g->n_point < 0 || g->n_eb < 0 || g->n_et < 0 || g->n_ep < 0 || g->n_prior < 0)
    return set_error(VDO_ERR_INVALID, "vdo_ba_create: negative/empty sizes");
  int rc = ctx_bind(ctx);
  if (rc != VDO_OK) return rc;
  const auto t_create0 = std::chrono::steady_clock::now();
  const BaPlanOptions plan_opt = BaPlanOptions::from_env();
  BaPlan plan;      // (alive until the uploads have been synchronised: they read its pageable memory)
  rc = plan_graph(*g, plan_opt, plan);
  if (rc != VDO_OK) return rc;
  const BADev dims = device_dims(*g, plan, UploadOptions::from_env());
  // Every tile kernel's workgroup holds the largest tile's pose slots in LDS (at 32 sums per partial row the sweep passes the 160 KB of a CU above 400 slots):
  // a graph whose tile kernels cannot be launched is refused here, with its sizes, and not at its first launch.  The same size helpers as the launch sites.
  const LdsNeed need = tile_lds_need(dims);
  if (need.bytes > (size_t)VDO_LDS_MAX_BYTES)
    return set_error(VDO_ERR_UNSUPPORTED, "a tile of %d pose slots with %d sums per partial row needs %zu bytes of LDS in %s, more than the %d bytes of a workgroup "
                     "(a landmark track touches too many pose vertices)", plan.max_slots, plan.ps_stride, need.bytes, need.kernel, (int)VDO_LDS_MAX_BYTES);
  const auto t_built = std::chrono::steady_clock::now();

  vdo_ba* ba = new vdo_ba();
  ba->ctx = ctx;
  ba->d = dims;
  ba->n_eb = plan.Eb;
  ba->compact_edges = plan.compact_edges;
  ba->pose_graph_is_paths = plan.pose_graph_is_paths;
  // (a tile of > ~200 pose slots: the dense assembly's workgroup no longer fits the LDS; PCG does - 76 KB at 256 slots)
  ba->dense_tiles_ok = plan.dense_tiles_ok && dense_tile_lds(dims) <= (size_t)VDO_LDS_MAX_BYTES;
  // a small graph takes the context's pool if nobody holds it; the slab itself is allocated on the first such graph.  Taken only here, once the graph has been
  // accepted (from here on vdo_ba_destroy gives it back)
  if (!ctx->ba_pool_busy && (int64_t)plan.L + plan.Eb + plan.Et < 200000) {
    if (!ctx->ba_slab && hipMalloc((void**)&ctx->ba_slab, kBaSlabBytes) == hipSuccess) ctx->ba_slab_cap = kBaSlabBytes;
    if (ctx->ba_slab) { ctx->ba_pool_busy = true; ctx->ba_slab_used = 0; ba->pooled = true; }
    else (void)hipGetLastError();
  }
  hipStream_t s = ctx->stream;
  BADev& d = ba->d;
  const int P = plan.P, L = plan.L, Et = plan.Et, Ep = plan.Ep, Npr = plan.Npr, Ebp = plan.Ebp();
  const int n_tiles = plan.n_tiles(), NPS = plan.NPS, n_pchains = plan.n_pchains(), n_hubs = plan.n_hubs(), n_hub_edges = plan.n_hub_edges();
  UP(pose[0], g->pose, 12 * (size_t)P); UP(pose[1], g->pose, 12 * (size_t)P);
  UP(point[0], plan.point.data(), 3 * (size_t)L); UP(point[1], plan.point.data(), 3 * (size_t)L);
  UP(tile_pose, plan.tile_pose.data(), plan.tile_pose.size());
  UP(tiles, plan.tiles_launch.data(), plan.tiles_launch.size());
  UP(chain_off, plan.chain_off.data(), plan.chain_off.size()); UP(pt_prev_edge, plan.pt_prev_edge.data(), L);
  UP(pt_single, plan.pt_single.data(), plan.pt_single.size());
  UP(eb_key, plan.eb_key.data(), plan.eb_key.size());
  UP(et_key, plan.et_key.data(), Et); UP(et_slot, plan.et_slot.data(), Et);
  // the edge inputs in the formats the plan found lossless (ba_dev.hpp)
  if (plan.compact_edges & 1) d.eb_w_uni = g->eb_w[0]; else UP(eb_w, plan.eb_w.data(), Ebp);
  if (plan.compact_edges & 4) d.et_w_uni = plan.et_w[0]; else UP(et_w, plan.et_w.data(), Et);
  if (plan.compact_edges & 2) UP(eb_zf, plan.eb_zf.data(), plan.eb_zf.size());
  else UP(eb_z, plan.eb_z.data(), 3 * (size_t)Ebp);
  if (!(plan.compact_edges & 8)) UP(et_z, plan.et_z.data(), 3 * (size_t)Et);
  UP(inc_key, plan.inc_key.data(), plan.inc_key.size());
  UP(ep_i, g->ep_i, Ep); UP(ep_j, g->ep_j, Ep); UP(ep_z, g->ep_z, 12 * (size_t)Ep); UP(ep_info, g->ep_info, 36 * (size_t)Ep);
  UP(pr_pose, g->pr_pose, Npr); UP(pr_z, g->pr_z, 12 * (size_t)Npr); UP(pr_info, g->pr_info, 36 * (size_t)Npr);
  UP(ps_off, plan.ps_off.data(), P + 1); UP(ps_idx, plan.ps_idx.data(), NPS);
  UP(slot_dst, plan.slot_dst.data(), plan.slot_dst.size()); UP(pose_kind, plan.pose_kind.data(), std::max(P, 1));
  if (n_hubs) {
    UP(hub_off, plan.hub_off.data(), plan.hub_off.size()); UP(hub_point, plan.hub_point.data(), plan.hub_point.size()); UP(hub_pose, plan.hub_pose.data(), plan.hub_pose.size());
    UP(hub_row, plan.hub_row.data(), (size_t)n_hub_edges); UP(hub_z, plan.hub_z.data(), 3 * (size_t)n_hub_edges); UP(hub_w, plan.hub_w.data(), (size_t)n_hub_edges);
    const double* Zh = nullptr;
    UP(hub_we, Zh, (size_t)n_hub_edges); UP(hub_chi, Zh, 2 * (size_t)n_hubs);
  }
  UP(pe_off, plan.pe_off.data(), P + 1); UP(pe_idx, plan.pe_idx.data(), plan.pe_idx.size());
  UP(pr_off, plan.pr_off.data(), P + 1); UP(pr_idx, plan.pr_idx.data(), plan.pr_idx.size());
  UP(pc_off, plan.pc_off.data(), plan.pc_off.size()); UP(pc_pose, plan.pc_pose.data(), P); UP(pc_edge, plan.pc_edge.data(), P);
  UP(pc_far_pos, plan.pc_far_pos.data(), plan.pc_far_pos.size()); UP(pc_far_edge, plan.pc_far_edge.data(), plan.pc_far_edge.size());
  const double* Z = nullptr;
  // ONE block: Hpp | bp | red_chi [4] | block-Jacobi sums msum [21 P] | failure flag | qs [6 P].  Sharded solves send Hpp .. red_chi[1] per linearisation, msum .. qs per trial -
  // and the whole block at once for the first trial of an LM iteration (launch_linearize(defer_exchange) + launch_factor_and_rhs(lin_pending): red_chi[2..3], the scale partial
  // of the last update, ride along; k_update rewrites them before they are read again)
  UP(Hpp, Z, 69 * (size_t)P + 6);
  ba->d.bp = ba->d.Hpp + 36 * (size_t)P; ba->d.red_chi = ba->d.bp + 6 * (size_t)P;
  ba->d.msum = ba->d.red_chi + 4;
  ba->d.qs = ba->d.msum + 21 * (size_t)P + 1;
  UP(Hll, Z, (size_t)L); UP(bl, Z, 3 * (size_t)L);
  UP(Finc, Z, std::max<size_t>((size_t)Ebp, VDO_TILE_THREADS) + (size_t)Et + 1); UP(Oll, Z, 9 * (size_t)Et); UP(Hpp_ep, Z, 36 * (size_t)Ep); UP(ep_blk, Z, 84 * (size_t)std::max(Ep + Npr, 1));
  UP(part_sums, Z, (size_t)plan.ps_stride * (size_t)std::max(NPS, 1));
  UP(part_chi, Z, 2 * (size_t)n_tiles + 2 * (size_t)(Ep + Npr) + 2);
  UP(part_red, Z, 256);
  UP(Dinv, Z, 9 * (size_t)L); UP(Gl, Z, 9 * (size_t)L); UP(Gdiag, Z, 9 * (size_t)L); UP(Goff, Z, 9 * (size_t)L);
  UP(xl, Z, 3 * (size_t)L); UP(dscal, Z, (size_t)std::max(L, 1));
  UP(Minv, Z, 36 * (size_t)P); UP(Lc, Z, 36 * (size_t)P); UP(Lfar, Z, 36 * (size_t)std::max(n_pchains, 1)); UP(Pf, Z, 36 * (size_t)P); UP(Qb, Z, 36 * (size_t)P); UP(Adg, Z, 36 * (size_t)P);
  UP(xp, Z, 6 * (size_t)P); UP(rp, Z, 6 * (size_t)P); UP(zp, Z, 6 * (size_t)P); UP(pp, Z, 6 * (size_t)P); UP(pp2, Z, 6 * (size_t)P);
  UP(qp, Z, 6 * (size_t)P); UP(bs, Z, 6 * (size_t)P);
  UP(part_pq, Z, (size_t)(P + 3) / 4 + 1); UP(part_rz, Z, (size_t)n_pchains + 1);
  UP(part_q, Z, 8 * (size_t)NPS + 8); UP(part_m, Z, 16 * (size_t)NPS + 16); UP(part_m8, Z, 8 * (size_t)NPS + 8);
  UP(scal, Z, S_COUNT);
  const int32_t* ZI = nullptr;
  UP(flags, ZI, 4);
  if (ba->pooled && ctx->ba_hscal) {                     // the pinned block, the side stream and the events of the last pooled handle
    ba->h_scal = ctx->ba_hscal; ba->d_hscal = ctx->ba_hscal_dev;
    ba->ev0 = ctx->ba_ev[0]; ba->ev1 = ctx->ba_ev[1]; ba->ev_fork = ctx->ba_ev[2]; ba->ev_join = ctx->ba_ev[3]; ba->side = ctx->ba_side;
  } else {
    void* dp = nullptr;
    if (hipHostMalloc((void**)&ba->h_scal, S_COUNT * sizeof(double) + 8 * sizeof(int32_t), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(&dp, ba->h_scal, 0) != hipSuccess || !dp) {
      vdo_ba_destroy(ba);
      return set_error(VDO_ERR_OOM, "hipHostMalloc failed");
    }
    ba->d_hscal = (double*)dp;
    hipEventCreate(&ba->ev0); hipEventCreate(&ba->ev1);
    if (hipStreamCreateWithFlags(&ba->side, hipStreamNonBlocking) == hipSuccess) {
      hipEventCreateWithFlags(&ba->ev_fork, hipEventDisableTiming); hipEventCreateWithFlags(&ba->ev_join, hipEventDisableTiming);
    } else ba->side = nullptr;
    if (ba->pooled) {                                    // first pooled handle of this context: they stay with the context from here on
      ctx->ba_hscal = ba->h_scal; ctx->ba_hscal_dev = ba->d_hscal;
      ctx->ba_ev[0] = ba->ev0; ctx->ba_ev[1] = ba->ev1; ctx->ba_ev[2] = ba->ev_fork; ctx->ba_ev[3] = ba->ev_join; ctx->ba_side = ba->side;
    }
  }
  std::memset(ba->h_scal, 0, S_COUNT * sizeof(double) + 8 * sizeof(int32_t));      // (scalars, flags, the read-back ticket: ba_lm.hip fetch)
  ba->ticket = 0;
  ba->h_flags = (int32_t*)(ba->h_scal + S_COUNT);
  if (hipStreamSynchronize(s) != hipSuccess) { vdo_ba_destroy(ba); return set_error(VDO_ERR_NO_DEVICE, "upload failed: %s", hipGetErrorString(hipGetLastError())); }
  if (plan_opt.trace)
    std::fprintf(stderr, "[vdo_ba_create] validated %.2f, chains %.2f, tiles %.2f (of which closing tiles %.2f), hubs %.2f, permuted data %.2f ms (cumulative); tiles built in %.2f ms, uploaded in %.2f ms (%s)\n", plan.t_mark[0], plan.t_mark[1], plan.t_mark[2], plan.t_close_ms, plan.t_mark[3], plan.t_mark[4], std::chrono::duration<double, std::milli>(t_built - t_create0).count(),
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_built).count(), ba->pooled ? "pooled" : "own allocations");
  // the uploads are done: what the handle keeps of the plan moves over
  ba->pt_old_of_new = std::move(plan.pt_old_of_new); ba->pt_new_of_old = std::move(plan.pt_new_of_old);
  ba->eb_old_of_new = std::move(plan.eb_old_of_new); ba->et_old_of_new = std::move(plan.et_old_of_new);
  ba->inc_of_eb = std::move(plan.inc_of_eb); ba->inc1_of_et = std::move(plan.inc1_of_et); ba->inc2_of_et = std::move(plan.inc2_of_et);
  ba->hub_eb_old = std::move(plan.hub_eb_old);
  *out = ba;
  return VDO_OK;
}

extern "C" int vdo_ba_destroy(vdo_ba* ba) {
  if (!ba) return VDO_OK;
  if (ba->ctx) ctx_bind(ba->ctx);
  if (ba->pooled) {
    // the slab, the pinned block, the side stream and the events go back to the context - once nothing in flight uses them (hipFree below waits by itself)
    if (ba->ctx->stream) hipStreamSynchronize(ba->ctx->stream);
    if (ba->side) hipStreamSynchronize(ba->side);
    ba->ctx->ba_slab_used = 0; ba->ctx->ba_pool_busy = false;
    const bool kept = ba->ctx->ba_hscal == ba->h_scal;       // (false: the handle failed before its pinned block was handed to the context)
    for (void* p : ba->allocs) hipFree(p);
    if (!kept) {
      if (ba->h_scal) hipHostFree(ba->h_scal);
      for (hipEvent_t e : {ba->ev0, ba->ev1, ba->ev_fork, ba->ev_join}) if (e) hipEventDestroy(e);
      if (ba->side) hipStreamDestroy(ba->side);
    }
    delete ba;
    return VDO_OK;
  }
  for (void* p : ba->allocs) hipFree(p);
  if (ba->h_scal) hipHostFree(ba->h_scal);      // (h_flags lives in the same block)
  if (ba->ev0) hipEventDestroy(ba->ev0);
  if (ba->ev1) hipEventDestroy(ba->ev1);
  if (ba->ev_fork) hipEventDestroy(ba->ev_fork);
  if (ba->ev_join) hipEventDestroy(ba->ev_join);
  if (ba->side) hipStreamDestroy(ba->side);
  delete ba;
  return VDO_OK;
}

extern "C" int vdo_ba_set_allreduce(vdo_ba* ba, vdo_allreduce_fn fn, void* user, int shard_rank) {
  if (!ba || shard_rank < 0) return set_error(VDO_ERR_INVALID, "vdo_ba_set_allreduce: bad argument");
  ba->red.fn = fn; ba->red.user = user; ba->red.err = 0;
  ba->d.sharded = fn ? 1 : 0;
  ba->d.shard_rank = fn ? shard_rank : 0;
  return VDO_OK;
}

extern "C" int vdo_ba_linearize(vdo_ba* ba, int repeat, float* ms_sweep) {
  if (!ba) return set_error(VDO_ERR_INVALID, "null handle");
  int rc = ctx_bind(ba->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = ba->ctx->stream;
  if (repeat < 1) repeat = 1;
  if (ms_sweep) {
    launch_sweep_only(ba->d, s);   // warm-up
    hipEventRecord(ba->ev0, s);
    for (int i = 0; i < repeat; ++i) launch_sweep_only(ba->d, s);
    hipEventRecord(ba->ev1, s);
    hipEventSynchronize(ba->ev1);
    float ms = 0;
    hipEventElapsedTime(&ms, ba->ev0, ba->ev1);
    *ms_sweep = ms / repeat;
  }
  for (int i = 0; i < (ms_sweep ? 1 : repeat); ++i) launch_linearize(ba->d, s, ba->red);
  ba->lin_current = true;
  return sync_check(ba, "vdo_ba_linearize");
}

extern "C" int vdo_ba_profile_linearize(vdo_ba* ba, int repeat, float ms[2], int64_t dims[8]) {
  if (!ba || !ms) return set_error(VDO_ERR_INVALID, "vdo_ba_profile_linearize: null argument");
  int rc = ctx_bind(ba->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = ba->ctx->stream;
  if (repeat < 1) repeat = 1;
  const BADev& d = ba->d;
  for (int which = 0; which < 2; ++which) {
    if (which == 0) launch_sweep_only(d, s); else launch_linearize(d, s, ba->red);          // warm-up
    hipEventRecord(ba->ev0, s);
    for (int i = 0; i < repeat; ++i) { if (which == 0) launch_sweep_only(d, s); else launch_linearize(d, s, ba->red); }
    hipEventRecord(ba->ev1, s);
    hipEventSynchronize(ba->ev1);
    float t = 0;
    hipEventElapsedTime(&t, ba->ev0, ba->ev1);
    ms[which] = t / repeat;
  }
  if (dims) {
    dims[0] = d.n_tiles; dims[1] = d.NPS; dims[2] = d.ps_stride; dims[3] = d.max_slots;
    dims[4] = 4 + (d.eb_zf ? 12 : 24) + (d.eb_w ? 8 : 0);
    dims[5] = 8 + (d.et_z ? 24 : 0) + (d.et_w ? 8 : 0);
    dims[6] = d.Eb; dims[7] = d.n_hubs;
  }
  ba->lin_current = true;
  return sync_check(ba, "vdo_ba_profile_linearize");
}

// Mean duration of the Schur mat-vec of one CG iteration (k_schur_tile<0>: part_q = B Hll^-1 B^T p over every tile) - the largest consumer of an LM
// iteration - timed alone with events on the context's stream.  Call after an optimisation (vdo_ba_optimize) of this handle: the landmark factors of its
// last trial and the direction of its last solve are what the launches read.  ms: mean milliseconds per launch.
extern "C" int vdo_ba_profile_schur(vdo_ba* ba, int repeat, float* ms) {
  if (!ba || !ms) return set_error(VDO_ERR_INVALID, "vdo_ba_profile_schur: null argument");
  int rc = ctx_bind(ba->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = ba->ctx->stream;
  if (repeat < 1) repeat = 1;
  const BADev& d = ba->d;
  if (!d.n_tiles) { *ms = 0.f; return VDO_OK; }
  hipMemsetAsync(d.flags, 0, 4 * sizeof(int32_t), s);          // (flags[1] = "PCG converged" turns the queued mat-vecs into no-ops)
  launch_schur_matvec_only(d, s);                              // warm-up
  hipEventRecord(ba->ev0, s);
  for (int i = 0; i < repeat; ++i) launch_schur_matvec_only(d, s);
  hipEventRecord(ba->ev1, s);
  hipEventSynchronize(ba->ev1);
  float t = 0;
  hipEventElapsedTime(&t, ba->ev0, ba->ev1);
  *ms = t / repeat;
  return sync_check(ba, "vdo_ba_profile_schur");
}

extern "C" int vdo_ba_download_system(vdo_ba* ba, vdo_ba_system* out) {
  if (!ba || !out) return set_error(VDO_ERR_INVALID, "null argument");
  int rc = ctx_bind(ba->ctx);
  if (rc != VDO_OK) return rc;
  const BADev& d = ba->d;
  hipStream_t s = ba->ctx->stream;
  auto D2H = [&](void* dst, const void* src, size_t bytes) { if (dst && bytes) hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s); };
  // The pose-landmark blocks are kept factored (one scalar per incidence) and expanded with the CURRENT estimate; after an optimisation or
  // vdo_ba_set_estimates the stored Hpp / bp / Hll / Finc belong to an older estimate and the expansion would mix the two: re-linearise
  // first, so that what comes back is always one self-consistent system at the current estimate.
  if (!ba->lin_current) { launch_linearize(ba->d, s, ba->red); ba->lin_current = true; }
  std::vector<double> hll, bl, oll, binc, hub_binc;
  D2H(out->Hpp, d.Hpp, sizeof(double) * 36 * (size_t)d.P);
  D2H(out->bp, d.bp, sizeof(double) * 6 * (size_t)d.P);
  D2H(out->Hpp_ep, d.Hpp_ep, sizeof(double) * 36 * (size_t)d.Ep);
  if (out->Hll) { hll.resize((size_t)d.L); D2H(hll.data(), d.Hll, sizeof(double) * hll.size()); }      // device: one scalar per point (block = s * I3)
  if (out->bl) { bl.resize(3 * (size_t)d.L); D2H(bl.data(), d.bl, sizeof(double) * bl.size()); }
  if (out->Hll_et) { oll.resize(9 * (size_t)d.Et); D2H(oll.data(), d.Oll, sizeof(double) * oll.size()); }
  if (out->Hpl_eb || out->Hlp1_et || out->Hlp2_et) {
    // the solve path keeps the blocks factored (Finc); materialise the explicit 6x3 blocks on demand
    if (!ba->d.Binc && d.Ninc) {
      if (hipMalloc((void**)&ba->d.Binc, sizeof(double) * 18 * (size_t)d.Ninc) != hipSuccess) return set_error(VDO_ERR_OOM, "hipMalloc(Binc) failed");
      ba->allocs.push_back((void*)ba->d.Binc);
    }
    launch_expand_binc(ba->d, s);
    if (d.n_hub_edges && out->Hpl_eb) {                    // the hub landmarks' edges (ba_hub.hip)
      if (!ba->hub_binc) ba->hub_binc = (double*)ba_device_alloc(ba, sizeof(double) * 18 * (size_t)d.n_hub_edges);      // (kept with the handle, like Binc)
      double* hb = ba->hub_binc;
      if (!hb) return set_error(VDO_ERR_OOM, "hipMalloc(hub blocks) failed");
      launch_hub_expand_binc(ba->d, hb, s);
      hub_binc.resize(18 * (size_t)d.n_hub_edges);
      D2H(hub_binc.data(), hb, sizeof(double) * hub_binc.size());
    }
    binc.resize(18 * (size_t)d.Ninc);
    D2H(binc.data(), ba->d.Binc, sizeof(double) * binc.size());
  }
  D2H(ba->h_scal, d.scal, sizeof(double) * S_COUNT);
  rc = sync_check(ba, "vdo_ba_download_system");
  if (rc != VDO_OK) return rc;
  const size_t N = d.Ninc, Ebp = d.Eb, Eb = (size_t)ba->n_eb, Et = d.Et;      // (Ebp: padded edge entries of the device, Eb: edges of the graph)
  if (out->Hll) for (int l = 0; l < d.L; ++l) { double* o = out->Hll + 9 * (size_t)ba->pt_old_of_new[l]; for (int i = 0; i < 9; ++i) o[i] = (i % 4 == 0) ? hll[(size_t)l] : 0.0; }
  if (out->bl) for (int l = 0; l < d.L; ++l) std::memcpy(out->bl + 3 * (size_t)ba->pt_old_of_new[l], bl.data() + 3 * (size_t)l, 24);
  if (out->Hll_et)
    for (size_t e = 0; e < Et; ++e) for (int i = 0; i < 9; ++i) out->Hll_et[i * Et + ba->et_old_of_new[e]] = oll[9 * e + i];
  if (out->Hpl_eb) {
    for (size_t e = 0; e < Ebp; ++e) { if (ba->eb_old_of_new[e] < 0) continue; for (int i = 0; i < 18; ++i) out->Hpl_eb[i * Eb + ba->eb_old_of_new[e]] = binc[i * N + ba->inc_of_eb[e]]; }
    for (size_t e = 0; e < ba->hub_eb_old.size(); ++e) for (int i = 0; i < 18; ++i) out->Hpl_eb[i * Eb + ba->hub_eb_old[e]] = hub_binc[18 * e + i];      // (hub landmarks, ba_hub.hip)
  }
  for (int rep = 0; rep < 2; ++rep) {
    double* dst = rep == 0 ? out->Hlp1_et : out->Hlp2_et;
    if (!dst) continue;
    const std::vector<int32_t>& inc = rep == 0 ? ba->inc1_of_et : ba->inc2_of_et;
    for (size_t e = 0; e < Et; ++e)
      for (int r = 0; r < 3; ++r)          // dst: 3x6 (point x pose) = transpose of the stored 6x3
        for (int c = 0; c < 6; ++c) dst[(size_t)(r * 6 + c) * Et + ba->et_old_of_new[e]] = binc[(size_t)(c * 3 + r) * N + inc[e]];
  }
  out->chi2 = ba->h_scal[S_CHI2];
  out->robust_chi2 = ba->h_scal[S_RCHI2];
  return VDO_OK;
}

extern "C" int vdo_ba_get_estimates(vdo_ba* ba, double* pose_out, double* point_out) {
  if (!ba) return set_error(VDO_ERR_INVALID, "null handle");
  int rc = ctx_bind(ba->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = ba->ctx->stream;
  if (pose_out) hipMemcpyAsync(pose_out, ba->d.pose[0], sizeof(double) * 12 * (size_t)ba->d.P, hipMemcpyDeviceToHost, s);
  if (point_out && ba->d.L) {
    ba->h_tmp.resize(3 * (size_t)ba->d.L);
    hipMemcpyAsync(ba->h_tmp.data(), ba->d.point[0], sizeof(double) * 3 * (size_t)ba->d.L, hipMemcpyDeviceToHost, s);
  }
  rc = sync_check(ba, "vdo_ba_get_estimates");
  if (rc != VDO_OK) return rc;
  if (point_out)
    for (int l = 0; l < ba->d.L; ++l) std::memcpy(point_out + 3 * (size_t)ba->pt_old_of_new[l], ba->h_tmp.data() + 3 * (size_t)l, 24);
  return VDO_OK;
}

extern "C" int vdo_ba_set_estimates(vdo_ba* ba, const double* pose, const double* point) {
  if (!ba) return set_error(VDO_ERR_INVALID, "null handle");
  ba->lin_current = false;
  int rc = ctx_bind(ba->ctx);
  if (rc != VDO_OK) return rc;
  hipStream_t s = ba->ctx->stream;
  if (pose) hipMemcpyAsync(ba->d.pose[0], pose, sizeof(double) * 12 * (size_t)ba->d.P, hipMemcpyHostToDevice, s);
  if (point && ba->d.L) {
    ba->h_tmp.resize(3 * (size_t)ba->d.L);
    for (int l = 0; l < ba->d.L; ++l) std::memcpy(ba->h_tmp.data() + 3 * (size_t)l, point + 3 * (size_t)ba->pt_old_of_new[l], 24);
    hipMemcpyAsync(ba->d.point[0], ba->h_tmp.data(), sizeof(double) * 3 * (size_t)ba->d.L, hipMemcpyHostToDevice, s);
  }
  ba->oplus_calls = 0;
  return sync_check(ba, "vdo_ba_set_estimates");
}
