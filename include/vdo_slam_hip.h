/* vdo_slam_hip.h — C-ABI of libvdo_hip.so: the MI355X (gfx950) hot path of VDO-SLAM.
 *
 * The reference (halajun/VDO_SLAM) has no FFI/plugin boundary: its hot path sits behind
 * C++ class signatures in libObjSLAM.so.  This header is the one boundary
 * the new build introduces: host C++ that keeps the reference's class API
 * (vdo_slam_amd/host/: ORBextractor, Frame, Tracking, Optimizer, System) calls these
 * entry points; nothing else does.  Conventions:
 *   - every function returns int: 0 = ok, <0 = vdo_status error; never throws, never aborts
 *     (vdo_last_error() gives a thread-local message);
 *   - plain pointers + explicit sizes, no C++/torch types;
 *   - all device work is stream-ordered on the context's hipStream_t (which may be an
 *     externally owned stream, e.g. torch's current stream), so callers can bracket calls
 *     with their own events;
 *   - fp64 for everything the reference computes in g2o (number_t = double,
 *     dependencies/g2o/config.h:14-29), fp32/u8/i32 for image-side data (cv::Mat types).
 * There is no CPU fallback: without a HIP device every compute entry point returns
 * VDO_ERR_NO_DEVICE.
 */
#ifndef VDO_SLAM_HIP_H_
#define VDO_SLAM_HIP_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vdo_status {
  VDO_OK = 0,
  VDO_ERR_INVALID = -1,     /* bad argument / malformed graph                         */
  VDO_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime failure                    */
  VDO_ERR_OOM = -3,
  VDO_ERR_UNSUPPORTED = -4, /* structurally valid input outside the supported envelope */
  VDO_ERR_INTERNAL = -5
} vdo_status;

int vdo_version(void);               /* 100*major + minor */
const char* vdo_last_error(void);    /* thread-local, never NULL */

/* ---- context ---------------------------------------------------------------------------*/
typedef struct vdo_ctx vdo_ctx;
/* stream == NULL: the context creates (and owns) a non-blocking stream on `device`. */
int vdo_ctx_create(int device, void* hip_stream, vdo_ctx** out);
int vdo_ctx_destroy(vdo_ctx* ctx);
int vdo_ctx_synchronize(vdo_ctx* ctx);
int vdo_ctx_stream(vdo_ctx* ctx, void** hip_stream_out);   /* the hipStream_t all calls are ordered on */
/* Context with an owned stream restricted to the compute units [cu_first, cu_first+cu_count) (invert != 0:
 * to every CU except those).  The per-frame LM kernels are one latency-bound workgroup per problem: giving
 * them CUs of their own keeps the image kernels of the same frame (which run concurrently) off their SIMDs. */
int vdo_ctx_create_cu_mask(int device, int cu_first, int cu_count, int invert, vdo_ctx** out);

/* ---- batch dynamic bundle adjustment ------------------------------------------------------
 * Replaces the g2o calls inside Optimizer::FullBatchOptimization (reference
 * src/Optimizer.cc:1232-2175: graph at :1355-1766, optimize(300) at :1935) and
 * Optimizer::PartialBatchOptimization (:42-1230, optimize(100) at :807): i.e.
 * SparseOptimizer::initializeOptimization/optimize (g2o/core/sparse_optimizer.cpp:205-267,
 * 354-443), OptimizationAlgorithmLevenberg::solve (g2o/core/optimization_algorithm_levenberg.cpp:61-164),
 * BlockSolver::buildSystem (g2o/core/block_solver.hpp:502-560) and the linear solve
 * (g2o/solvers/linear_solver_csparse.h:108-144).
 *
 * Graph in SoA form.  Poses = g2o::VertexSE3 estimates (Isometry3) as 12 doubles:
 * R row-major (9) then t (3).  For bandwidth the binary edges should be sorted by eb_pose
 * and the ternary edges by et_pose (the reference inserts them frame by frame, which already
 * is camera-major); correctness does not depend on the order.
 * Structural requirement (checked): a point is p1 of at most one and p2 of at most one
 * ternary edge (dynamic tracks are chains, src/Optimizer.cc:1704-1741). */
typedef struct vdo_ba_graph {
  int32_t n_pose, n_point, n_eb, n_et, n_ep, n_prior;
  const double* pose;      /* [n_pose][12]  cameras (T_wc) and object motions (H)        */
  const double* point;     /* [n_point][3]  VertexPointXYZ (world)                       */
  /* EdgeSE3PointXYZ (g2o/types/edge_se3_pointxyz.cpp:99-140), information = w * I3 */
  const int32_t* eb_pose;  /* [n_eb] */
  const int32_t* eb_point; /* [n_eb] */
  const double* eb_z;      /* [3][n_eb] SoA: measured point in the camera frame           */
  const double* eb_w;      /* [n_eb] */
  /* LandmarkMotionTernaryEdge (g2o/types/types_dyn_slam3d.cpp:53-85), information = w * I3 */
  const int32_t* et_p1;    /* [n_et] point at frame k-1 */
  const int32_t* et_p2;    /* [n_et] point at frame k   */
  const int32_t* et_pose;  /* [n_et] motion vertex H    */
  const double* et_z;      /* [3][n_et] SoA measurement (zero in the reference)           */
  const double* et_w;      /* [n_et] */
  /* EdgeSE3 (g2o/types/edge_se3.cpp:77-104): odometry + motion smoothness */
  const int32_t* ep_i;     /* [n_ep] */
  const int32_t* ep_j;     /* [n_ep] */
  const double* ep_z;      /* [n_ep][12] measurement */
  const double* ep_info;   /* [n_ep][36] information, row-major */
  /* EdgeSE3Prior (g2o/types/edge_se3_prior.cpp:89-102), ParameterSE3Offset = identity */
  const int32_t* pr_pose;  /* [n_prior] */
  const double* pr_z;      /* [n_prior][12] */
  const double* pr_info;   /* [n_prior][36] */
  /* RobustKernelHuber delta per edge class (<=0: none); the prior has no kernel
   * (src/Optimizer.cc:1364-1373).  NB the reference keeps delta^2 in a float
   * (g2o/core/robust_kernel_impl.h:84); reproduced. */
  double huber_eb, huber_et, huber_ep;
} vdo_ba_graph;

/* One linearisation in block form (what BlockSolver::buildSystem leaves in Hpp/Hpl/Hll/b).
 * Host arrays, caller-allocated; NULL pointers are skipped. */
typedef struct vdo_ba_system {
  double* Hpp;     /* [n_pose][36]  diagonal blocks, row-major                           */
  double* bp;      /* [n_pose][6]                                                       */
  double* Hll;     /* [n_point][9]                                                      */
  double* bl;      /* [n_point][3]                                                      */
  double* Hpl_eb;  /* [18][n_eb] SoA 6x3 block (pose x point) of each binary edge (index r*3+c) */
  double* Hll_et;  /* [9][n_et]  SoA 3x3 block p1 x p2                                    */
  double* Hlp1_et; /* [18][n_et] SoA 3x6 block p1 x pose                                  */
  double* Hlp2_et; /* [18][n_et] SoA 3x6 block p2 x pose                                  */
  double* Hpp_ep;  /* [n_ep][36] 6x6 block pose_i x pose_j                                */
  double chi2;        /* activeChi2 */
  double robust_chi2; /* activeRobustChi2 (g2o/core/sparse_optimizer.cpp:102-114) */
} vdo_ba_system;

typedef struct vdo_lm_options {
  int32_t max_iterations;     /* SparseOptimizer::optimize(n): 300 full batch, 100 partial */
  double gain_threshold;      /* SparseOptimizerTerminateAction::setGainThreshold; <0 = not installed */
  int32_t verbose;
  int32_t solver;             /* 2: Schur complement solved matrix-free by PCG with the pose-chain preconditioner;
                               * 3: Schur complement assembled densely and factorised by a blocked Cholesky on the fp64 MFMA
                               *    units (6 n_pose <= 8192) - what g2o's LinearSolverDense / CSparse do on the reduced system;
                               * 0: auto = 3 when the EdgeSE3 graph is not a set of simple paths (loop closures, branches) or a
                               *    PCG solve needed more than 60 iterations, else 2                                      */
  double pcg_tolerance;       /* relative residual ||r||_M / ||b||_M; <=0 -> 1e-8 (1e-10 until round 6; g2o's own PCG: 1e-6) */
  int32_t pcg_max_iterations; /* <=0 -> 24 n_pose + 200, capped at 20000                   */
} vdo_lm_options;

#define VDO_LM_MAX_TRACE 512
typedef struct vdo_lm_stats {
  int32_t iterations;          /* outer iterations executed (return value of optimize())   */
  int32_t total_trials;        /* levenberg trials summed over iterations                  */
  int32_t stop_reason;         /* 0 max_iter, 1 LM terminate, 2 chi2 increase, 3 gain action, 4 fail */
  double initial_chi2, final_chi2, final_lambda;
  double chi2_trace[VDO_LM_MAX_TRACE];
  int32_t trials_trace[VDO_LM_MAX_TRACE];
  double ms_total, ms_linearize, ms_solve;
} vdo_lm_stats;

typedef struct vdo_ba vdo_ba;
/* Uploads the graph to HBM (SoA, resident until destroy) and builds the chain structure.
 * Limits (g2o has none; VDO_ERR_UNSUPPORTED names the offending track): a DYNAMIC landmark track - a chain of points linked by
 * LandmarkMotionTernaryEdges - is processed by ONE workgroup and must fit its tile: <= 256 points, <= 1536 edge incidences, <= 512 distinct
 * pose vertices (cameras + motions), and sum over those poses of ceil(observations / 6) <= 256: it may run over up to 256 frames (its
 * points bring a camera and a motion vertex each; 128 until round 6).  A STATIC point has no such limit since round 6: up to 256 pose vertices it lives in a tile
 * (a graph that holds such a track pays with fewer resident workgroups per CU - the tile kernels' LDS grows with the pose slots of the
 * largest tile - and has no dense solver beyond ~200 slots); beyond them it becomes a hub landmark with a workgroup of its own
 * (csrc/ba_hub.hip; such graphs are solved by the PCG, the dense solver refuses them). */
int vdo_ba_create(vdo_ctx* ctx, const vdo_ba_graph* g, vdo_ba** out);
int vdo_ba_destroy(vdo_ba* ba);
/* K18: `repeat` back-to-back linearisation sweeps (errors + Jacobians + Huber + block
 * accumulation) at the current estimate.  If ms_sweep != NULL it receives the mean
 * duration of ONE binary-edge sweep kernel measured with hipEvents on the ctx stream. */
int vdo_ba_linearize(vdo_ba* ba, int repeat, float* ms_sweep);
/* Measurement hook of the roofline leg (bench.py, tools/sweep_only.py; no counterpart in the reference - its g2o prints one
 * time per outer iteration, g2o/core/sparse_optimizer.cpp:406-418): `repeat` back-to-back runs, hipEvents on the ctx stream, of
 *   ms[0] the tile sweep kernel alone (k_sweep_tile<true, .>),
 *   ms[1] a whole linearisation as BlockSolver::buildSystem means it (g2o/core/block_solver.hpp:502-560): sweep + expansion of
 *         the pose blocks (k_finalize_pose) + pose-pose edges (k_posepose) + chi2 reduction,
 * and the layout figures the byte model of DESIGN.md 4.1 needs:
 *   dims[0] tiles, [1] (tile, pose-slot) pairs, [2] running sums per partial row (16 / 32), [3] max slots of a tile,
 *   [4] bytes read per EdgeSE3PointXYZ entry (key + measurement [+ weight]), [5] bytes read per ternary edge,
 *   [6] EdgeSE3PointXYZ ENTRIES of the tiles' edge blocks (>= the graph's edges: every tile holds its edges as a padded block of
 *       256 x (edges per thread) entries, thread-transposed, so that every load of a tile kernel is one contiguous row), [7] hub landmarks (static points whose observations do not fit a tile: a workgroup of its own each). */
int vdo_ba_profile_linearize(vdo_ba* ba, int repeat, float ms[2], int64_t dims[8]);
/* new (measurement): mean milliseconds of ONE Schur mat-vec launch (k_schur_tile<0>, the product B Hll^-1 B^T p of a CG iteration of the reduced-camera solve that
   replaces g2o's BlockSolver::solve / LinearSolverCSparse, g2o/core/block_solver.hpp:143-295), timed alone with events on the context's stream.  Call after vdo_ba_optimize. */
int vdo_ba_profile_schur(vdo_ba* ba, int repeat, float* ms);
/* One self-consistent linearisation in block form (BlockSolver::buildSystem) AT THE CURRENT ESTIMATE: the blocks of the last
 * vdo_ba_linearize when nothing moved the estimate since, else (after vdo_ba_optimize / vdo_ba_set_estimates) a fresh linearisation is
 * run first - collective on a sharded handle. */
int vdo_ba_download_system(vdo_ba* ba, vdo_ba_system* out);
/* Full Levenberg–Marquardt (control flow identical to the modified g2o). */
int vdo_ba_optimize(vdo_ba* ba, const vdo_lm_options* opt, vdo_lm_stats* stats);
int vdo_ba_get_estimates(vdo_ba* ba, double* pose_out /*[n_pose][12]*/, double* point_out /*[n_point][3]*/);
int vdo_ba_set_estimates(vdo_ba* ba, const double* pose, const double* point);
/* Multi-GPU (landmark-track shards).  One process per GPU; every rank creates its
 * vdo_ba from a SHARD graph: all pose vertices, all pose-pose edges and priors (replicated), and
 * the points it owns with every binary/ternary edge incident to them (vdo_ba_partition assigns
 * whole tracks to ranks).  `fn` must reduce `count` doubles in place at the DEVICE pointer `buf`
 * across ranks, stream-ordered on the ctx stream (op 0 = sum, 1 = max; e.g. torch.distributed
 * all_reduce over RCCL).  Exchanges: Hpp|bp|chi2 (42P+2 doubles) once per linearisation, the
 * block-Jacobi diagonal (21P+1) once per Levenberg trial, 6P doubles per PCG iteration, 3 scalars per
 * trial.  Every rank returns the same poses; points come back for the owned shard only. */
typedef int (*vdo_allreduce_fn)(void* user, void* device_buf, int64_t count, int op);
int vdo_ba_set_allreduce(vdo_ba* ba, vdo_allreduce_fn fn, void* user, int shard_rank);
/* The same exchanges issued by the library itself over RCCL (xGMI inside a node): ncclAllReduce in place on the solver's
 * device buffers, on the context's stream - no host callback in the loop.  Rank 0 draws a 128-byte id
 * (ncclGetUniqueId) which the host hands to every rank over any side channel; every rank then creates its communicator on the
 * context its vdo_ba uses and attaches it.  vdo_rccl_comm_stats: all-reduces issued so far and their payload bytes. */
typedef struct vdo_rccl_comm vdo_rccl_comm;
int vdo_rccl_unique_id(char id_out[128]);
int vdo_rccl_comm_create(vdo_ctx* ctx, const char id[128], int n_ranks, int rank, vdo_rccl_comm** out);
int vdo_rccl_comm_destroy(vdo_rccl_comm* comm);
int vdo_rccl_comm_stats(const vdo_rccl_comm* comm, int64_t* calls, int64_t* bytes);
int vdo_rccl_allreduce(vdo_rccl_comm* comm, double* device_buf, int64_t count, int op /* 0 sum, 1 max */);
int vdo_ba_set_rccl(vdo_ba* ba, vdo_rccl_comm* comm /* NULL: back to single GPU */);
/* Host-only (no GPU needed): owner rank of every point so that tracks (points linked by ternary
 * edges) stay together, shards are contiguous in first-observing-frame order and balanced by
 * incidence count. */
int vdo_ba_partition(const vdo_ba_graph* g, int world, int32_t* owner_of_point /*[n_point]*/);
/* Host-only (no GPU, no context): the device layout vdo_ba_create decides for `g` - tiles, permutations, CSR tables, pose chains - or its refusal, for
 * tests of the layout (csrc/ba_plan.hpp).  vdo_ba_plan_array hands out one array of the plan by its field name, read-only and valid until the plan is
 * destroyed (an unknown name is VDO_ERR_INVALID); "tiles" / "tiles_launch" are the descriptors as 12 int32 each; "dims" is int64 [13]: tiles,
 * (tile, pose-slot) pairs, max slots of a tile, sums per partial row, hubs, hub edges, entries of the padded edge blocks, dynamic tiles, pose chains,
 * longest pose chain, pose graph is paths, dense assembly possible (incidences), compact edge formats (bits). */
typedef struct vdo_ba_plan vdo_ba_plan;
int vdo_ba_plan_create(const vdo_ba_graph* g, vdo_ba_plan** out);
int vdo_ba_plan_array(const vdo_ba_plan* p, const char* name, const void** data, int64_t* count, int32_t* elem_bytes);
int vdo_ba_plan_destroy(vdo_ba_plan* p);

/* ---- per-frame joint pose + optical-flow optimisation ------------------------------------------
 * Replaces the g2o calls inside Optimizer::PoseOptimizationFlow2Cam (reference
 * src/Optimizer.cc:2333-2542; camera, called from Tracking::Track src/Tracking.cc:697) and
 * Optimizer::PoseOptimizationFlow2 (:2755-2972; one call per object, src/Tracking.cc:932):
 * graph of 1 VertexSE3Expmap + N marginalised VertexSBAFlow, N EdgeSE3ProjectFlow2 (Huber) +
 * N EdgeFlowPrior, BlockSolver_6_3 + LinearSolverDense, optimize(100|200), chi2 gating.
 * The whole LM loop of a problem runs in one persistent workgroup; a batch (e.g. all objects
 * of a frame) is one kernel launch.  All pointers are HOST pointers; values are the
 * float->double conversions the reference performs in Converter (src/Converter.cc:25-35). */
typedef struct vdo_flow2_problem {
  int32_t n;              /* correspondences (TemperalMatch.size() / ObjId.size())          */
  const double* obs;      /* [n][2] last-frame pixel (kpUn.pt)                             */
  const double* flow;     /* [n][2] measured optical flow (initial estimate and prior)     */
  const double* depth;    /* [n]    depth of the last-frame pixel                          */
  double K[4];            /* fx, fy, cx, cy                                                */
  double Twl[16];         /* 4x4 row-major: last-frame camera-to-world                     */
  double T0[16];          /* 4x4 row-major initial estimate (mTcw / mInitModel)            */
  double info_flow;       /* 0.1  (Optimizer.cc:2405,2827)                                 */
  double info_prior;      /* 0.3 camera (:2440) / 0.5 object (:2863)                       */
  double huber_delta;     /* (double)sqrtf(0.04f) (:2371,2793)                             */
  double chi2_gate;       /* 0.04f (:2335,2757)                                            */
  int32_t max_iterations; /* 100 camera (:2455) / 200 object (:2878)                       */
  int32_t ref_quirks;     /* 1 = reproduce the BlockSolver_6_3 / 2-DoF aliasing;
                             0 = mathematically intended 2x2 Schur step (not parity-comparable) */
} vdo_flow2_problem;

typedef struct vdo_flow2_result {
  double T[16];           /* refined pose, 4x4 row-major (SE3Quat::to_homogeneous_matrix)  */
  int32_t n_inliers;      /* nInitialCorrespondences - nBad                                */
  int32_t iterations, trials, stop_reason;
  double initial_chi2, final_chi2, final_lambda;
} vdo_flow2_result;

typedef struct vdo_flow2_batch vdo_flow2_batch;
/* Upload n_problems problems (inputs become HBM-resident). */
int vdo_flow2_batch_create(vdo_ctx* ctx, int n_problems, const vdo_flow2_problem* probs, vdo_flow2_batch** out);
/* Per-frame use: slots of fixed capacity that are (re)defined every frame without re-allocating —
 * vdo_flow2_batch_reserve once, then per frame vdo_flow2_batch_set (inputs staged through pinned memory,
 * stream-ordered, no sync; problem == NULL empties a slot) -> run -> fetch. */
int vdo_flow2_batch_reserve(vdo_ctx* ctx, int n_problems, const int32_t* capacity, vdo_flow2_batch** out);
int vdo_flow2_batch_set(vdo_flow2_batch* batch, int k, const vdo_flow2_problem* problem);
/* Rewrites the initial pose (4x4 row-major) of a slot vdo_flow2_batch_set has filled - for a caller that packs the correspondences before it knows the pose.
 * The next run starts from it, exactly as if the slot had been set with that pose. */
int vdo_flow2_batch_set_T0(vdo_flow2_batch* batch, int k, const double T0[16]);
/* One kernel launch: every problem is optimised from its initial estimate (stream-ordered, no sync). */
int vdo_flow2_batch_run(vdo_flow2_batch* batch);
/* results[n_problems]; flow_out[k] -> [n_k][2] refined flows; inlier_out[k] -> [n_k] (1 = inlier). Synchronises. */
int vdo_flow2_batch_fetch(vdo_flow2_batch* batch, vdo_flow2_result* results, double** flow_out, uint8_t** inlier_out);
int vdo_flow2_batch_destroy(vdo_flow2_batch* batch);
/* Convenience: create + run + fetch + destroy for a single problem. */
int vdo_flow2_optimize(vdo_ctx* ctx, const vdo_flow2_problem* p, vdo_flow2_result* result, double* flow_out, uint8_t* inlier_out);

/* ---- non-joint per-frame pose refinement (bJoint == false) -----------------------------------------
 * Replaces the g2o calls inside Optimizer::PoseOptimizationNew (reference src/Optimizer.cc:2177-2331;
 * camera, called from src/Tracking.cc:699) and Optimizer::PoseOptimizationObjMot (:2544-2753; per
 * object, src/Tracking.cc:936): 1 VertexSE3Expmap + n unary reprojection edges with information I2
 * (EdgeSE3ProjectXYZOnlyPose with Huber sqrt(0.01) / EdgeSE3ProjectXYZOnlyObjMotion without kernel),
 * BlockSolver_6_3 + LinearSolverDense, optimize(100 / 200), one classification round at chi2 > 0.01f.
 * Results use vdo_flow2_result. */
typedef struct vdo_pose_problem {
  int32_t n;              /* correspondences                                               */
  int32_t kind;           /* 0 EdgeSE3ProjectXYZOnlyPose (K) ; 1 EdgeSE3ProjectXYZOnlyObjMotion (P) */
  const double* obs;      /* [n][2] current-frame pixel (kpUn.pt)                          */
  const double* Xw;       /* [n][3] back-projected last-frame point (float -> double)      */
  double K[4];            /* fx, fy, cx, cy (kind 0)                                       */
  double P[12];           /* 3x4 row-major K*Tcw (kind 1, Optimizer.cc:2604-2606)          */
  double T0[16];          /* initial estimate: mTcw (kind 0) / Tcw^-1 * mInitModel (kind 1) */
  double huber_delta;     /* (double)sqrtf(0.01f) kind 0 (:2213) ; <= 0: no kernel (kind 1) */
  double chi2_gate;       /* 0.01f (:2181, :2546)                                          */
  int32_t max_iterations; /* 100 (:2269) / 200 (:2664)                                     */
  int32_t pad;
} vdo_pose_problem;

typedef struct vdo_pose_batch vdo_pose_batch;
int vdo_pose_batch_create(vdo_ctx* ctx, int n_problems, const vdo_pose_problem* probs, vdo_pose_batch** out);
int vdo_pose_batch_run(vdo_pose_batch* batch);       /* one kernel launch, stream-ordered, no sync */
int vdo_pose_batch_fetch(vdo_pose_batch* batch, vdo_flow2_result* results, uint8_t** inlier_out);
int vdo_pose_batch_destroy(vdo_pose_batch* batch);
int vdo_pose_optimize(vdo_ctx* ctx, const vdo_pose_problem* p, vdo_flow2_result* result, uint8_t* inlier_out);

/* ---- RANSAC initialiser of the per-frame pose problems -------------------------------
 * What Tracking::GetInitModelCam / GetInitModelObj (reference src/Tracking.cc:1614-1715, 1717-1849) get from
 * cv::solvePnPRansac(pre_3d, cur_2d, K, distCoeffs = 0, rvec, tvec, false, 500, 0.4, 0.98, inliers,
 * SOLVEPNP_AP3P): the sequential RANSAC of OpenCV 3.4 (cv::RNG subsets of 4 points, minimal P3P solve on 3 with
 * the 4th as tie-breaker, inliers = squared reprojection error <= thr^2, iteration budget shrunk by
 * RANSACUpdateNumIters) with every hypothesis solved (AP3P) and voted on the GPU at once and the loop replayed on the
 * host over the votes.  `refit` is a FLAG WORD (below): bit 0 applies OpenCV's final EPnP re-estimation on the inliers (what
 * solvePnPRansac returns since 3.3 and what the reference's LM is seeded with - the host classes set it); with the bit clear
 * the winning minimal hypothesis is returned.  Behaviour change of round 5 for callers that pass 0 or 1: the minimal solver
 * is AP3P with the hypotheses re-orthogonalised as cv::Rodrigues does (bit 1 restores Grunert's P3P of rounds 1-4), so
 * hypotheses, inlier sets and poses of noisy problems differ from the earlier rounds'; a batch that mixes the two solvers
 * returns VDO_ERR_INVALID.  T = [R|t] camera-from-world (what Rodrigues(rvec), tvec give). */
typedef struct vdo_pnp_problem {
  int32_t n;
  const double* X;          /* [n][3] 3-D points (pre_3d)                         */
  const double* uv;         /* [n][2] pixels (cur_2d)                             */
  double K[4];              /* fx, fy, cx, cy                                     */
  int32_t max_iterations;   /* 500                                                */
  double reproj_threshold;  /* 0.4 px                                             */
  double confidence;        /* 0.98                                               */
  int32_t refit;            /* bit 0: the winning model is re-estimated on its inliers by EPnP, as cv::solvePnPRansac does for the P3P
                             *    / AP3P kernels since OpenCV 3.3 (the inlier set stays the RANSAC one); clear: the minimal hypothesis.
                             * bit 1 (value 2): Grunert's P3P as the minimal solver (rounds 1-4) instead of AP3P - Ke & Roumeliotis in the
                             *    layout of OpenCV 3.4's ap3p.cpp, the solver the reference's calls name (SOLVEPNP_AP3P), the default.
                             *    All problems of a batch must name the same solver.                                                */
} vdo_pnp_problem;
typedef struct vdo_pnp_result {
  double T[16];             /* 4x4 row-major; identity when no model was found    */
  int32_t n_inliers;        /* inliers.rows                                       */
  int32_t iterations_run;   /* hypotheses the sequential loop would have examined */
  int32_t best_iteration;   /* index of the winning hypothesis (-1: none)         */
} vdo_pnp_result;
/* All problems of a frame (camera + every object) in one call: two launches, one synchronisation. */
int vdo_pnp_ransac_batch(vdo_ctx* ctx, int n_problems, const vdo_pnp_problem* probs, vdo_pnp_result* results, uint8_t** inlier_out);
/* The same with a hook: host_work(host_arg) is called once, on the calling thread, while the device runs the hypotheses and the votes - for host work of the
 * caller that does not depend on the result (GetInitModelObj's motion-model inlier count, src/Tracking.cc:1767-1800, depends on neither).  NULL: no hook. */
int vdo_pnp_ransac_batch_overlap(vdo_ctx* ctx, int n_problems, const vdo_pnp_problem* probs, vdo_pnp_result* results, uint8_t** inlier_out,
                                 void (*host_work)(void*), void* host_arg);
/* The same for a caller that uses the re-estimated model of a problem only if its vote beats a count of the caller's own (GetInitModelCam / GetInitModelObj
 * seed the optimisation with the RANSAC model only if it has MORE inliers than the motion model, src/Tracking.cc:1690-1712, 1803-1825), and that has work to do
 * on the inlier flags which does not need the model:
 *   refit_above  [n_problems] or NULL (no gate).  Read after host_work has returned, so host_work may fill it.  Problem k is re-estimated by EPnP only if
 *                results[k].n_inliers > refit_above[k] (and its refit bit is set, as ever); otherwise T stays the winning hypothesis, exactly as with the bit
 *                off.  -1 therefore means "always".  Votes, flags, iterations_run and best_iteration never depend on the gate.
 *   after_replay (nullable) is called once, on the calling thread, when the inlier flags and results[].n_inliers / iterations_run / best_iteration are final
 *                and results[].T is NOT yet: the refits - a single one too - run on the pool threads meanwhile.  The call joins them before it returns.
 * VDO_PNP_NO_GATE in the environment (read on every call): refit_above is ignored and after_replay runs behind the refits. */
int vdo_pnp_ransac_batch_gated(vdo_ctx* ctx, int n_problems, const vdo_pnp_problem* probs, vdo_pnp_result* results, uint8_t** inlier_out,
                               const int32_t* refit_above, void (*host_work)(void*), void* host_arg, void (*after_replay)(void*), void* after_arg);
int vdo_pnp_ransac(vdo_ctx* ctx, const vdo_pnp_problem* p, vdo_pnp_result* result, uint8_t* inlier_out);

/* ---- ORB front-end ------------------------------------------------------------------------------
 * Replaces ORBextractor::ORBextractor (reference src/ORBextractor.cc:399-459) and
 * ORBextractor::operator() (:1035-1110): ComputePyramid (:1112-1137), ComputeKeyPointsOctTree
 * (:754-842: per-cell cv::FAST with threshold fallback, DistributeOctTree :528-752, IC_Angle
 * :66-93) and the per-level 7x7 GaussianBlur (:1083-1084).  vdo_orb_extract produces no descriptors, as the
 * reference does not (its computeDescriptors call is commented out at :1091); the rotated-BRIEF rows that call
 * would have written come from vdo_orb_descriptors / vdo_orb_extract_desc (K8) on request, and vdo_orb_match* consume them. */
typedef struct vdo_orb_params {
  int32_t n_features;     /* ORBextractor.nFeatures  2500 */
  float scale_factor;     /* ORBextractor.scaleFactor 1.2 */
  int32_t n_levels;       /* ORBextractor.nLevels    8    */
  int32_t ini_th;         /* ORBextractor.iniThFAST  20   */
  int32_t min_th;         /* ORBextractor.minThFAST  7    */
} vdo_orb_params;

/* SoA mirror of std::vector<cv::KeyPoint>; arrays are caller-allocated with `capacity` entries. */
typedef struct vdo_keypoints {
  int32_t capacity, n;
  float *x, *y, *response, *angle, *size;
  int32_t* octave;
} vdo_keypoints;

typedef struct vdo_orb vdo_orb;
/* Accepted: width, height >= 64, 1-16 levels, scale_factor > 1 (VDO_ERR_INVALID otherwise), every level at least 46 px on
 * both sides (VDO_ERR_UNSUPPORTED otherwise), no upper size limit.  Also VDO_ERR_UNSUPPORTED, naming the level: a level with
 * FAST cells whose keypoint region (the level minus 16 px on every side) is less than half as wide as it is tall -
 * DistributeOctTree would start from round(w/h) = 0 nodes, undefined behaviour in the reference (portrait images, deep
 * levels of tall ones). */
int vdo_orb_create(vdo_ctx* ctx, const vdo_orb_params* prm, int width, int height, vdo_orb** out);
int vdo_orb_destroy(vdo_orb* orb);
/* Upper bound on the keypoints one extraction returns (sum over the levels with cells of max(4 nIni, quota + 2), see
 * vdo_orb_create): the `capacity` of a vdo_keypoints that never fails.  It can exceed n_features - by far for small budgets. */
int vdo_orb_max_keypoints(const vdo_orb* orb, int* n);
/* Keypoints the last vdo_orb_extract / _end returned (0 before the first): the rows vdo_orb_descriptors and vdo_orb_match_extractors work on. */
int vdo_orb_last_keypoints(const vdo_orb* orb, int* n);
/* gray: 8-bit single channel, row stride `stride` bytes; host pointer unless src_is_device. */
int vdo_orb_extract(vdo_orb* orb, const uint8_t* gray, int stride, int src_is_device, vdo_keypoints* out);
/* The same in two halves: _begin queues the device stage (K3, K4, K5, K6, K7; the candidates and the ids of the selected ones are
 * written to mapped host memory) on the extractor's stream and returns at once, _end waits for it and builds the keypoints - a
 * caller overlaps other work with the device stage.
 * K5, DistributeOctTree, runs on the device (k_quadtree: one workgroup per level, the host's list bit for bit and in its order)
 * within these limits, all fixed before the launch: a level's quota N + 3 <= 1024 nodes (n_features up to about 4700 with the
 * default pyramid) and no more initial column strips than that; a level's keypoint region below 65536 px on both sides; at most
 * min(32768, cells of the level x candidates per cell) FAST candidates on the level; 48 rounds.  A level over the first two
 * limits takes the host tree from the start; on any other limit its workgroup writes a status word and stops, and _end runs the
 * host tree for that level - the results are the same either way.  With the device tree the angles of the returned keypoints are
 * computed with their rows; the angle row of ALL candidates (vdo_orb_get_candidates, the descriptors) is computed when first asked for.
 * Environment, read in vdo_orb_create: VDO_ORB_HOST_TREE=1
 * keeps every level on the host tree (helper threads: VDO_ORB_THREADS, default 3; they are not started otherwise), as does
 * VDO_ORB_FUSED_ANGLE=1; VDO_ORB_QT_NODE_CAP=n lowers the node limit (tests). */
int vdo_orb_extract_begin(vdo_orb* orb, const uint8_t* gray, int stride, int src_is_device);
int vdo_orb_extract_end(vdo_orb* orb, vdo_keypoints* out);
/* K8 - rotated BRIEF, the `_descriptors` output of ORBextractor::operator() (computeOrbDescriptor src/ORBextractor.cc:97-136,
 * pattern :139-397; the reference allocates the 32-byte rows but has the call commented out, :1083-1091).  vdo_orb_descriptors:
 * descriptors of the keypoints the last vdo_orb_extract / _end returned, same order, host buffer [capacity_rows][32];
 * vdo_orb_extract_desc = operator() with both outputs (desc32 nullable, [out->capacity][32]). */
int vdo_orb_descriptors(vdo_orb* orb, uint8_t* desc32, int capacity_rows);
int vdo_orb_extract_desc(vdo_orb* orb, const uint8_t* gray, int stride, int src_is_device, vdo_keypoints* out, uint8_t* desc32);
/* Inspection of the last extraction (mvImagePyramid is a public member of the reference class). */
int vdo_orb_level_info(vdo_orb* orb, int level, int* w, int* h, int* n_features, int* n_candidates);
int vdo_orb_get_pyramid(vdo_orb* orb, int level, uint8_t* out_bordered /* (w+38)*(h+38) */);
int vdo_orb_get_blurred(vdo_orb* orb, int level, uint8_t* out /* w*h */);
int vdo_orb_get_candidates(vdo_orb* orb, int level, float* x, float* y, float* response, float* angle, int cap, int* n);
/* Wall time of the last vdo_orb_extract: ms[0] device stage launch .. candidates on the host (with the device tree: and the
 * keypoint ids), ms[1] the rest of _end (host quadtrees, wait for the angles, keypoint rows). */
int vdo_orb_last_timing(vdo_orb* orb, double ms[2]);
/* Where K5 of `level` ran in the last extraction: *on_device 1 = k_quadtree, 0 = the host tree; *status 0, or why the level
 * took the host tree: 1 over the node limit at create (or VDO_ORB_HOST_TREE / VDO_ORB_FUSED_ANGLE), 2 more candidates than
 * the scratch holds, 3 more nodes than N + 3, 4 round limit, 5 a candidate outside the initial strips. */
int vdo_orb_tree_info(vdo_orb* orb, int level, int* on_device, int* status);
/* Diagnostic: K5 alone on given candidate lists instead of an image's.  level_count[n_levels]; x, y, resp level-major (level 0's
 * list first), x, y relative to the level's keypoint region as vdo_orb_get_candidates returns them.  The lists are placed where
 * the extraction's compaction puts its candidates, then the extraction's own tree launch and per-level resolution run (device
 * ids where the status is 0, the host tree otherwise; a handle created under VDO_ORB_HOST_TREE=1 runs the host tree);
 * vdo_orb_tree_info tells where each level ran.  sel: for level 0, 1, ... the indices INTO THAT LEVEL'S LIST of its keypoints,
 * in the order of the node list; sel_count[n_levels] their numbers.  Refused with VDO_ERR_INVALID, the message naming the
 * argument, and nothing written: a null argument, a negative count, more candidates in all than the extractor's dense
 * capacity, a sel_capacity below what the lists can return (per level min(count, max(4 nIni, n_features + 2))), an x or y that
 * is not an integer-valued float inside the level's region [0, w - 32) x [0, h - 32), a resp that is not an integer-valued
 * float in [0, 255] - what the compaction guarantees and the device tree relies on.  Afterwards the handle holds no keypoints
 * (vdo_orb_last_keypoints 0, no descriptors; vdo_orb_get_candidates returns the lists, with angles that mean nothing: no
 * pyramid stands behind them); the next vdo_orb_extract behaves as on a fresh handle. */
int vdo_orb_tree_run(vdo_orb* orb, const int32_t* level_count, const float* x, const float* y, const float* resp,
                     int32_t* sel, int sel_capacity, int32_t* sel_count);
/* Kernel launches that build the pyramid of one image: 2 (levels 0-4 cascaded in LDS from the image, the rest from level 4;
 * 1 with <= 5 levels) - possible with <= 8 levels whose cascaded source windows fit the LDS buffers - or n_levels (level by
 * level; also forced by the environment variable VDO_ORB_PYRAMID_LAUNCHES). */
int vdo_orb_pyramid_launches(const vdo_orb* orb);

/* ---- ORB descriptor matcher ---------------------------------------------------------------------
 * New (the reference keeps ORB-SLAM2's mDescriptors / mvKeysUn / feature grid but has no matcher): gated brute-force Hamming
 * search between two sets of 32-byte rotated-BRIEF rows.  For query row i, train row j is a CANDIDATE iff every gate that is
 * switched on passes:
 *   window gate (window >= 0):           fabsf(tx[j] - qx[i]) <= window && fabsf(ty[j] - qy[i]) <= window  - one fp32 subtraction,
 *                                        fabsf and compare per axis, nothing fused; a NaN position is never a candidate;
 *   octave gate (max_octave_diff >= 0):  |toct[j] - qoct[i]| <= max_octave_diff.
 * d(i, j) = popcount of the XOR of the two rows, 0..256.  Per query row:
 *   best_dist    the smallest d over the candidates, -1 without a candidate;
 *   second_dist  the second-smallest value of the MULTISET of candidate distances (== best_dist when two candidates tie), -1 with
 *                fewer than two candidates;
 *   train_idx    the lowest j that attains best_dist (what a sequential scan with strict < keeps) if every filter passes, else -1:
 *     distance     best_dist <= max_distance;
 *     ratio        only when 0 < ratio < 1 and a second candidate exists: (float)best_dist < ratio * (float)second_dist - one fp32
 *                  multiply, strict compare;
 *     cross-check  (cross_check != 0) the reverse best of train row j is i: over all query rows under the same gates, smallest
 *                  distance, lowest query index on ties, whatever the distance and ratio filters say.
 * *n_matches = rows with train_idx >= 0.  No result depends on chunk_rows or on any other tiling of the work. */

/* One side of a match.  desc: n rows of 32 bytes.  x, y (fp32) and octave are nullable: x and y are read only with the window gate on,
 * octave only with the octave gate on.  is_device: every pointer is a device pointer (desc 8-byte aligned), else a host pointer. */
typedef struct vdo_match_set {
  int32_t n;                        /* rows, 0 .. 1 << 24 */
  const uint8_t* desc;              /* [n][32] */
  const float *x, *y;               /* nullable */
  const int32_t* octave;            /* nullable */
  int32_t is_device;
} vdo_match_set;

/* Gates, filters and tiling of a match (see above). */
typedef struct vdo_match_params {
  int32_t max_distance;             /* 0..256; 256 accepts every best */
  float ratio;                      /* ratio test for 0 < ratio < 1, off otherwise; not NaN */
  float window;                     /* window gate half-width in pixels for >= 0, off for < 0; not NaN */
  int32_t max_octave_diff;          /* octave gate for >= 0, off for < 0 */
  int32_t cross_check;              /* != 0: keep mutual bests only */
  int32_t chunk_rows;               /* train rows per workgroup: >= 1 is honoured exactly, 0 picks it (about two workgroups per CU at 2 500 x 2 500) */
} vdo_match_params;

/* Matches `query` against `train` on the context's stream and returns when the outputs - host arrays of query->n entries each, and
 * *n_matches - are written.  With query->n == 0 or train->n == 0 nothing is launched and the outputs are -1.  Scratch comes from
 * the context (grown on demand, freed with it).  VDO_ERR_INVALID, the message naming the argument: a null struct, descriptor or
 * output pointer; window >= 0 without x and y on both sets; max_octave_diff >= 0 without octave on both sets; max_distance outside
 * 0..256; NaN ratio or window; n < 0 or n > 1 << 24; chunk_rows < 0.  VDO_ERR_UNSUPPORTED: a caller-given chunk_rows so small that
 * the partial results would take more than 65535 chunks or 1 GiB. */
int vdo_orb_match(vdo_ctx* ctx, const vdo_match_set* query, const vdo_match_set* train, const vdo_match_params* prm, int32_t* train_idx,
                  int32_t* best_dist, int32_t* second_dist, int32_t* n_matches);
/* The same between the keypoints of the LAST EXTRACTION of two extractors, in the order vdo_orb_extract returned them, with no host
 * round trip of descriptors or keypoints: K8 is queued for an extractor whose descriptors have not been asked for since, positions are
 * the returned level-0 x, y (bit for bit), octaves the returned octaves.  A later vdo_orb_descriptors returns the same bytes as ever.
 * The match runs on the query extractor's stream, ordered behind the train extractor's by an event; both must live on one device
 * (VDO_ERR_INVALID otherwise) and may be one object.  Outputs: host, the query extractor's keypoint count entries each; VDO_ERR_INVALID
 * when `capacity` is smaller than that, between vdo_orb_extract_begin and _end of either, and as for vdo_orb_match. */
int vdo_orb_match_extractors(vdo_orb* query, vdo_orb* train, const vdo_match_params* prm, int32_t* train_idx, int32_t* best_dist,
                             int32_t* second_dist, int32_t* n_matches, int32_t capacity);

/* K1: Tracking::GrabImageRGBD depth preprocessing (src/Tracking.cc:180-204), in place. */
int vdo_depth_preprocess(vdo_ctx* ctx, float* depth, int64_t n, float bf, float depth_map_factor, int is_device);
/* K2: cv::cvtColor(RGB2GRAY / BGR2GRAY) as called at src/Tracking.cc:209-222 (host in, host out). */
int vdo_rgb2gray(vdo_ctx* ctx, const uint8_t* rgb, int64_t n_pixels, int channels, int rgb_order, uint8_t* gray);

/* ---- Frame construction (src/Frame.cc:61-260) -------------------------------------------------*/
typedef struct vdo_frame_images vdo_frame_images;   /* HBM-resident depth (f32), flow (2 x f32), mask (i32) */
int vdo_frame_images_create(vdo_ctx* ctx, int width, int height, vdo_frame_images** out);
int vdo_frame_images_upload(vdo_frame_images* f, const float* depth, const float* flow, const int32_t* mask);
/* The same copies issued and awaited on the stream of `ctx` instead of the image set's own - for a host thread that brings the flow and the
 * mask of a frame up while another one already works on its depth map (the reference hands TrackRGBD host cv::Mat's, include/System.h:45-51). */
int vdo_frame_images_upload_on(vdo_ctx* ctx, vdo_frame_images* f, const float* depth, const float* flow, const int32_t* mask);
int vdo_frame_images_upload_device(vdo_frame_images* f, const float* depth_dev, const float* flow_dev, const int32_t* mask_dev);
int vdo_frame_images_depth_preprocess(vdo_frame_images* f, float bf, float depth_map_factor);   /* K1 in place, resident image */
/* vdo_frame_images_upload_device + (convert_depth != 0) vdo_frame_images_depth_preprocess as ONE launch (GrabImageRGBD's head,
 * src/Tracking.cc:180-204 + the cv::Mat headers it keeps): same bytes, same two divisions per depth pixel, a quarter of the stream operations. */
int vdo_frame_images_ingest_device(vdo_frame_images* f, const float* depth_dev, const float* flow_dev, const int32_t* mask_dev, float bf, float depth_map_factor,
                                   int convert_depth);
int vdo_frame_images_destroy(vdo_frame_images* f);
/* Later calls on these images run on `ctx` (its stream and scratch arena) instead of the context they were created with.
 * Every call on vdo_frame_images is host-synchronous, so the switch needs no device-side ordering; it exists so that a
 * host worker thread can work on the images of one frame while the main thread works on another context (FramePipeline). */
int vdo_frame_images_set_ctx(vdo_frame_images* f, vdo_ctx* ctx);
/* K9: static keypoint filter of Frame::Frame (:100-128) + depth gather (:178-194); outputs in input order. */
int vdo_frame_static_filter(vdo_frame_images* f, int n, const float* kx, const float* ky, float th_depth,
                            int32_t* keep_idx, float* corr_x, float* corr_y, float* flow_x, float* flow_y,
                            float* depth_out, int* n_out);
/* The same for UseSampleFeature = 1 (src/Frame.cc:132-166: the destination is tested on all four sides), and the sampler that
 * replaces ORB there: Frame::SampleKeyPoints (:672-737), 3000 random grid positions from cv::RNG(seed); host only. */
int vdo_frame_static_filter_sampled(vdo_frame_images* f, int n, const float* kx, const float* ky, float th_depth,
                                    int32_t* keep_idx, float* corr_x, float* corr_y, float* flow_x, float* flow_y,
                                    float* depth_out, int* n_out);
int vdo_sample_keypoints(int rows, int cols, uint64_t seed, int capacity, float* x_out, float* y_out, int* n_out);
/* K10: semi-dense object sampling (:201-228), raster order.  Pass key_x == NULL to keep results on the device. */
int vdo_frame_object_sample(vdo_frame_images* f, float th_depth_obj, int step, int cap,
                            float* key_x, float* key_y, float* corr_x, float* corr_y,
                            float* flow_x, float* flow_y, float* depth_out, int32_t* label, int* n_out);
/* K10 on the stream of `on_ctx` (NULL: the image set's own) with a scratch set of its own: for a caller that samples the objects on
 * a second host thread while the owning thread runs K9 / RenewFrameInfo on the same image set.  Host outputs required. */
int vdo_frame_object_sample_on(vdo_ctx* on_ctx, vdo_frame_images* f, float th_depth_obj, int step, int cap,
                               float* key_x, float* key_y, float* corr_x, float* corr_y,
                               float* flow_x, float* flow_y, float* depth_out, int32_t* label, int* n_out);
/* K9 + K10 of one image in one call and ONE synchronisation (Frame::Frame runs them back to back: src/Frame.cc:104-131 / 132-166,
 * 168-199): the arguments of vdo_frame_static_filter[_sampled] (sampled != 0: the UseSampleFeature branch) followed by those of
 * vdo_frame_object_sample (host outputs required). */
int vdo_frame_filters(vdo_frame_images* f, int n, const float* kx, const float* ky, float th_depth, int sampled,
                      int32_t* keep_idx, float* s_corr_x, float* s_corr_y, float* s_flow_x, float* s_flow_y, float* s_depth, int* n_static,
                      float th_depth_obj, int step, int cap,
                      float* key_x, float* key_y, float* corr_x, float* corr_y, float* flow_x, float* flow_y, float* depth_out, int32_t* label, int* n_obj);
/* The same on the stream of `on_ctx` instead of the image set's own context (NULL: the latter): for a caller that runs K9 / K10 on a
 * second host thread while the owning thread keeps using the image set (the scratch of this call is used by nothing else). */
int vdo_frame_filters_on(vdo_ctx* on_ctx, vdo_frame_images* f, int n, const float* kx, const float* ky, float th_depth, int sampled,
                         int32_t* keep_idx, float* s_corr_x, float* s_corr_y, float* s_flow_x, float* s_flow_y, float* s_depth, int* n_static,
                         float th_depth_obj, int step, int cap,
                         float* key_x, float* key_y, float* corr_x, float* corr_y, float* flow_x, float* flow_y, float* depth_out, int32_t* label, int* n_obj);

/* ---- Tracking-side gathers over the resident images ------------
 * All coordinate arrays are host pointers (the reference keeps them in std::vector<cv::KeyPoint>). */

/* Tracking::GrabImageRGBD, static correspondences: depth at ((int)kx,(int)ky) if inside the
 * 1-px-inset image and > 0, else -1.  Replaces src/Tracking.cc:259-275. */
int vdo_propagate_static(vdo_frame_images* f, int n, const float* kx, const float* ky, float* depth_out);
/* Object correspondences: (depth,label) if inside and 0 < depth < th_depth_obj, else (0.1, 0).
 * Replaces src/Tracking.cc:278-305. */
int vdo_propagate_object(vdo_frame_images* f, int n, const float* kx, const float* ky, float th_depth_obj,
                         float* depth_out, int32_t* label_out);
/* Optimizer::Get3DinWorld over a vector of keypoints: Twc[:3,:3]*x3Dc + Twc[:3,3] with cv::gemm
 * rounding (double accumulate, one rounding).  Replaces src/Optimizer.cc:2974-2995 (called per point
 * from Tracking.cc:1086,1094 and Optimizer builders).  K4 = fx,fy,cx,cy ; Twc row-major 4x4. */
int vdo_get3d_world(vdo_ctx* ctx, int n, const float* kx, const float* ky, const float* depth,
                    const float K4[4], const float Twc[16], float* xyz_out);
/* Tracking::GetSceneFlowObj: flow3d = X_cur - X_last with both points back-projected through
 * Frame::UnprojectStereoObject / UnprojectStereoObjectLast (src/Frame.cc:517-555); entries whose
 * semantic label is <= 0 in either frame get obj_label = -1 and zero flow.  Replaces src/Tracking.cc:1278-1364 (per-point part). */
int vdo_scene_flow(vdo_ctx* ctx, int n, const float* cur_x, const float* cur_y, const float* cur_d, const int32_t* cur_label, const float Tcw_cur[16],
                   const float* last_x, const float* last_y, const float* last_d, const int32_t* last_label, const float Tcw_last[16],
                   const float K4[4], float* flow3d_out, int32_t* obj_label_inout);
/* Tracking::RenewFrameInfo, static part (src/Tracking.cc:2666-2790): carry the inliers TM_sta, top
 * up from the ORB keypoints (stride-20 interleave, skipping keypoints within 1 px of a carried one),
 * then depth.  Outputs need capacity max_num_sta + 1 ; *n_out = count. */
int vdo_renew_static(vdo_frame_images* f, int n_tm, const int32_t* tm_sta, const float* stat_x, const float* stat_y,
                     int n_orb, const float* orb_x, const float* orb_y, int max_num_sta,
                     float* key_x, float* key_y, float* corr_x, float* corr_y, float* flow_x, float* flow_y,
                     int32_t* inlier_id, float* depth_out, int* n_out);
/* The same + Optimizer::Get3DinWorld of the new set (mvStat3DPointTmp, src/Tracking.cc:2784-2790) in one pass over the device
 * (one synchronisation): xyz_out [3 * (max_num_sta + 1)], nullable (K4 / Twc unused then). */
int vdo_renew_static_world(vdo_frame_images* f, int n_tm, const int32_t* tm_sta, const float* stat_x, const float* stat_y,
                           int n_orb, const float* orb_x, const float* orb_y, int max_num_sta, const float K4[4], const float Twc[16],
                           float* key_x, float* key_y, float* corr_x, float* corr_y, float* flow_x, float* flow_y,
                           int32_t* inlier_id, float* depth_out, float* xyz_out, int* n_out);
/* New (no counterpart in the reference): K9 of the ORB keypoints (vdo_frame_static_filter) and vdo_renew_static_world topping up from the SAME keypoints, as one
 * round trip - K9 is queued in front of the renewal kernels on the keypoints the renewal sends and writes its rows where the host reads them, one
 * synchronisation delivers both.  Returns exactly what the two calls
 * return one after the other: first K9's outputs (capacity n_orb each, *n_static = count), then the renewal's.  For the ORB mode once a last frame exists; where
 * the renewal tops up from K9's own output (UseSampleFeature, Initialization) the two calls stay two.  VDO_ERR_INVALID as vdo_frame_static_filter when the
 * keypoints exceed the image set's staging (10 * n_orb > 8 * capacity). */
int vdo_static_stage(vdo_frame_images* f, int n_orb, const float* orb_x, const float* orb_y, float th_depth,
                     int32_t* keep_idx, float* s_corr_x, float* s_corr_y, float* s_flow_x, float* s_flow_y, float* s_depth, int* n_static,
                     int n_tm, const int32_t* tm_sta, const float* stat_x, const float* stat_y, int max_num_sta, const float K4[4], const float Twc[16],
                     float* key_x, float* key_y, float* corr_x, float* corr_y, float* flow_x, float* flow_y,
                     int32_t* inlier_id, float* depth_out, float* xyz_out, int* n_out);
/* Tracking::UpdateMask (src/Tracking.cc:3015-3065): labels of this frame's mask at n positions
 * (-1 outside), and the warp of label `label` from `last`'s mask into `cur`'s mask by `last`'s flow. */
int vdo_mask_at(vdo_frame_images* f, int n, const float* cx, const float* cy, int32_t* label_out);
int vdo_mask_warp(vdo_frame_images* cur, vdo_frame_images* last, int32_t label);
int vdo_frame_images_download_mask(vdo_frame_images* f, int32_t* mask_out);
/* The resident depth image after K1 (metres): GrabImageRGBD converts the caller's imD in place (src/Tracking.cc:180-204); a host
 * caller that uploaded the raw map gets the converted one back with this. */
int vdo_frame_images_download_depth(vdo_frame_images* f, float* depth_out);
/* The resident flow image, [h][w][2] floats. */
int vdo_frame_images_download_flow(vdo_frame_images* f, float* flow_out);

/* ---- Tracking bookkeeping around the gathers ------------------------------------ */

/* Tracking::DynObjTracking (src/Tracking.cc:1366-1612): groups the object points of the current frame
 * by semantic label; drops labels with > 50 % of their points in the image border (obj label -1),
 * labels whose share of slow points (||flow3d_xz|| < sf_mg_thres) exceeds sf_ds_thres become static
 * (obj label 0), labels with mean depth > th_depth_obj or < 150 points are dropped (-1); the survivors
 * get the motion label of the last-frame object whose semantic label wins the vote of their points'
 * last-frame labels (else a fresh id from *max_id_inout).  flow3d comes from vdo_scene_flow.
 * Outputs: obj_label_inout updated; accepted objects as CSR obj_off[n_obj+1] / obj_idx (capacity n),
 * obj_sem / obj_mod (capacity: number of distinct labels). */
typedef struct vdo_dyn_obj_params {
  int32_t img_w, img_h;
  int32_t shrink_row, shrink_col; /* 25 / 50 on KITTI, 0 / 0 otherwise (:1412-1416)               */
  float sf_mg_thres, sf_ds_thres; /* Tracking::fSFMgThres / fSFDsThres (yaml SFMgThres, SFDsThres) */
  float th_depth_obj;             /* mThDepthObj                                                   */
  int32_t f_id;                   /* frame id: 1 resets the id counter (:1536-1537)                 */
} vdo_dyn_obj_params;
int vdo_dyn_obj_tracking(const vdo_dyn_obj_params* prm, int n, const int32_t* sem_label, int32_t* obj_label_inout,
                         const float* key_x, const float* key_y, const float* depth, const float* flow3d, const int32_t* last_sem_label,
                         int n_last_obj, const int32_t* last_sem_pos, const int32_t* last_mod_label, const uint8_t* last_obj_stat,
                         int32_t* max_id_inout, int32_t* obj_off, int32_t* obj_idx, int32_t* obj_sem, int32_t* obj_mod, int* n_obj_out);

/* Tracking::RenewFrameInfo, object part (src/Tracking.cc:2806-2995).  `f` holds the NEW frame's images.
 * Carries the inliers of every tracked object (int-truncated position must lie on a mask != 0 with
 * 0 < depth < 25 and flow inside the image), tops every tracked object up to max_num_obj from the
 * semi-dense sampling tmp_* of the new image (stride-15 interleave, skipping samples within 1 px of a
 * carried point), then appends all samples of labels that are not tracked yet (object label -2).
 * Outputs (capacity `cap` each): key, depth, semantic label, flow, correspondence, inlier id (-1 for
 * added points), object label. */
int vdo_renew_object(vdo_frame_images* f, int n_obj, const int32_t* inl_off, const int32_t* inl_idx, const uint8_t* obj_stat,
                     const int32_t* sem_pos, const int32_t* mod_label,
                     const float* cur_x, const float* cur_y, const int32_t* cur_obj_label,
                     int n_tmp, const float* tmp_x, const float* tmp_y, const float* tmp_depth, const int32_t* tmp_label,
                     const float* tmp_flow_x, const float* tmp_flow_y, const float* tmp_corr_x, const float* tmp_corr_y,
                     int max_num_obj, int cap,
                     float* key_x, float* key_y, float* depth_out, int32_t* sem_out, float* flow_x, float* flow_y,
                     float* corr_x, float* corr_y, int32_t* dyn_inlier_id, int32_t* obj_label_out, int* n_out);
/* The same + the 3-D points of the new set (mvObj3DPoint, src/Tracking.cc:2981-2990) in one pass over the device (one
 * synchronisation): xyz_out [3 * cap], nullable (K4 / Twc unused then). */
int vdo_renew_object_world(vdo_frame_images* f, int n_obj, const int32_t* inl_off, const int32_t* inl_idx, const uint8_t* obj_stat,
                           const int32_t* sem_pos, const int32_t* mod_label,
                           const float* cur_x, const float* cur_y, const int32_t* cur_obj_label,
                           int n_tmp, const float* tmp_x, const float* tmp_y, const float* tmp_depth, const int32_t* tmp_label,
                           const float* tmp_flow_x, const float* tmp_flow_y, const float* tmp_corr_x, const float* tmp_corr_y,
                           int max_num_obj, int cap, const float K4[4], const float Twc[16],
                           float* key_x, float* key_y, float* depth_out, int32_t* sem_out, float* flow_x, float* flow_y,
                           float* corr_x, float* corr_y, int32_t* dyn_inlier_id, int32_t* obj_label_out, float* xyz_out, int* n_out);

/* Tracking::UpdateMask (src/Tracking.cc:2997-3068) in one stream-ordered sequence without host round
 * trips: per last-frame semantic label (ascending) the labels of `cur`'s mask at the flowed positions
 * vote; with >= 100 votes and background winning, that label's pixels of `last`'s mask are warped by
 * `last`'s flow into `cur`'s mask (visible to the next label's vote, as in the reference). */
int vdo_update_mask(vdo_frame_images* cur, vdo_frame_images* last, int n, const int32_t* last_sem_label,
                    const float* last_corr_x, const float* last_corr_y, int* n_recovered);
/* UpdateMask (K15) -> object part of the propagation (K11) -> GetSceneFlowObj (K13) in one call (src/Tracking.cc:2997-3068,
 * :283-305, :1278-1364): what vdo_update_mask + vdo_propagate_object + vdo_scene_flow do in that order, with one upload, one
 * download and one synchronisation.  obj_label_out starts at -2 like vObjLabel (Tracking.cc:1289). */
int vdo_object_chain(vdo_frame_images* cur, vdo_frame_images* last, int n, const int32_t* last_sem_label, const float* last_corr_x, const float* last_corr_y,
                     float th_depth_obj, const float Tcw_cur[16], const float* last_x, const float* last_y, const float* last_d, const float Tcw_last[16],
                     const float K4[4], int* n_recovered, float* depth_out, int32_t* sem_out, float* flow3d_out, int32_t* obj_label_out);
/* vdo_object_chain in two halves, for a caller that does not know the current camera pose yet: of the chain only the scene flow reads Tcw_cur.
 *   begin: stages the last frame's inputs (or finds them prestaged, as vdo_object_chain does), queues UpdateMask (K15) on the stream of cur's context and
 *          returns WITHOUT waiting.  The arrays must stay valid and unchanged until the end has returned.
 *   end:   queues K11 (objects) + K13 with Tcw_cur, synchronises once, checks the flags and delivers what vdo_object_chain delivers.
 * vdo_object_chain is the begin followed by the end.  One chain can be open per context; between its begin and its end no other call may use that context's
 * scratch (every vdo_frame_images call on a set of that context, vdo_pnp_ransac*, vdo_get3d_world, vdo_scene_flow on it: they fail with VDO_ERR_OOM), and
 * nothing else may touch the two image sets.  A begin that fails leaves no chain open (a second begin on a context fails and leaves the first open); an end
 * closes the chain whether it succeeds or not - also when it reports a mask label outside the vote's histogram.  n == 0: the begin queues nothing and opens
 * nothing; an end with no chain open returns VDO_OK and writes only *n_recovered = 0. */
int vdo_object_chain_begin(vdo_frame_images* cur, vdo_frame_images* last, int n, const int32_t* last_sem_label, const float* last_corr_x, const float* last_corr_y,
                           const float* last_x, const float* last_y, const float* last_d);
int vdo_object_chain_end(vdo_frame_images* cur, float th_depth_obj, const float Tcw_cur[16], const float Tcw_last[16], const float K4[4],
                         int* n_recovered, float* depth_out, int32_t* sem_out, float* flow3d_out, int32_t* obj_label_out);
/* Optional, new (no counterpart in the reference): the inputs of vdo_object_chain that belong to the LAST frame (mLastFrame's object set: vSemObjLabel, mvObjCorres,
 * mvObjKeys, mvObjDepth - src/Tracking.cc:1040-1063 leaves them final at the end of Track()) sent to the device a frame ahead, asynchronously on `ctx`'s stream.  The
 * next vdo_object_chain on a frame of that context uses them if - compared value by value - they are what it is called with, and otherwise stages its inputs itself. */
int vdo_object_chain_prestage(vdo_ctx* ctx, int n, const int32_t* last_sem_label, const float* last_corr_x, const float* last_corr_y,
                              const float* last_x, const float* last_y, const float* last_d);

/* Tracklets: Tracking::GetStaticTrack / GetDynamicTrackNew (src/Tracking.cc:2201-2421) rebuild every
 * tracklet from frame 0 on every frame; this builder is incremental (one association vector per call)
 * and yields the same tracklets in the same order.  Host only. */
typedef struct vdo_tracks vdo_tracks;
int vdo_tracks_create(int with_object_label, vdo_tracks** out);
int vdo_tracks_destroy(vdo_tracks* t);
int vdo_tracks_add_frame(vdo_tracks* t, int n, const int32_t* asso /* index in the previous frame or -1 */, const int32_t* feat_label);
int vdo_tracks_size(vdo_tracks* t, int* n_tracks, int64_t* n_pairs);
int vdo_tracks_get(vdo_tracks* t, int32_t* track_off, int32_t* pair_frame, int32_t* pair_feat, int32_t* obj_id);
/* Only the tracks still observed in frame >= first_frame, whole and in creation order (buffers sized as for vdo_tracks_get; *n_tracks / *n_pairs = what was written):
 * what the windowed optimisation reads (Optimizer::PartialBatchOptimization, reference src/Optimizer.cc:42-1230, walks mpMap->TrackletSta of the window's frames). */
int vdo_tracks_get_since(vdo_tracks* t, int first_frame, int* n_tracks, int64_t* n_pairs, int32_t* track_off, int32_t* pair_frame, int32_t* pair_feat, int32_t* obj_id);

/* ---- Dataset ingest: one frame's four files decoded on the device (example/vdo_slam.cc:104-131) ------------------------------
 * What the driver does on one host thread per frame - LoadMask's text parse, the PNG scanline un-filter (PNG spec 9.2) + pixel
 * conversion, the .flo copy - as kernels, into the four device images FramePipeline::Step takes.  The host keeps only the file reads
 * and zlib's inflate (vdo_slam_amd/host/DatasetIO.h: InflatePNG).  A handle is sized once per sequence (width x height of the images). */
typedef struct vdo_ingest vdo_ingest;
/* An inflated PNG image: `height` rows of (1 filter byte + width * channels * bit_depth / 8 bytes), host memory. */
typedef struct vdo_png_scanlines {
  const uint8_t* data;
  int64_t bytes;
  int32_t width, height, bit_depth, channels;
} vdo_png_scanlines;
enum { VDO_INGEST_MASK = 0, VDO_INGEST_FLO = 1, VDO_INGEST_DEPTH = 2, VDO_INGEST_COLOR = 3 };
int vdo_ingest_create(vdo_ctx* ctx, int width, int height, vdo_ingest** out);
int vdo_ingest_destroy(vdo_ingest* h);
/* The handle's pinned staging buffer of one input kind (VDO_INGEST_*), grown to >= bytes (contents are not kept when it grows).  A
 * file read or inflated straight into it goes to the device by DMA; any other host pointer is accepted by vdo_ingest_frame as well. */
int vdo_ingest_host_buffer(vdo_ingest* h, int which, int64_t bytes, void** ptr);
/* Device images owned by the handle (width x height: gray u8, depth_raw f32, flow 2 x f32, mask i32), for callers without their own. */
int vdo_ingest_device_outputs(vdo_ingest* h, uint8_t** gray, float** depth_raw, float** flow, int32_t** mask);
/* One frame, host-synchronous.  Outputs are DEVICE pointers; a part whose output is NULL is skipped (its input is not read).
 *   mask  <- mask_text: the result of LoadMask (host/DatasetIO.cc) on these bytes, rows = height, cols = width;
 *   flow  <- flo: a Middlebury .flo file (magic 202021.25, width / height equal to the handle's), payload copied as it is;
 *   depth_raw <- depth: 8/16-bit grey scanlines as float (ReadPNG(.., as_float = true));
 *   gray  <- color: 8-bit grey / RGB / RGBA scanlines as ReadPNG's image (BGR(A), like cv::imread) through vdo_rgb2gray(.., rgb_order).
 * VDO_ERR_INVALID (the message names the file kind) for a bad .flo header, a size that is not the handle's, a filter byte > 4, an
 * unsupported bit depth / channel count or a mask text without a row - and then nothing is written.  No CPU fallback. */
int vdo_ingest_frame(vdo_ingest* h, const char* mask_text, int64_t mask_bytes, const void* flo, int64_t flo_bytes, const vdo_png_scanlines* depth,
                     const vdo_png_scanlines* color, int rgb_order, uint8_t* gray, float* depth_raw, float* flow, int32_t* mask);
/* The last vdo_ingest_frame: ms[0] wall time of the call, ms[1] device time from the first upload to the last kernel (events),
 * ms[2] device time of the kernels alone (after the uploads). */
int vdo_ingest_last_timing(vdo_ingest* h, double ms[3]);

/* ---- Stereo matcher: census + semi-global matching -------------------------------------------------------------------------------
 * New (the reference consumes a stereo disparity map x 256 as its depth input, src/Tracking.cc:180-204, and leaves making it to an offline
 * matcher): from a rectified pair of 8-bit grey images to disparity in 1/256 px, float - the `depth_raw` image that
 * vdo_frame_images_ingest_device(.., bf, 256, convert_depth = 1) and FramePipeline::Step take.  Integer arithmetic in every stage; the
 * result does not depend on the order in which directions or workgroups run.  With W x H images, D = max_disparity, candidates d = 0 .. D-1:
 *
 * 1. Census, 9 wide x 7 high, 62 bits in a uint64.  For pixel (x, y), bit k is 1 iff I(clamp(x+dx, 0, W-1), clamp(y+dy, 0, H-1)) < I(x, y);
 *    k counts the window offsets in raster order - dy = -3 .. 3 outer, dx = -4 .. 4 inner, the centre skipped - and bit k sits at bit position k.
 * 2. Cost, 0 .. 62.  C(x, y, d) = popcount(cL(x, y) ^ cR(x-d, y)) when x - d >= 0, else 62.
 * 3. Aggregation.  The directions r = (dx, dy) are the first `paths` of (1,0), (-1,0), (0,1), (0,-1), (1,1), (-1,1), (1,-1), (-1,-1); the
 *    predecessor of p is p - r.  If p - r lies outside the image, L_r(p, d) = C(p, d); otherwise
 *      L_r(p, d) = C(p, d) + min(L_r(p-r, d), L_r(p-r, d-1) + P1, L_r(p-r, d+1) + P1, m + P2) - m,   m = min_k L_r(p-r, k),
 *    where a d-1 or d+1 outside [0, D) takes no part.  S = sum over r of L_r.  P1, P2 are constants.  L_r <= 62 + P2, so S <= 8 * (62 + P2) < 2^16.
 * 4. Selection, per pixel; the output is 0 (invalid) as soon as one rule fails.  d* = argmin_d S(x, y, d), the lowest d on ties; s0 = its value.
 *      (a) d* >= 1 (disparity 0 is infinite depth; K1 and the depth gates read 0 as "no depth");
 *      (b) x - d* >= 0;
 *      (c) uniqueness, if uniqueness > 0: 100 * s0 < (100 - uniqueness) * s2, s2 = the minimum of S over |d - d*| > 1 (+infinity, hence passed, if
 *          there is no such d);
 *      (d) left-right check, if lr_max_diff >= 0: dR(x', y) = argmin over d with x' + d < W of S(x'+d, y, d), lowest d on ties - the right image's
 *          disparity read from the same volume; require |dR(x - d*, y) - d*| <= lr_max_diff.
 *    Sub-pixel, if subpixel != 0, 1 <= d* <= D-2 and den = S(d*-1) + S(d*+1) - 2 * s0 > 0: num = 128 * (S(d*-1) - S(d*+1)),
 *    off = sign(num) * ((2 * |num| + den) / (2 * den)) in integer division; otherwise off = 0.
 *    Output: (float)(256 * d* + off) - an integer below 2^17, exact in fp32.  *n_valid = the number of non-zero outputs. */
typedef struct vdo_stereo vdo_stereo;
typedef struct vdo_stereo_params {
  int32_t max_disparity;            /* D: a multiple of 16 in 16..256 */
  int32_t p1, p2;                   /* 1 <= p1 <= p2 <= 1000 */
  int32_t paths;                    /* 4 or 8 */
  int32_t uniqueness;               /* 0..99; 0 switches rule (c) off */
  int32_t lr_max_diff;              /* >= -1; -1 switches rule (d) off */
  int32_t subpixel;                 /* != 0: sub-pixel offset */
} vdo_stereo_params;
/* A matcher for width x height images.  ALL device memory is taken here (two staged images, two census images, the uint8 cost volume
 * [y][x][d], the uint16 volume of sums in the same layout, one float image): 3 bytes per volume entry + 22 per pixel; vdo_stereo_compute
 * allocates nothing.  VDO_ERR_INVALID, the message naming the argument: width or height < 1; max_disparity not a multiple of 16 in 16..256;
 * paths not 4 or 8; not 1 <= p1 <= p2 <= 1000; uniqueness outside 0..99; lr_max_diff < -1; a null pointer.  VDO_ERR_UNSUPPORTED when
 * width * height * max_disparity > 2^28.  VDO_ERR_OOM when the device has no room. */
int vdo_stereo_create(vdo_ctx* ctx, int width, int height, const vdo_stereo_params* params, vdo_stereo** out);
int vdo_stereo_destroy(vdo_stereo* h);
/* One pair, host-synchronous, on the context's stream.  left / right: rows of `width` bytes, *_stride bytes apart (>= width); host pointers, or
 * device pointers when src_is_device != 0 (read where they are).  disparity256: width x height floats, packed, a device pointer when
 * out_is_device != 0; n_valid: host.  VDO_ERR_INVALID, the message naming the argument, for a null image, output or count and a stride < width -
 * and then NOTHING is written.  No state of an earlier compute on the handle enters the result. */
int vdo_stereo_compute(vdo_stereo* h, const uint8_t* left, int64_t left_stride, const uint8_t* right, int64_t right_stride, int src_is_device,
                       float* disparity256, int out_is_device, int32_t* n_valid);
/* The output is multiplied by `scale` (fp32, one multiply fused into the selection; 1 by default, which changes no bit): a pipeline whose
 * DepthMapFactor is f takes scale = f / 256, so that K1's d / f is the disparity in pixels again.  Only a power of two keeps that composition
 * exact.  VDO_ERR_INVALID outside (0, 65536]. */
int vdo_stereo_set_output_scale(vdo_stereo* h, float scale);
/* Inspection of the LAST compute (VDO_ERR_INVALID before the first), host outputs: the census image of the left (which = 0) or right (1)
 * image [H][W]; the cost volume [H][W][D]; the volume of sums S [H][W][D]. */
int vdo_stereo_get_census(vdo_stereo* h, int which, uint64_t* out);
int vdo_stereo_get_cost(vdo_stereo* h, uint8_t* out);
int vdo_stereo_get_aggregated(vdo_stereo* h, uint16_t* out);
/* The last compute: ms[0] wall time of the call, ms[1] device time from the first upload to the end of the selection kernel (events). */
int vdo_stereo_last_timing(vdo_stereo* h, double ms[2]);
/* Device images owned by the handle, for callers without their own: the packed width x height staging images a HOST pair is uploaded to (after
 * such a compute `left` is the left image on the device) and a float image to pass as a device disparity256.  Any of the three may be NULL. */
int vdo_stereo_device_images(vdo_stereo* h, uint8_t** left, uint8_t** right, float** disparity256);
/* Brings the frame's other two host images (flow 2 x f32, mask i32, width x height, packed) to device images owned by the handle (made on the
 * first call), for a caller that hands the whole frame to a device-input step (Tracking::GrabImageStereo).  Host-synchronous. */
int vdo_stereo_stage_frame(vdo_stereo* h, const float* flow, const int32_t* mask, float** flow_dev, int32_t** mask_dev);

/* ---- Dense optical-flow matcher: coarse-to-fine census search ---------------------------------------------------------------------
 * New (the reference's TrackRGBD takes a dense flow image per frame, src/Tracking.cc:164-314 / src/Frame.cc, and leaves making it to an offline
 * flow network): from two 8-bit grey images I0, I1 of W x H to flow[H][W][2] fp32, u then v - the .flo payload layout vdo_ingest_frame and
 * FramePipeline::Step take.  Pixel (x, y) of I0 is seen at (x + u, y + v) in I1; the flow image handed in with frame t is the flow from frame t
 * to frame t + 1 (the reference's Frame adds it to reach the next frame).  Integer arithmetic in every stage; no result depends on workgroup
 * shape or order.  L = levels, r = radius, w = window; the search range per axis is r * (2^L - 1) pixels.
 *
 * 1. Pyramid, per image.  Level 0 is the image; level l+1 has size (ceil(W_l / 2), ceil(H_l / 2)) and
 *    P(x, y) = (a + b + c + d + 2) >> 2 over the 2 x 2 block at (2x, 2y) of level l, the + 1 coordinates clamped to W_l - 1 / H_l - 1.
 *    Every size >= 1 x 1 is legal at every L: a 1 x 1 level halves to 1 x 1.
 * 2. Census, per level and image: step 1 of the stereo section above (9 x 7, 62 bits, clamped borders, the same bit order).
 * 3. Search, from level L-1 down to 0, per pixel of the level.  Prior (u0, v0) = (0, 0) at level L-1, else 2 * F_{l+1}(x >> 1, y >> 1).
 *    Candidates (du, dv) in [-r, r]^2, ranked k = 0, 1, .. by ascending (du^2 + dv^2, dv, du): zero displacement is k = 0.  Cost
 *      A(k) = sum_{j=-w..w} sum_{i=-w..w} popcount(c0(cx(x+i), cy(y+j)) ^ c1(cx(x+i+u0+du), cy(y+j+v0+dv))),
 *    cx, cy clamping into the level's image: the prior of the CENTRE pixel moves the whole block.  A <= 62 * 81.  k* = argmin of the packed
 *    key (A << 8) | k; F_l = (u0 + du*, v0 + dv*).  If median != 0 and l >= 1, each component of F_l is then replaced by the median (the fifth of
 *    the nine sorted values) of its clamped 3 x 3 neighbourhood before the level below reads it.  Level 0 is never filtered.
 * 4. Sub-pixel, level 0 only, per component: for u, if subpixel != 0 and |du*| < r, with A- = A(du*-1, dv*), A+ = A(du*+1, dv*) and
 *    den = A- + A+ - 2 A*: if den > 0, num = 128 * (A- - A+), off = sign(num) * ((2 * |num| + den) / (2 * den)) in integer division (the stereo
 *    formula); otherwise off = 0.  v likewise with dv.  Output u = (float)(256 * u_int + off) * (1 / 256): exact in fp32.
 * 5. Forward-backward check.  If fb_max_diff >= 0 the backward integer flow B is steps 1-3 with the images' roles swapped (the pyramids and
 *    census images are shared); a pixel is valid iff p' = (x + u_int, y + v_int) lies in the image and
 *    max(|u_int + B_u(p')|, |v_int + B_v(p')|) <= fb_max_diff.  With -1 nothing backward runs and every pixel is valid.  The flow is written
 *    for EVERY pixel, valid or not (a tracker wants a guess at an occlusion); *n_valid = the number of valid pixels.
 * A constant pair gives flow 0 everywhere (the tie rule). */
typedef struct vdo_optflow vdo_optflow;
typedef struct vdo_optflow_params {
  int32_t levels;                   /* L: 1..7 pyramid levels */
  int32_t radius;                   /* r: 1..4, search radius per level */
  int32_t window;                   /* w: 0..4, box half-width of the block sum */
  int32_t median;                   /* 0 / 1: 3 x 3 median between levels */
  int32_t fb_max_diff;              /* >= -1; -1 switches the forward-backward check off */
  int32_t subpixel;                 /* 0 / 1: sub-pixel offset */
} vdo_optflow_params;
/* A matcher for width x height images.  ALL device memory is taken here (per image the pyramid and its census images, per direction the integer
 * flows of every level, one more level-1 flow image for the median, a float flow image and a validity image: about 60 bytes per pixel);
 * vdo_optflow_compute allocates nothing.  VDO_ERR_INVALID, the message naming the argument: width or height < 1; levels outside 1..7; radius
 * outside 1..4; window outside 0..4; median or subpixel not 0 / 1; fb_max_diff < -1; a null pointer.  VDO_ERR_UNSUPPORTED when
 * width * height > 2^26.  VDO_ERR_OOM when the device has no room. */
int vdo_optflow_create(vdo_ctx* ctx, int width, int height, const vdo_optflow_params* params, vdo_optflow** out);
int vdo_optflow_destroy(vdo_optflow* h);
/* One pair, host-synchronous, on the context's stream.  im0 / im1: rows of `width` bytes, stride* bytes apart (>= width); host pointers, or device
 * pointers when src_is_device != 0.  flow: width x height x 2 floats, packed; valid: width x height bytes (1 = valid), packed, may be NULL; both
 * device pointers when out_is_device != 0; n_valid: host.  VDO_ERR_INVALID, the message naming the argument, for a null image, flow or count and
 * a stride < width - and then NOTHING is written.  No state of an earlier compute on the handle enters the result. */
int vdo_optflow_compute(vdo_optflow* h, const uint8_t* im0, int64_t stride0, const uint8_t* im1, int64_t stride1, int src_is_device, float* flow,
                        uint8_t* valid, int out_is_device, int32_t* n_valid);
/* The size of pyramid level `level` (0 .. levels-1). */
int vdo_optflow_level_size(vdo_optflow* h, int level, int* width, int* height);
/* Inspection of the LAST compute (VDO_ERR_INVALID before the first), host outputs of the level's size: the pyramid level [H_l][W_l] and its census
 * image of I0 (which = 0) or I1 (1); the integer flow [H_l][W_l][2] of the forward (dir = 0) or backward (1; VDO_ERR_INVALID when fb_max_diff is -1)
 * run, as the level below reads it - after the median. */
int vdo_optflow_get_pyramid(vdo_optflow* h, int which, int level, uint8_t* out);
int vdo_optflow_get_census(vdo_optflow* h, int which, int level, uint64_t* out);
int vdo_optflow_get_level_flow(vdo_optflow* h, int dir, int level, int32_t* out);
/* The last compute: ms[0] wall time of the call, ms[1] device time from the first upload to the end of the check kernel (events). */
int vdo_optflow_last_timing(vdo_optflow* h, double ms[2]);
/* Device images owned by the handle, for callers without their own: the packed width x height images the pair is brought to (level 0 of the two
 * pyramids; uploading into them and passing them as a device pair is allowed), a flow image [H][W][2] and a validity image [H][W] to pass as
 * device outputs.  Any of the four may be NULL. */
int vdo_optflow_device_images(vdo_optflow* h, uint8_t** im0, uint8_t** im1, float** flow, uint8_t** valid);
/* Brings the frame's host mask (i32, width x height, packed) to a device image owned by the handle (made on the first call), for a caller that
 * computes the flow into the handle's device flow image and hands the whole frame to a device-input step (Tracking::GrabImageStereoPair).
 * Host-synchronous. */
int vdo_optflow_stage_mask(vdo_optflow* h, const int32_t* mask, int32_t** mask_dev);

/* ---- Instance labeller: connected components to the mask image ---------------------------------------------------------------------
 * New (the reference's TrackRGBD takes an instance mask per frame - int32, 0 = background, labels below 1024 - and leaves making it to an
 * offline instance-segmentation network): from a class image cls[H][W] (uint8, 0 = background; a semantic map without instances, or a drawn
 * region) and optionally a disparity image to mask[H][W] int32, the layout vdo_ingest_frame and FramePipeline::Step take; and the same engine as
 * the speckle filter a stereo matcher ends with.  Integer arithmetic in every stage; no result depends on workgroup shape or order.  Raster
 * index i = y * W + x.  A disparity v (fp32: the disparity256 image of vdo_stereo_compute, possibly scaled) enters as d = (int32)v (truncation)
 * when 0 <= v < 2^24, else (NaN, negative, too large) d = 0 = unknown.
 *
 * 1. Links.  Neighbour offsets (1,0), (0,1) at connectivity 4; also (1,1), (-1,1) at connectivity 8.
 *    Instance mode: p and q are linked iff cls(p) == cls(q) != 0 and (max_disp_diff == -1 or d(p) == 0 or d(q) == 0 or
 *    |d(p) - d(q)| <= max_disp_diff): an unknown disparity does not cut an object.
 *    Speckle mode (connectivity 4): p and q are linked iff d(p) != 0, d(q) != 0 and |d(p) - d(q)| <= max_diff; pixels with d == 0 belong to
 *    no component.
 * 2. Components: the transitive closure of the links.  A component's root is its smallest raster index, its area its pixel count.  Pixels of
 *    no component (background; d == 0 in speckle mode) have root -1.
 * 3. Selection (instance mode).  Let A be the smallest value >= min_area such that at most max_labels components have area >= A (components of
 *    equal area are kept or dropped together).  The reported threshold A* is min_area when nothing overflows (A == min_area); otherwise the area
 *    of the smallest component of area >= A - the same components pass A and A* - or A itself when none does: areas 9, 9, 4, 4, 1 give A* = 9
 *    with max_labels 3 and A* = 4 with max_labels 4.  The components of area >= A* are numbered 1..n_labels in
 *    ascending order of their roots; mask(p) = the number of p's component, or 0.  The per-frame numbers carry no identity over time: the tracker
 *    associates objects through the flow.
 * 4. Speckle filter, in place on an fp32 disparity image: every pixel of a component with area <= max_size becomes 0.0f, every other value stays
 *    bit for bit; *n_removed = the number of pixels zeroed. */
typedef struct vdo_labels vdo_labels;
typedef struct vdo_labels_params {
  int32_t connectivity;             /* 4 or 8 */
  int32_t max_disp_diff;            /* >= -1, in the units of the disparity image; -1 switches the disparity gate off */
  int32_t min_area;                 /* >= 1: smaller components get no label */
  int32_t max_labels;               /* 1..1023: labels stay below the frame step's 1024 vote bins */
} vdo_labels_params;
/* A labeller for width x height images.  ALL device memory is taken here (link bits, parent, area and rank per pixel, staged class, disparity and
 * mask images: about 22 bytes per pixel); computes and filters allocate nothing.  VDO_ERR_INVALID, the message naming the argument: width or
 * height < 1; connectivity not 4 or 8; max_disp_diff < -1; min_area < 1; max_labels outside 1..1023; a null pointer.  VDO_ERR_UNSUPPORTED when
 * width * height > 2^26.  VDO_ERR_OOM when the device has no room. */
int vdo_labels_create(vdo_ctx* ctx, int width, int height, const vdo_labels_params* params, vdo_labels** out);
int vdo_labels_destroy(vdo_labels* h);
/* One image, host-synchronous, on the context's stream.  cls: rows of `width` bytes, cls_stride bytes apart (>= width); disp: rows of `width`
 * floats, disp_stride_floats floats apart (>= width), NULL allowed only when max_disp_diff == -1 (then it is not read); host pointers, or device
 * pointers when src_is_device != 0 (packed device images are read where they are).  mask: width x height int32, packed, a device pointer when
 * out_is_device != 0.  out (host): n_labels, n_components (all components, kept or not), area_threshold = A*.  VDO_ERR_INVALID, the message naming
 * the argument, for a null cls, mask or out, a null disp with the gate on and a stride < width - and then NOTHING is written.  No state of an
 * earlier compute or filter on the handle enters the result.  VDO_ERR_INTERNAL should a walk of the union-find pass its step bound. */
int vdo_labels_compute(vdo_labels* h, const uint8_t* cls, int64_t cls_stride, const float* disp, int64_t disp_stride_floats, int src_is_device,
                       int32_t* mask, int out_is_device, int32_t out[3]);
/* Step 4 on a packed width x height fp32 image (a device pointer when is_device != 0), host-synchronous.  VDO_ERR_INVALID for max_diff < 0,
 * max_size < 0 or a null pointer, and then nothing is written.  The handle's connectivity and selection parameters play no part. */
int vdo_labels_filter_speckles(vdo_labels* h, float* disparity256, int is_device, int max_diff, int max_size, int32_t* n_removed);
/* Inspection of the LAST compute or filter (VDO_ERR_INVALID before the first), host outputs [H][W]: the root of every pixel or -1; the area at
 * each root and 0 elsewhere. */
int vdo_labels_get_roots(vdo_labels* h, int32_t* out);
int vdo_labels_get_areas(vdo_labels* h, int32_t* out);
/* The last compute or filter: ms[0] wall time of the call, ms[1] device time from the first upload to the end of the last kernel (events). */
int vdo_labels_last_timing(vdo_labels* h, double ms[2]);
/* Device images owned by the handle, for callers without their own: a packed class image to upload into and pass as a device source, and a mask
 * image to pass as a device output.  Either may be NULL. */
int vdo_labels_device_images(vdo_labels* h, uint8_t** cls, int32_t** mask);
/* Brings a host class image (rows cls_stride bytes apart) to the handle's device class image, for a caller whose disparity is already on the
 * device (src_is_device covers both sources of a compute): Tracking::GrabImageStereoPairSemantic.  Host-synchronous. */
int vdo_labels_stage_classes(vdo_labels* h, const uint8_t* cls, int64_t cls_stride, uint8_t** cls_dev);

/* ---- Stereo rectifier: lens undistortion and fixed-point remap ---------------------------------------------------------------------
 * New (the reference's stereo example starts with cv::initUndistortRectifyMap + cv::remap; its System takes images that are already
 * rectified): from the raw 8-bit images of one or two cameras to the rectified grey images the stereo and flow matchers take.  Two parts: a map,
 * computed once per camera on the host, and a remap, computed per image on the device.  The weights are the project's own (5 fractional bits,
 * not OpenCV's table): no bit equality with cv::remap is claimed.
 *
 * MAP, fp64, every operation rounded on its own and done in the order written (no contraction).  Raw camera K = (fx, fy, cx, cy),
 * D = (k1, k2, p1, p2, k3), rectifying rotation R (row-major; its transpose is used, nothing is inverted), rectified camera
 * P = (fx', fy', cx', cy'), source size Ws x Hs, destination size W x H.  For destination pixel (u, v):
 *     x = (u - cx') / fx';  y = (v - cy') / fy'
 *     X = (R00*x + R10*y) + R20;  Y = (R01*x + R11*y) + R21;  Wc = (R02*x + R12*y) + R22
 *     invalid unless Wc > 0;  xn = X / Wc;  yn = Y / Wc
 *     x2 = xn*xn; y2 = yn*yn; r2 = x2 + y2; xy2 = 2*(xn*yn)
 *     t = r2*k3; t = k2 + t; t = r2*t; t = k1 + t; t = r2*t; kr = 1 + t
 *     xd = (xn*kr + p1*xy2) + p2*(r2 + 2*x2)
 *     yd = (yn*kr + p1*(r2 + 2*y2)) + p2*xy2
 *     us = fx*xd + cx;  vs = fy*yd + cy
 *     qx = rint(32*us), qy = rint(32*vs)        (ties to even; invalid when not finite or |.| >= 2^30)
 *     ix = qx >> 5, ax = qx & 31, iy = qy >> 5, ay = qy & 31     (arithmetic shift)
 *     valid iff 0 <= ix, ix + (ax > 0) <= Ws - 1, 0 <= iy, iy + (ay > 0) <= Hs - 1
 * The stored map is int32 [H][W][2] = (qx, qy); an invalid pixel stores (INT32_MIN, INT32_MIN).  A uint8 validity image [H][W] (1 = valid) and
 * its count go with it.
 *
 * REMAP, integer arithmetic only, S the source image.  For a valid pixel the taps are p00 = S(ix, iy), p01 = S(ix+1, iy), p10 = S(ix, iy+1),
 * p11 = S(ix+1, iy+1); a tap with weight 0 is not read;
 *     out = ((32-ax)*(32-ay)*p00 + ax*(32-ay)*p01 + (32-ax)*ay*p10 + ax*ay*p11 + 512) >> 10.
 * An invalid pixel gets the `border` byte.  For a 3- or 4-channel source every tap is first made grey by the arithmetic of vdo_rgb2gray (K2:
 * (r*4899 + g*9617 + b*1868 + 8192) >> 14, r = byte 0 when rgb_order != 0, else byte 2), then interpolated: vdo_rgb2gray followed by a
 * one-channel remap.  In `nearest` mode (one channel only; for class images) out = S((qx + 16) >> 5, (qy + 16) >> 5) (the sum taken without
 * overflow), valid iff that tap lies inside the source.
 * NO OUT-OF-RANGE READS: the kernel re-derives validity from the stored (qx, qy) and the source size, in the remap's mode; it trusts no flag, so
 * whatever map it is handed it cannot read outside the source image. */
typedef struct vdo_rectify vdo_rectify;
typedef struct vdo_rectify_camera {
  double K[4];                      /* fx, fy, cx, cy of the raw camera; fx, fy > 0 */
  double D[5];                      /* k1, k2, p1, p2, k3 */
  double R[9];                      /* rectifying rotation, row-major */
  int32_t src_width, src_height;    /* Ws x Hs, >= 1 */
} vdo_rectify_camera;
typedef struct vdo_rectify_params {
  int32_t n_cams;                   /* 1 or 2 */
  int32_t width, height;            /* W x H of every destination image, >= 1 */
  double P[4];                      /* fx', fy', cx', cy' of the rectified camera; fx', fy' > 0 */
  vdo_rectify_camera cam[2];
} vdo_rectify_params;
typedef struct vdo_rectify_job {
  const uint8_t* src;               /* rows of Ws * channels bytes, src_stride bytes apart */
  int64_t src_stride;
  int32_t channels;                 /* 1, 3 or 4 */
  int32_t rgb_order;                /* as vdo_rgb2gray; ignored with one channel */
  int32_t cam;                      /* whose map and source size */
  int32_t nearest;                  /* != 0: nearest mode, one channel only */
  uint8_t* dst;                     /* rows of W bytes, dst_stride bytes apart */
  int64_t dst_stride;
} vdo_rectify_job;
/* The MAP above for camera `cam` of `params`: host only, it needs no device and no context (like vdo_ba_plan_create).  map: width x height x 2
 * int32; valid (width x height bytes) and n_valid may be NULL.  VDO_ERR_INVALID, the message naming the argument, and then nothing is written:
 * a null params or map; n_cams outside 1..2; cam outside 0..n_cams-1; a size < 1; fx, fy, fx' or fy' not finite or <= 0; any other parameter
 * not finite.  VDO_ERR_UNSUPPORTED when width * height or a source's width * height exceeds 2^26. */
int vdo_rectify_plan(const vdo_rectify_params* params, int cam, int32_t* map, uint8_t* valid, int32_t* n_valid);
/* A rectifier for params->n_cams cameras and one destination size.  ALL device memory is taken here (per camera the map, 8 bytes per destination
 * pixel, and the validity image; staging for 4 source images of 4 channels of the largest source; 4 destination images; one float image for a
 * host image of vdo_rectify_gate); vdo_rectify_compute and vdo_rectify_gate allocate nothing.  Refusals as vdo_rectify_plan, and a null ctx or
 * out.  VDO_ERR_OOM when the device has no room. */
int vdo_rectify_create(vdo_ctx* ctx, const vdo_rectify_params* params, vdo_rectify** out);
/* The same from ready-made maps - the door for every lens model the planner leaves out (fisheye, a look-up calibration): maps[c] is
 * width x height x 2 int32 = (qx, qy) for a source of src_width[c] x src_height[c]; any values are legal (NO OUT-OF-RANGE READS above).  The
 * validity images are re-derived from the maps in bilinear mode. */
int vdo_rectify_create_from_maps(vdo_ctx* ctx, int width, int height, int n_cams, const int32_t* const* maps, const int32_t* src_width,
                                 const int32_t* src_height, vdo_rectify** out);
int vdo_rectify_destroy(vdo_rectify* h);
/* n_jobs = 1..4 remaps in ONE kernel launch, host-synchronous, on the context's stream.  Every src is a host pointer, or a device pointer when
 * src_is_device != 0 (read where it lies, at its stride); every dst likewise with dst_is_device (written where it lies; any alignment).  Two
 * jobs may share a map or a source; destinations must not overlap.  VDO_ERR_INVALID, the message naming the argument, for a null handle, jobs,
 * src or dst; n_jobs outside 1..4; cam outside the handle's cameras; channels not 1, 3 or 4; nearest with more than one channel;
 * src_stride < Ws * channels; dst_stride < W; border outside 0..255 - and then NOTHING is written.  No state of an earlier compute on the handle enters the result. */
int vdo_rectify_compute(vdo_rectify* h, const vdo_rectify_job* jobs, int n_jobs, int src_is_device, int dst_is_device, int border);
/* Writes 0.0f wherever cam's (bilinear) validity is 0 and leaves every other value bit for bit: a disparity made from border filler becomes "no
 * depth".  image: width x height floats, rows stride_floats apart (>= width), a device pointer when is_device != 0.  *n_cleared = the number of
 * values whose bits changed (an invalid pixel that already held +0.0f is not counted).  Host-synchronous.  VDO_ERR_INVALID for a null pointer, a
 * cam out of range or a stride < width, and then nothing is written. */
int vdo_rectify_gate(vdo_rectify* h, int cam, float* image, int64_t stride_floats, int is_device, int32_t* n_cleared);
/* Host outputs: cam's map [H][W][2]; its validity image [H][W] and count (either may be NULL). */
int vdo_rectify_get_map(vdo_rectify* h, int cam, int32_t* map);
int vdo_rectify_get_valid(vdo_rectify* h, int cam, uint8_t* valid, int32_t* n_valid);
/* The last compute or gate: ms[0] wall time of the call, ms[1] device time from the first upload to the end of the kernel (events). */
int vdo_rectify_last_timing(vdo_rectify* h, double ms[2]);
/* Device images owned by the handle, for callers without their own, k = 0..3: the staging image a host source of job k is uploaded to (room for
 * 4 channels of the largest source; uploading into it and passing it as a device source is allowed) and a packed width x height destination
 * image.  Either may be NULL. */
int vdo_rectify_device_images(vdo_rectify* h, int k, uint8_t** src, uint8_t** dst);
/* Brings a width x height destination image that lies on the device (rows stride bytes apart; e.g. the stereo matcher's left staging image a
 * device-destination job wrote) to the host, packed: for a caller that wants to look at a rectified image.  Host-synchronous. */
int vdo_rectify_download_image(vdo_rectify* h, const uint8_t* image_dev, int64_t stride, uint8_t* out);

/* ---- Motion segmenter: moving pixels from disparity and flow -----------------------------------------------------------------------
 * New (the reference takes the class of every pixel from an offline segmentation network and then tracks only what moves: bObjStat, fSFMgThres /
 * fSFDsThres): from the disparity of frame t, the disparity of frame t + 1, the flow between them and the camera motion to the class image
 * cls[H][W] (uint8) vdo_labels_compute takes - class_value where the pixel moves against the scene, else 0.  Three stages; stage 1 is fp32, one
 * rounded operation per step in the order written, no contraction (/ and floorf correctly rounded); stage 2 is integer; no result depends on
 * workgroup shape or order.  disp0, disp1: fp32 in depth-image units, disparity x disp_unit (the disparity256 image of vdo_stereo_compute with
 * its output scale).  flow[H][W][2] from t to t + 1; flow_valid[H][W] (vdo_optflow_compute's `valid`) or NULL.  T: 4 x 4 row-major, camera
 * t + 1 from camera t; its last row is not read.  K = (fx, fy, cx, cy).
 *
 * 1. Residual, per pixel (x, y), xf = (float)x, yf = (float)y, (fu, fv) = flow(y, x):
 *      d0 = disp0(y, x) / unit;  uo = xf + fu;  vo = yf + fv;  xq = floorf(uo + 0.5f);  yq = floorf(vo + 0.5f)
 *    The pixel is UNKNOWN (state 2, residual -1.0f) unless all of: d0 finite and d0 >= max(min_disparity, FLT_MIN); uo and vo finite;
 *    0 <= xq <= (float)(W - 1) and 0 <= yq <= (float)(H - 1), compared as floats before any conversion to int (a NaN fails); flow_valid NULL or
 *    non-zero at (y, x); d1 = disp1((int)yq, (int)xq) / unit finite and > 0; Z' > 0; e finite - with
 *      Z = bf / d0;  X = ((xf - cx) * Z) / fx;  Y = ((yf - cy) * Z) / fy
 *      X' = (T0*X + T1*Y) + (T2*Z + T3);  Y' = (T4*X + T5*Y) + (T6*Z + T7);  Z' = (T8*X + T9*Y) + (T10*Z + T11)
 *      u' = (fx * X') / Z' + cx;  v' = (fy * Y') / Z' + cy;  d' = bf / Z'
 *      du = uo - u';  dv = vo - v';  dd = d1 - d'
 *      e = (du*du + dv*dv) * wf + (dd*dd) * wd,     wf = 1.0f / (sigma_flow * sigma_flow), wd = 1.0f / (sigma_disp * sigma_disp), fp32, made once
 *    A known pixel has residual e and state 1 (moving) iff e > chi2, else state 0.
 *    NO OUT-OF-RANGE READS: the one gathered address follows from the float compares above; no flag and no value is trusted.
 * 2. Vote.  m(p), s(p): the numbers of state-1 and state-0 pixels in the (2r + 1)^2 window around p clipped at the image.  p is moving iff
 *    m + s >= min_known and m * vote_den > vote_num * (m + s); cls(p) = class_value, else 0.  The pixel's own state has no special role: an
 *    unknown hole inside an object is filled.
 * 0. Ego-motion (vdo_motionseg_egomotion; a separate entry, so that the segmenter is a function of its inputs and T alone).  Grid positions
 *    x = step / 2 + i * step < W, y = step / 2 + j * step < H (integer division), in raster order.  A position is kept under stage 1's tests on
 *    d0, uo, vo, (xq, yq) and flow_valid (not on disp1).  Its sample is X3 = (X, Y, Z) of stage 1 widened to double and uv = (uo, vo) widened.
 *    The kept samples are compacted in order on the device and downloaded once; vdo_pnp_ransac runs on them with K widened, refit = 1 (AP3P, EPnP
 *    re-estimation) and the caller's max_iterations, threshold and confidence.  T = its result narrowed to float; with fewer than min_inliers
 *    inliers (or no model) T is the identity and the call still answers VDO_OK. */
typedef struct vdo_motionseg vdo_motionseg;
typedef struct vdo_motionseg_params {
  float K[4];                       /* fx, fy, cx, cy; fx, fy > 0 */
  float bf;                         /* baseline x fx, > 0 */
  float disp_unit;                  /* > 0: the disparity images hold disparity x disp_unit (DepthMapFactor) */
  float sigma_flow, sigma_disp;     /* > 0, px */
  float chi2;                       /* >= 0 */
  float min_disparity;              /* >= 0, px: a source pixel below it is unknown */
  int32_t vote_radius;              /* r: 0..7 */
  int32_t vote_num, vote_den;       /* 0 <= vote_num < vote_den <= 65535 */
  int32_t min_known;                /* >= 1 */
  int32_t class_value;              /* 1..255 */
} vdo_motionseg_params;
/* A segmenter for width x height images.  ALL device memory is taken here (state, residual and class image; disp1 and one uint8 image for the
 * next-right picture of a rectified frame; staging for disp0, flow and flow_valid; the sample lists at the capacity of step 1, 40 bytes per
 * pixel, with a pinned mirror; counters: about 71 bytes per pixel); the other entries allocate nothing.  VDO_ERR_INVALID, the message naming
 * the argument: a null pointer; width or height < 1; a parameter outside the range written beside it or not finite.  VDO_ERR_UNSUPPORTED when
 * width * height > 2^26 or a side exceeds 2^24.  VDO_ERR_OOM when the device has no room. */
int vdo_motionseg_create(vdo_ctx* ctx, int width, int height, const vdo_motionseg_params* params, vdo_motionseg** out);
int vdo_motionseg_destroy(vdo_motionseg* h);
/* Stage 0, host-synchronous, on the context's stream.  disp0: rows of `width` floats, disp0_stride_floats apart (>= width); flow: rows of
 * 2 * width floats, flow_stride_floats apart (>= 2 * width); flow_valid: NULL or rows of `width` bytes, flow_valid_stride apart (>= width); host
 * pointers, or device pointers when src_is_device != 0 (packed device images are read where they lie - the flow if it is 8-byte aligned -
 * anything else goes through the handle's staging images).  T (host, 16 floats); out (host): n_samples, n_inliers, iterations_run.
 * VDO_ERR_INVALID, the message naming the argument, and then NOTHING is written: a null handle, disp0, flow, T or out; a stride too small;
 * step < 1; max_iterations < 0; reproj_threshold not positive and finite; confidence outside (0, 1); min_inliers < 0.  A step beyond the image
 * leaves no samples: the identity. */
int vdo_motionseg_egomotion(vdo_motionseg* h, const float* disp0, int64_t disp0_stride_floats, const float* flow, int64_t flow_stride_floats,
                            const uint8_t* flow_valid, int64_t flow_valid_stride, int src_is_device, int step, int max_iterations,
                            double reproj_threshold, double confidence, int min_inliers, float T[16], int32_t out[3]);
/* Stages 1 and 2, host-synchronous, on the context's stream: two kernels.  Sources as above, disp1 like disp0.  T: host.  cls: width x height
 * bytes, packed, a device pointer when out_is_device != 0.  out (host): moving pixels after the vote, state-0 pixels, state-2 pixels.
 * VDO_ERR_INVALID, the message naming the argument, for a null handle, disp0, disp1, flow, T, cls or out and a stride too small - and then
 * NOTHING is written.  No state of an earlier call on the handle enters the result. */
int vdo_motionseg_compute(vdo_motionseg* h, const float* disp0, int64_t disp0_stride_floats, const float* disp1, int64_t disp1_stride_floats,
                          const float* flow, int64_t flow_stride_floats, const uint8_t* flow_valid, int64_t flow_valid_stride, int src_is_device,
                          const float T[16], uint8_t* cls, int out_is_device, int32_t out[3]);
/* Inspection of the LAST compute (VDO_ERR_INVALID before the first), host outputs [H][W]: the state bytes; the residuals. */
int vdo_motionseg_get_state(vdo_motionseg* h, uint8_t* out);
int vdo_motionseg_get_residual(vdo_motionseg* h, float* out);
/* The sample lists of the LAST ego-motion (VDO_ERR_INVALID before the first): *n = n_samples; X3 ([n][3]) and uv ([n][2]), host, may be NULL
 * (a caller that sizes them asks for n first; n <= width * height always). */
int vdo_motionseg_get_samples(vdo_motionseg* h, double* X3, double* uv, int32_t* n);
/* The last compute or ego-motion: ms[0] wall time of the call, ms[1] device time from the first upload to the end of the last kernel (events). */
int vdo_motionseg_last_timing(vdo_motionseg* h, double ms[2]);
/* Device images owned by the handle, for callers without their own: a packed float image for the next pair's disparity (pass it as a matcher's
 * device output, then as a device disp1), a packed uint8 image for the next-right picture, and a class image to pass as a device output.  Any
 * of the three may be NULL. */
int vdo_motionseg_device_images(vdo_motionseg* h, float** disp1, uint8_t** next_right, uint8_t** cls);

/* ---- Dense mapper: TSDF fusion of the static scene ---------------------------------------------------------------------------------
 * New (the reference keeps no dense map): a truncated-signed-distance voxel volume on the device, world-aligned, cyclically addressed, following
 * the camera; every frame's metric depth is fused into it projectively with the frame's pose, pixels with a non-zero instance mask left out;
 * surface points are extracted in a fixed order.  The geometry is fp32, one rounded operation per step in the order written, no contraction
 * (/ and floorf correctly rounded); the fusion and everything after it is integer; no result depends on workgroup shape, on the voxels a thread
 * takes or on the schedule.
 *
 * Volume.  n = (nx, ny, nz) voxels of edge `voxel`; the integer origin o, in global voxel units: the volume stands for the global voxels
 *   o_a <= g_a < o_a + n_a, every |g| in use below 2^22 (so (float)g + 0.5f is exact).  Voxel g lives at slot (g_a mod n_a) per axis (the
 *   mathematical, non-negative mod), slots laid out x fastest, then y, then z.  One 32-bit word per voxel: the low 16 bits the TSDF t as int16,
 *   -32767..32767, the high 16 bits the weight w; w = 0 is "never seen" and the whole word is then 0.  The centre of g: p_a = ((float)g_a + 0.5f) * voxel.
 * Integrate.  depth[H][W] fp32 metres; mask[H][W] int32 or NULL; T 4 x 4 row-major, world -> camera (mTcw), last row not read; K = (fx, fy, cx, cy).
 *   Every voxel of the volume, from its own integer index:
 *      Xc = (T0*px + T1*py) + (T2*pz + T3);  Yc = (T4*px + T5*py) + (T6*pz + T7);  Zc = (T8*px + T9*py) + (T10*pz + T11)
 *      skip unless Zc finite and Zc > max(min_depth, FLT_MIN)
 *      u = (fx*Xc)/Zc + cx;  v = (fy*Yc)/Zc + cy;  xq = floorf(u + 0.5f);  yq = floorf(v + 0.5f)
 *      skip unless u, v finite and 0 <= xq <= (float)(W-1) and 0 <= yq <= (float)(H-1), compared as floats before any conversion to int (a NaN fails)
 *      d = depth((int)yq, (int)xq);  skip unless d finite, d > min_depth, d <= max_depth
 *      skip (counted as masked) if mask != NULL and mask((int)yq, (int)xq) != 0
 *      s = d - Zc;  skip (counted as occluded) if s < -trunc;  s = fminf(s, trunc)
 *      q = (int)floorf((s / trunc) * 32767.0f + 0.5f)
 *      t' = floor_div(2*(t*w + q) + (w+1), 2*(w+1))  (floor towards -inf; below 2^25 in magnitude);   w' = min(w+1, max_weight)
 *   A skipped voxel keeps its word bit for bit.  NO OUT-OF-RANGE READS: the one gathered address follows from the float compares alone.
 * Recenter.  The slots whose global voxel changes are set to 0, every other word is untouched; a shift of >= n_a on any axis clears everything, a
 *   shift of 0 nothing; only the leaving slabs are written.
 * Extract.  A box [lo, hi) in global voxels, clipped to the volume; min_weight >= 1.  The voxels a of the box in the order z, y, x (x fastest),
 *   axes 0, 1, 2 within a voxel: the neighbour b = a + e_axis must be inside the VOLUME (not the box), both weights >= min_weight; a crossing iff
 *   (ta < 0) != (tb < 0); frac = (float)ta / (float)(ta - tb); the coordinate on the axis (((float)g_a + 0.5f) + frac) * voxel, the other two the
 *   centre's.  Per point: xyz float[3]; grad int32[3] = t(a+e_k) - t(a), k = 0..2, if all three neighbours are inside the volume with
 *   w >= min_weight, else (0, 0, 0) - unnormalised, so that no sqrt enters the parity; weight int32, the smaller of the two weights.  The points are
 *   compacted in the visiting order; the call returns the total count and writes exactly the first min(capacity, count) points. */
typedef struct vdo_dense vdo_dense;
typedef struct vdo_dense_params {
  int32_t n[3];                     /* 1..4096 each, nx * ny * nz <= 2^31 */
  float voxel;                      /* > 0, metres */
  int32_t origin[3];                /* global voxels; -2^22 < origin_a and origin_a + n_a <= 2^22 */
  float K[4];                       /* fx, fy, cx, cy; fx, fy > 0 */
  float trunc;                      /* > 0, metres */
  float min_depth, max_depth;       /* 0 <= min_depth < max_depth, metres */
  int32_t max_weight;               /* 1..255 */
  int32_t stage_points;             /* >= 1: the points one window of a host-output extraction holds on the device (28 bytes each) */
} vdo_dense_params;
/* A mapper for width x height depth and mask images.  ALL device memory is taken here (the volume, 4 bytes per voxel, cleared; the compaction
 * offsets, 8 bytes per 256 voxels; the counters; staging for a host or strided depth and mask, 8 bytes per pixel; the point staging); the other
 * entries allocate nothing.  VDO_ERR_INVALID, the message naming the argument: a null pointer; a size < 1; a parameter outside the range written
 * beside it or not finite; an origin out of range.  VDO_ERR_UNSUPPORTED when nx * ny * nz > 2^31 or a side exceeds 2^12 (or the image exceeds
 * 2^26 pixels or 2^24 on a side).  VDO_ERR_OOM when the device has no room. */
int vdo_dense_create(vdo_ctx* ctx, int width, int height, const vdo_dense_params* params, vdo_dense** out);
int vdo_dense_destroy(vdo_dense* h);
/* One frame, host-synchronous, on the context's stream: one kernel.  depth: rows of `width` floats, depth_stride_floats apart (>= width); mask:
 * NULL or rows of `width` int32, mask_stride_ints apart (>= width); host pointers, or device pointers when src_is_device != 0 (packed device images
 * are read where they lie, anything else goes through the handle's staging images).  T: host.  out (host): updated voxels, voxels skipped by the
 * mask, voxels skipped as occluded.  VDO_ERR_INVALID, the message naming the argument, and then NOTHING is written: a null handle, depth, T or
 * out; a stride too small. */
int vdo_dense_integrate(vdo_dense* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device,
                        const float T[16], int64_t out[3]);
/* The same from the resident depth (after K1: metres) and mask of a vdo_frame_images of the mapper's size, read where they lie and not written. */
int vdo_dense_integrate_frame(vdo_dense* h, const vdo_frame_images* frame, const float T[16], int64_t out[3]);
/* Moves the volume to new_origin (host, global voxels).  VDO_ERR_INVALID for a null pointer or an origin out of range, and then nothing changes. */
int vdo_dense_recenter(vdo_dense* h, const int32_t new_origin[3]);
/* Surface points of the box [lo, hi) (host, global voxels; an empty or outside box has no points).  xyz [capacity][3], grad [capacity][3],
 * weight [capacity]: host pointers, or device pointers when out_is_device != 0; all three may be NULL when capacity is 0.  *count (host): the
 * total, whatever the capacity.  VDO_ERR_INVALID, the message naming the argument, and then NOTHING is written: a null handle, lo, hi or count;
 * min_weight < 1; capacity < 0; a null output with capacity > 0. */
int vdo_dense_extract(vdo_dense* h, const int32_t lo[3], const int32_t hi[3], int min_weight, int64_t capacity, float* xyz, int32_t* grad, int32_t* weight,
                      int out_is_device, int64_t* count);
/* Inspection: the words in slot order (host, nx * ny * nz; may be NULL) and the origin (host; may be NULL; not both). */
int vdo_dense_get_volume(vdo_dense* h, uint32_t* words, int32_t origin[3]);
/* The reverse: nx * ny * nz host words in slot order replace the volume (a saved volume; the origin is not changed).  The caller keeps the
 * format: w = 0 only with the whole word 0, w <= 255, t not -32768. */
int vdo_dense_set_volume(vdo_dense* h, const uint32_t* words);
/* The last integrate, recenter or extract: ms[0] wall time of the call, ms[1] device time from the first upload to the end of the last kernel. */
int vdo_dense_last_timing(vdo_dense* h, double ms[2]);
/* The volume where it lives (a device pointer owned by the handle). */
int vdo_dense_device_volume(vdo_dense* h, uint32_t** words);
/* The voxels along y one thread of the integrate kernel takes: 1, 2, 4 (the default) or 8.  No result depends on it. */
int vdo_dense_set_voxels_per_thread(vdo_dense* h, int voxels);
/* Sets every word of the volume to 0 on the context's stream (host-synchronous) and leaves the origin alone: a retired handle is reused. */
int vdo_dense_clear(vdo_dense* h);

/* ---- Mesher: surface-nets triangles from a TSDF volume --------------------------------------------------------------------------------------
 * New (the reference keeps no dense map): connected triangles from a vdo_dense - the static map or an object's volume -, in one-to-one relation with
 * what Extract finds: one quad (two triangles) per sign-changing lattice edge, one vertex per cell at the mean of the cell's edge crossings.  No case
 * table.  A vertex is fp32, one rounded operation per step in the order written, no contraction; everything else is integer.  The map is read only.
 * Notation as above: the volume covers the global voxels o_a <= g_a < o_a + n_a, words t (int16) and w; a voxel is NEGATIVE iff t < 0 (t = 0 is
 * positive).
 *
 * Cell.  Cell c has the 8 corner voxels c + {0,1}^3.  It is VALID iff all 8 corners are inside the VOLUME with w >= min_weight, ACTIVE iff it is
 *   valid and its corners are not all of one sign.
 * Vertex of an active cell.  Its 12 edges in this order: axis k = 0, 1, 2 with i = (k+1) % 3, j = (k+2) % 3; within an axis the lower corner offset
 *   d_j = 0, 1 (outer), d_i = 0, 1 (inner).  Edge (a, b = a + e_k) crosses iff (ta < 0) != (tb < 0); then frac = (float)ta / (float)(ta - tb) (what
 *   Extract computes) and the local point p is the corner offset as floats with (float)d_k + frac on axis k (d_k is 0).  s_c += p_c per coordinate
 *   from 0.0f, in visiting order, crossing edges only; m their number (>= 3).  mean_c = s_c / (float)m; the coordinate
 *   (((float)g_c + 0.5f) + mean_c) * voxel with g the cell's lower corner.
 *   Per vertex also grad int32[3]: grad_k = the sum over the cell's four axis-k edges of t(b) - t(a), unnormalised, towards free space; weight
 *   int32: the smallest of the 8 corner weights.
 * Quad of a lattice edge (a, k) with a sign change: it uses the four cells a - d_i*e_i - d_j*e_j, which must ALL be valid (so their lower corners are
 *   >= o, and both ends of the edge have w >= min_weight).  Vertex order (d_i, d_j) = (1,1), (0,1), (0,0), (1,0) when ta < 0, reversed when ta >= 0;
 *   the triangles (v0, v1, v2) and (v0, v2, v3): counter-clockwise seen from free space.  The quad's CORNER BLOCK is the 3 x 3 x 2 corners its four
 *   cells touch: a_i - 1 .. a_i + 1, a_j - 1 .. a_j + 1, a_k .. a_k + 1.
 * Box and mode.  lo, hi: global voxels, clipped to the volume, as Extract takes them.  outside == 0: the quads whose corner block lies inside the
 *   box and the vertices of the active cells whose 8 corners lie inside the box.  outside != 0: the quads of the volume whose corner block does NOT
 *   lie inside the box, and the vertices of the active cells whose corners do not all lie inside the box shrunk by one voxel on every side - every
 *   cell an outside quad uses is among them.  An empty box with outside set is the whole volume.  For any box the two modes partition the quads of
 *   the whole volume exactly: a caller that meshes what STAYS with outside != 0 before a recentre and the whole volume at the end loses no quad at
 *   a seam and doubles none.
 * Order.  Vertices in the order z, y, x of the cell's lower corner (x fastest), numbered from 0 among the emitted ones; quads in the order z, y, x
 *   of a, then k = 0, 1, 2; triangle indices int32 into that numbering.  A vertex need not be referenced by any triangle.
 * No result depends on launch shape, schedule or the slot alignment of the cyclic volume. */
typedef struct vdo_mesh vdo_mesh;
typedef struct vdo_mesh_params {
  int32_t n[3];                     /* 1..4096 each, nx * ny * nz <= 2^31: the mesher serves every map with no more voxels than that product */
  int32_t stage_vertices;           /* >= 1: the vertices one window of a host output holds on the device (28 bytes each) */
  int32_t stage_triangles;          /* >= 1: the triangles one window of a host output holds on the device (12 bytes each) */
} vdo_mesh_params;
/* ALL device memory is taken here (2 bits per cell, 16 bytes per 256 cells, the two staging windows); the other entries allocate nothing.  One mesher
 * serves any vdo_dense of the same context whose nx * ny * nz fits: the static map and all object volumes can share one.  VDO_ERR_INVALID, the
 * message naming the argument: a null pointer, a size or a window < 1.  VDO_ERR_UNSUPPORTED beyond the dense mapper's limits (a side above 2^12,
 * more than 2^31 voxels).  VDO_ERR_OOM when the device has no room. */
int vdo_mesh_create(vdo_ctx* ctx, const vdo_mesh_params* params, vdo_mesh** out);
int vdo_mesh_destroy(vdo_mesh* h);
/* The mesh of `map` for the box and mode, host-synchronous on the context's stream.  xyz [vertex_capacity][3], grad [vertex_capacity][3], weight
 * [vertex_capacity], tri [triangle_capacity][3]: host pointers, or device pointers when out_is_device != 0 (a host output of any size goes through
 * the staging windows); an output may be NULL when its capacity is 0.  counts (host): the total vertices and triangles, whatever the capacities;
 * exactly the first min(capacity, count) of each are written, and indices always refer to the full numbering.  VDO_ERR_INVALID, the message naming
 * the argument, and then NOTHING is written: a null handle, map, lo, hi or counts; min_weight < 1; a negative capacity; a null output with
 * capacity > 0; a map of another context; a map with more voxels than the mesher.  VDO_ERR_UNSUPPORTED, nothing written, if a count would pass
 * 2^31 - 1. */
int vdo_mesh_extract(vdo_mesh* h, vdo_dense* map, const int32_t lo[3], const int32_t hi[3], int outside, int min_weight, int64_t vertex_capacity,
                     float* xyz, int32_t* grad, int32_t* weight, int64_t triangle_capacity, int32_t* tri, int out_is_device, int64_t counts[2]);
/* The last extract: ms[0] wall time of the call, ms[1] device time from the first kernel to the end of the last; 0, 0 after an extract that was
 * refused with VDO_ERR_UNSUPPORTED or failed on the device (one refused with VDO_ERR_INVALID leaves the times of the call before it). */
int vdo_mesh_last_timing(vdo_mesh* h, double ms[2]);

/* ---- Object mapper: label statistics and a batched, label-selecting TSDF fusion -----------------------------------------------------------
 * New: the per-frame device stage of a volume per tracked object.  An object's volume is a plain vdo_dense in a frame of the object's own
 * (vdo_dense_extract, vdo_raycast_* and vdo_align_* work on it unchanged with T = Tcw * Two); a vdo_objects handle owns the label table, the
 * counters, the batch table and the image staging, and NO volume.  fp32 with one rounded operation per step in the order written, no contraction;
 * everything accumulated is an integer, so no result depends on workgroup shape, on the schedule or on the culling.
 *
 * Stats.  depth[H][W] fp32 metres, mask[H][W] int32 (required), K = (fx, fy, cx, cy).  A pixel (x, y) COUNTS when its depth d is finite with
 *   min_depth < d <= max_depth and its mask value l lies in 1..max_labels.  Row l of the table, int64[8]:
 *      [0] the number of counting pixels;  [1..4] their inclusive box x0, y0, x1, y1;  [5..7] the sums over them of
 *      qx = (int64) floorf(((((float)x - cx) * d) / fx) * 1024.f + 0.5f)
 *      qy = (int64) floorf(((((float)y - cy) * d) / fy) * 1024.f + 0.5f)
 *      qz = (int64) floorf(d * 1024.f + 0.5f)                                   (the back-projected point in 2^-10 m)
 *   A label without a counting pixel: (0, width, height, -1, -1, 0, 0, 0).  Row 0: [0] the pixels of usable depth whose label is non-zero and
 *   outside 1..max_labels (negative labels among them), the rest as for an empty label.  The table has max_labels + 1 rows.
 *   Accumulation: 64-bit integer atomics on global memory (add, min, max), after the lanes of a wave that carry the same label were combined in
 *   registers - any order gives the same table.
 *   BOUND.  With m = max(width + |cx|, height + |cy|) and term = max(m / min(fx, fy), 1) * max_depth * 1024 + 1, no |q| exceeds term (to rounding),
 *   and vdo_objects_create refuses parameters with width * height * term > 2^62: no sum leaves int64, no q the range of the conversion.
 * Integrate.  n objects: maps[i] (a vdo_dense of the same context and image size whose depth range lies inside the stage's), labels[i] in
 *   1..max_labels, T[i] 4 x 4 row-major, object frame -> camera (Tcw * Two), last row not read.  One call = the stats pass on its images, then ONE
 *   fusion launch over all n volumes: a device table holds per object the map's own kernel arguments (size, origin, voxel, K, truncation, depth
 *   range, weight cap), its volume, its label and the label's pixel box; the object index rides on the grid's x, the grid is sized for the largest
 *   volume, threads outside an object's own volume do nothing.  Per voxel everything is vdo_dense_integrate's (the same device functions), with
 *   one difference: after `d usable`, the voxel is left alone unless mask((int)yq, (int)xq) == labels[i].  The volume and the first two counts
 *   equal vdo_dense_integrate on the map with the mask image (mask != labels[i]).
 *   out[i] = updated voxels, occluded voxels, row labels[i] [0] of the stats.
 * Culling (vdo_objects_set_cull; off by default - profiles/objects_timing.txt: it did not pay at 8 objects of 96 x 64 x 96): an object whose label counts 0 pixels gets no workgroup; a voxel whose (xq, yq) lies outside
 *   the label's box is dropped before any image read.  Every pixel with mask == label and a depth the map accepts is inside that box (the map's
 *   depth range lies inside the stage's), so NO volume word and NO count depends on the switch.
 * NO OUT-OF-RANGE ACCESS: the gathered address follows from float compares against 0 and W - 1 / H - 1 made before any conversion to int; every
 *   volume index is built from slot coordinates tested against the object's own n; a stats row is addressed by a label tested against
 *   1..max_labels. */
typedef struct vdo_objects vdo_objects;
typedef struct vdo_objects_params {
  float K[4];                       /* fx, fy, cx, cy; fx, fy > 0 */
  float min_depth, max_depth;       /* 0 <= min_depth < max_depth, metres */
  int32_t max_labels;               /* 1..1023 */
  int32_t max_batch;                /* 1..64 objects per integrate call */
} vdo_objects_params;
/* ALL device memory is taken here.  VDO_ERR_INVALID, the message naming the argument: a null pointer, a size < 1, a parameter outside its range
 * or not finite.  VDO_ERR_UNSUPPORTED: the BOUND above, or an image beyond 2^26 pixels or 2^24 on a side. */
int vdo_objects_create(vdo_ctx* ctx, int width, int height, const vdo_objects_params* params, vdo_objects** out);
int vdo_objects_destroy(vdo_objects* h);
/* The stats of one frame, host-synchronous.  Images, strides and src_is_device as vdo_dense_integrate takes them, the mask required.
 * stats (host, [(max_labels + 1)][8]) may be NULL (read it later with vdo_objects_last_stats).  VDO_ERR_INVALID and nothing written: a null
 * handle, depth or mask; a stride too small. */
int vdo_objects_stats(vdo_objects* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device,
                      int64_t* stats);
int vdo_objects_stats_frame(vdo_objects* h, const vdo_frame_images* frame, int64_t* stats);
/* Stats, then the batched fusion, host-synchronous.  maps, labels, T ([n][16]) and out ([n][3]) are host arrays; n == 0 refreshes the stats only
 * (the arrays may then be NULL).  VDO_ERR_INVALID, the message naming the argument, and then NO volume and no stats change: n < 0 or n > max_batch;
 * a null array or a null maps[i]; the same map twice; a map of another context, another image size or a depth range outside the stage's;
 * labels[i] < 1 or > max_labels; a null depth or mask; a stride too small. */
int vdo_objects_integrate(vdo_objects* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device,
                          int n, vdo_dense* const* maps, const int32_t* labels, const float* T, int64_t* out);
int vdo_objects_integrate_frame(vdo_objects* h, const vdo_frame_images* frame, int n, vdo_dense* const* maps, const int32_t* labels, const float* T,
                                int64_t* out);
/* The A/B switch of the culling (default 0).  No result depends on it. */
int vdo_objects_set_cull(vdo_objects* h, int on);
/* The table of the last stats or integrate call (host, [(max_labels + 1)][8]); VDO_ERR_INVALID before the first. */
int vdo_objects_last_stats(vdo_objects* h, int64_t* stats);
/* The last stats or integrate call: ms[0] wall time of the call, ms[1] device time from the first upload to the end of the last kernel. */
int vdo_objects_last_timing(vdo_objects* h, double ms[2]);

/* ---- Raycaster: depth and normal views of the TSDF volume ---------------------------------------------------------------------------
 * New (the reference keeps no dense map): what the dense mapper's volume predicts a camera at pose T would see - per pixel a depth, an
 * unnormalised surface gradient and a weight, from a march along the pixel's ray through the cyclic volume with trilinear sampling.  A raycaster
 * is a VIEW onto one vdo_dense with an image size and intrinsics of its own (a viewer window need not have the frame's size).  It BORROWS the map:
 * the caller destroys every view before the map.  All arithmetic is fp32, one rounded operation per step in the order written, no contraction
 * (/ and floorf correctly rounded); every sample is computed from its integer k; no result depends on workgroup shape, on the schedule or on the
 * empty-space skipping.
 *
 * T is what vdo_dense_integrate takes: 4 x 4 row-major, world -> camera, last row not read; Tij below is row i, column j.
 * Camera centre, once per call, a = 0..2:   c_a = -((T0a*T03 + T1a*T13) + T2a*T23)
 * Ray of pixel (x, y):   dx = ((float)x - cx) / fx;  dy = ((float)y - cy) / fy;  r_a = (T0a*dx + T1a*dy) + T2a.  Its camera-z component is 1, so
 *   the parameter lambda is z-depth, comparable with a depth image.
 * Sample k = 0 .. n_steps-1 at lambda_k = near + (float)k * step (from the integer k, never accumulated).  Per axis:
 *      p_a = c_a + lambda_k * r_a;   g_a = p_a / voxel - 0.5f;   b_a = floorf(g_a);   f_a = g_a - b_a
 *   VALID iff (1) every g_a is finite and (float)o_a <= b_a && b_a <= (float)(o_a + n_a - 2), compared as floats before any conversion to int
 *   (a NaN fails), and (2) all eight corner words - the global voxels b + {0,1}^3, each at slot (g mod n) per axis - have weight >= min_weight.
 *   Value: with t the corners' int16 as float and lerp(u, v, f) = u + f*(v - u) (three operations): four lerps along x with f_0 (the pairs at
 *   (y, z) = (0,0), (1,0), (0,1), (1,1)), two along y with f_1, one along z with f_2 -> F_k, in TSDF units.
 * Hit: the first k >= 1 with samples k-1 and k both valid, F_{k-1} > 0 and F_k <= 0:
 *      depth = lambda_{k-1} + step * (F_{k-1} / (F_{k-1} - F_k)),   lambda_{k-1} from the integer k-1.
 *   Nothing else ends a ray: an invalid sample breaks the pair, a crossing from negative to positive is not a hit.
 * Outputs.  depth[H][W]: the hit depth, 0.0f without a hit.  weight[H][W] (int32): the smallest of the eight corner weights of sample k, 0 without
 *   a hit.  grad[H][W][3]: the hit point is sampled again (p_a = c_a + depth * r_a, then g, b, f as above); grad_a = S(b + e_a) - S(b - e_a), where
 *   S(b') is the same trilinear form at the base cell b' with the SAME fractions f ((float)b_a +- 1 is exact; a base cell is compared as floats
 *   against the same bounds).  If any of the six evaluations is invalid, or the hit point's own cell is, all three components are 0.0f.  The
 *   gradient is in the world frame, unnormalised (no sqrt enters the parity), and points into free space.
 * Counts.  out[0] rays that hit, out[1] rays with at least one valid sample and no hit, out[2] rays with no valid sample; they sum to W*H.
 * NO OUT-OF-RANGE READS: every gathered address follows from the float compares alone; a skipped or invalid sample reads nothing, or reads only
 *   inside the volume.
 * Empty-space skipping (on by default): every render first builds an occupancy grid over bricks of 8 x 8 x 8 SLOTS - a brick's flag is set iff
 *   any word of the brick, dilated by one slot towards +x, +y, +z cyclically, is non-zero: exactly the slots a sample with its base cell in the
 *   brick can touch - and a sample whose base brick is clear is invalid without touching the volume (all eight weights are 0 < min_weight).  The
 *   grid is rebuilt per call, since the volume is also writable through vdo_dense_device_volume.  NO result depends on it. */
typedef struct vdo_raycast vdo_raycast;
typedef struct vdo_raycast_params {
  float K[4];                       /* fx, fy, cx, cy; fx, fy > 0, all finite */
  float near;                       /* >= 0, finite: the z-depth of sample 0, metres */
  float step;                       /* > 0, finite: z-depth between samples, metres */
  int32_t n_steps;                  /* 1..65536 samples per ray ((float)k exact) */
  int32_t min_weight;               /* 1..255 */
} vdo_raycast_params;
/* A width x height view of `map`.  ALL the view's device memory is taken here (staging for host outputs, 20 bytes per pixel; the counters; the
 * occupancy grid, one byte per brick); the other entries allocate nothing.  VDO_ERR_INVALID, the message naming the argument: a null map, params
 * or out; a size < 1; a parameter outside the range written beside it or not finite.  VDO_ERR_UNSUPPORTED for an image over 2^26 pixels or 2^24
 * on a side.  VDO_ERR_OOM when the device has no room. */
int vdo_raycast_create(vdo_dense* map, int width, int height, const vdo_raycast_params* params, vdo_raycast** out);
int vdo_raycast_destroy(vdo_raycast* h);
/* One view, host-synchronous, on the map's context stream.  T: host.  depth [H][W], grad [H][W][3], weight [H][W]: host pointers, or device
 * pointers when out_is_device != 0; each may be NULL (it is then not produced).  out (host): the three counts.  VDO_ERR_INVALID, the message
 * naming the argument, and then NOTHING is written: a null handle, T or out.  A non-finite T is not refused: its rays have no valid sample. */
int vdo_raycast_render(vdo_raycast* h, const float T[16], float* depth, float* grad, int32_t* weight, int out_is_device, int64_t out[3]);
/* Empty-space skipping on (the default) or off.  NO result depends on it. */
int vdo_raycast_set_skip(vdo_raycast* h, int on);
/* The last render: ms[0] wall time of the call, ms[1] device time from the first command to the end of the last kernel (events). */
int vdo_raycast_last_timing(vdo_raycast* h, double ms[2]);
/* The part of ms[1] the last render spent building the occupancy grid (0 with skipping off). */
int vdo_raycast_grid_timing(vdo_raycast* h, double* ms);

/* ---- Aligner: point-to-plane ICP of a depth frame against a view of the map ---------------------------------------------------------
 * New (the reference has no dense pose estimator): projective data association of a measured depth frame against a MODEL - a depth and a gradient
 * image exactly as vdo_raycast_render writes them, with the pose Tm and the intrinsics Km they were rendered at -, point-to-plane residuals, their
 * normal equations summed over the image, and a Gauss-Newton refinement of the frame's pose.  All per-sample arithmetic is fp32, one rounded
 * operation per step in the order written, no contraction (/ and floorf correctly rounded); every gathered address is bounded by float compares
 * made before any conversion to int (a NaN fails them); the sums are in double in ONE fixed tree.  No result depends on workgroup shape, on the
 * launch shape or on the schedule; two runs give the same bits.
 *
 * Inputs.  depth D[H][W] fp32 metres; mask[H][W] int32 or NULL (a non-zero value skips the pixel, as the mapper does); K = (fx, fy, cx, cy);
 *   T, the current estimate: 4 x 4 row-major, world -> camera, last row not read, Tab below is row a, column b.  The model: Dm[Hm][Wm],
 *   Gm[Hm][Wm][3], Tm (as T), Km = (fxm, fym, cxm, cym); its size and intrinsics may differ from the frame's.
 * Samples.  subsample s (1..8): Ws = ceil(W/s), Hs = ceil(H/s); sample (i, j) is pixel (x, y) = (i*s, j*s).
 * Per sample:
 *      d = D(y,x);                 skip[no depth] unless d finite, d > max(min_depth, 0) and d <= max_depth
 *                                  skip[masked] if mask != NULL and mask(y,x) != 0
 *      dx = ((float)x - cx)/fx;  dy = ((float)y - cy)/fy;  Pc = (dx*d, dy*d, d)
 *      q_a = Pc_a - Ta3;           Pw_a = (T0a*q0 + T1a*q1) + T2a*q2                                      (a = 0..2)
 *      Xm = (Tm00*Pw0 + Tm01*Pw1) + (Tm02*Pw2 + Tm03);  Ym, Zm likewise with rows 1, 2 (the association of vdo_dense_integrate)
 *                                  skip[no model] unless Zm finite and Zm > FLT_MIN
 *      u = (fxm*Xm)/Zm + cxm;  v = (fym*Ym)/Zm + cym;  xq = floorf(u + 0.5f);  yq = floorf(v + 0.5f)
 *                                  skip[no model] unless u, v finite, 0 <= xq <= (float)(Wm-1), 0 <= yq <= (float)(Hm-1)
 *      dm = Dm(yq,xq);  g = Gm(yq,xq);  gg = (g0*g0 + g1*g1) + g2*g2
 *                                  skip[no model] unless dm finite and dm > 0, and gg finite and gg > 0
 *      the model point by the raycaster's own formulas: the camera centre c of Tm (once per call), the ray r of pixel (xq, yq) with Km,
 *      Vm_a = c_a + dm*r_a;        del_a = Pw_a - Vm_a;  dist2 = (del0*del0 + del1*del1) + del2*del2
 *                                  skip[far] unless dist2 <= max_dist*max_dist   (the product once, in fp32)
 *      e = (g0*del0 + g1*del1) + g2*del2;   w = 1.0f / gg          (no sqrt: w*e*e = (g.del)^2 / (g.g) is the squared point-to-plane distance)
 *      gc_a = (Ta0*g0 + Ta1*g1) + Ta2*g2                           (the gradient in the camera frame)
 *      J = (gc0, gc1, gc2,  Pc1*gc2 - Pc2*gc1,  Pc2*gc0 - Pc0*gc2,  Pc0*gc1 - Pc1*gc0);   h_i = w*J_i;   we = w*e
 *   The twist is taken about the camera, not the world origin: the system stays well conditioned hundreds of metres into a sequence.
 * Terms, in double and exact (each is a product of two floats), 28 per sample: the 21 upper-triangle A_ij = (double)h_i * (double)J_j, i <= j,
 *   row-major (A00 A01 .. A05 A11 .. A55); the 6 b_i = (double)h_i * (double)e; chi2 = (double)we * (double)e.  A skipped sample contributes +0.0.
 * The sum.  The sample grid is cut into 8 x 8 tiles, tiles_x = ceil(Ws/8), tiles_y = ceil(Hs/8); sample (i, j) has slot
 *   ((j/8)*tiles_x + i/8)*64 + (j%8)*8 + (i%8); slots with no sample hold +0.0; the slot vector is padded with +0.0 to the next power of two.
 *   Each of the 28 sums is the adjacent-pair tree over that vector in double, v[k] = v[2k] + v[2k+1], level by level, down to one value.  (On the
 *   device a wave's xor-butterfly over its tile is the first six levels, a tree over the tile partials the rest.)  No float atomics.
 * Counts, int64: used, no depth, masked, no model, far; they add up to Ws*Hs.
 * Step (vdo_align_step, pure host code, no device or context).  The symmetric A is rebuilt from the 21 sums and A xi = -b is solved by a Cholesky
 *   factorisation in double (lower, column by column, pivot p_j = A_jj - sum_k L_jk^2; no threshold: a rank-deficient system whose rounding leaves a
 *   tiny positive pivot is stepped, and its step is as large as that pivot is small - min_pixels, max_dist and the caller's own look at xi and the rms
 *   are the guards).  T' = Exp(-xi) * T in double,
 *   xi = (v, omega), Exp the SE(3) exponential: theta = |omega|, R = I + A[w]x + B[w]x^2, t = (I + B[w]x + C[w]x^2) v with A = sin(theta)/theta,
 *   B = (1 - cos(theta))/theta^2, C = (theta - sin(theta))/theta^3, and below theta = 1e-4 the series A = 1 - theta^2/6, B = 1/2 - theta^2/24,
 *   C = 1/6 - theta^2/120; T' is rounded to float, its last row (0, 0, 0, 1).  Status 0: stepped.  1: used < min_pixels.  2: a pivot was not
 *   positive, or a sum, xi or T' was not finite.  On 1 and 2 T' = T bit for bit and xi = 0.  rms = sqrt(chi2 / used), 0 when used is 0. */
typedef struct vdo_align vdo_align;
typedef struct vdo_align_params {
  float K[4];                       /* fx, fy, cx, cy of the frame; fx, fy > 0, all finite */
  float min_depth, max_depth;       /* 0 <= min_depth < max_depth, finite, metres */
  float max_dist;                   /* > 0, finite, metres: the gate on the distance between a point and its model point */
  int32_t subsample;                /* 1..8 */
  int32_t min_pixels;               /* >= 6 */
  int32_t max_iterations;           /* 1..64 */
  float eps;                        /* >= 0, finite: a solve stops when every component of xi is at most eps in magnitude */
  int32_t keep_rows;                /* 0 / 1: keep the row image of the last linearisation (vdo_align_get_rows) */
} vdo_align_params;
typedef struct vdo_align_report {
  int32_t iterations;               /* linearisations done */
  int32_t status;                   /* of the last step: 0, 1, 2 */
  int64_t used;                     /* samples used at the last linearisation */
  double rms_first, rms_last;       /* the RMS point-to-plane distance before the first step and at the last linearisation, metres */
  double xi[6];                     /* of the last step (0 unless its status is 0) */
} vdo_align_report;
/* An aligner for width x height depth and mask images.  ALL device memory is taken here (staging for a host or strided depth and mask, 8 bytes per
 * pixel; the tile partials, 256 bytes per 8 x 8 sample tile, and the levels above them; the model images the handle owns, 16 bytes per pixel of
 * the FRAME's size - a host model or a view with more pixels than the frame is refused, a borrowed device model may have any size; with keep_rows
 * the row image, 32 bytes per sample); the other entries allocate nothing.  VDO_ERR_INVALID, the message naming the argument: a null ctx, params
 * or out; a size < 1; a parameter outside the range written beside it or not finite.  VDO_ERR_UNSUPPORTED for an image over 2^26 pixels or 2^24
 * on a side.  VDO_ERR_OOM when the device has no room. */
int vdo_align_create(vdo_ctx* ctx, int width, int height, const vdo_align_params* params, vdo_align** out);
int vdo_align_destroy(vdo_align* h);
/* The model.  depth [Hm][Wm], grad [Hm][Wm][3] (packed), Km and Tm host.  is_device == 0: host images, copied into the handle's model images
 * (VDO_ERR_UNSUPPORTED when Wm * Hm exceeds width * height).  is_device != 0: packed device images, BORROWED - the caller keeps them alive and
 * unchanged until the next set_model.  VDO_ERR_INVALID, the message naming the argument, and then nothing changes: a null pointer, a size < 1,
 * a Km that is not finite or has fxm, fym <= 0.  A non-finite Tm is not refused: every sample is then skipped. */
int vdo_align_set_model(vdo_align* h, const float* depth, const float* grad, int model_width, int model_height, const float Km[4], const float Tm[16], int is_device);
/* Renders `view` at Tm (vdo_raycast_render) straight into the handle's device model images, no host round trip, and takes the view's size and K as
 * the model's.  counts (host, may be NULL): the render's three counts.  The render is host-synchronous on the view's own context, which may differ from
 * the aligner's on the same device.  VDO_ERR_INVALID for a view on another device, VDO_ERR_UNSUPPORTED when the view has more pixels than the frame. */
int vdo_align_set_model_from_view(vdo_align* h, vdo_raycast* view, const float Tm[16], int64_t counts[3]);
/* One linearisation at T, host-synchronous on the context's stream.  depth, mask, strides and src_is_device as vdo_dense_integrate takes them.
 * sums (host): the 28 sums in the order of the contract.  counts (host): used, no depth, masked, no model, far.  VDO_ERR_INVALID, the message
 * naming the argument, and then NOTHING is written: a null handle, depth, T, sums or counts; a stride too small; no model set.  A non-finite T is
 * not refused: every sample is then skipped. */
int vdo_align_linearise(vdo_align* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device, const float T[16],
                        double sums[28], int64_t counts[5]);
/* The same from the resident depth (after K1: metres) and mask of a vdo_frame_images of the aligner's size, read where they lie and not written. */
int vdo_align_linearise_frame(vdo_align* h, const vdo_frame_images* frame, const float T[16], double sums[28], int64_t counts[5]);
/* The host step of the contract.  Returns the status 0, 1 or 2, or VDO_ERR_INVALID for a null sums, T or T_out.  xi (6) and rms may be NULL. */
int vdo_align_step(const double sums[28], int64_t used, int64_t min_pixels, const float T[16], float T_out[16], double xi[6], double* rms);
/* Up to max_iterations rounds of linearise + step from T_init; the model stays fixed.  It stops after a step whose status is not 0 (T_out is then
 * the T of that linearisation) or whose xi is at most eps in every component.  report (host, may be NULL).  trace (host, may be NULL):
 * [max_iterations][16 + 28 + 5] doubles, per linearisation done the T it used, its sums and its counts; later rows are not written.  Refusals as
 * vdo_align_linearise, and a null T_init or T_out. */
int vdo_align_solve(vdo_align* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device, const float T_init[16],
                    float T_out[16], vdo_align_report* report, double* trace);
int vdo_align_solve_frame(vdo_align* h, const vdo_frame_images* frame, const float T_init[16], float T_out[16], vdo_align_report* report, double* trace);
/* With keep_rows: rows (host) [Hs][Ws][8] floats of the last linearisation - J (6), e, w, all 0 where the sample was skipped.  Storing them changes
 * no sum.  VDO_ERR_INVALID without keep_rows, before the first linearisation, or for a null pointer. */
int vdo_align_get_rows(vdo_align* h, float* rows);
/* The last linearise or solve: ms[0] wall time of the call, ms[1] device time of its linearisations, first command to last kernel (events). */
int vdo_align_last_timing(vdo_align* h, double ms[2]);

/* ---- Colourer: fused RGB beside a TSDF volume ------------------------------------------------------------------------------------------
 * New (the reference keeps no dense map): a colour per voxel of a vdo_dense - the static map or an object's volume -, fused per frame from the
 * image the frame's depth belongs to, and read back at points (Sample) or along a depth image (Render).  A vdo_colour BORROWS its map: it uses the
 * map's context, image size, K, depth range, voxel and origin, and is destroyed before it.  The geometry is fp32, one rounded operation per step in
 * the order written, no contraction (/ and floorf correctly rounded); everything after it is integer; no result depends on workgroup shape, on the
 * voxels a thread takes or on the schedule.  No float atomics.  The TSDF words are never read: no result depends on whether the same frame's
 * vdo_dense_integrate ran before or after.
 *
 * Colour volume.  One 32-bit word per voxel in the map's slot layout (voxel g at slot g_a mod n_a per axis, x fastest, then y, then z): bits 0-7 R,
 *   8-15 G, 16-23 B, 24-31 the colour weight cw.  cw == 0 is "no colour" and the whole word is then 0.
 * Follow.  The handle remembers the map origin it last saw (at create: the map's).  EVERY entry that reads or writes the colour volume - integrate,
 *   sample, render, get_volume, set_volume - first follows the map: if the map's origin differs from the remembered one by d, the slots whose global
 *   voxel changes are set to 0 (per axis with d_a != 0 the leaving slab: the first d_a voxels when d_a > 0, the last -d_a when d_a < 0, whole on the
 *   other two axes, one launch each) and no other word is touched; |d_a| >= n_a on any axis clears everything.  Only the difference since the last
 *   entry counts: a map moved away and back between two entries clears nothing.
 * Image.  uint8, `channels` 1 (grey, replicated), 3 or 4 (the fourth is ignored) per pixel, rows image_stride_bytes apart; rgb_order 0: R first,
 *   1: B first.  A pack kernel writes one uint32 R | G << 8 | B << 16 per pixel into the handle's [H][W] image; the fusion reads that word.
 * Integrate.  depth, mask, T and K as vdo_dense_integrate takes them; label an int.  Every voxel of the volume, from its own integer index:
 *      the projection and the tests of vdo_dense_integrate up to and including "skip unless d finite, d > min_depth, d <= max_depth", the pixel
 *      j = ((int)yq, (int)xq) the same bit for bit
 *      m = mask != NULL ? mask(j) : 0
 *      label == 0: skip if m != 0 (the static map);  label > 0: skip unless m == label (an object's volume);  label < 0: the mask is not read.
 *                                  A voxel skipped here counts in out[1].
 *      s = d - Zc;                 skip (counted in out[2]) if !(fabsf(s) <= band)
 *      q_c the pixel's channel c;  c' = (2*(c*cw + q_c) + (cw+1)) / (2*(cw+1)) per channel (integers, all non-negative);  cw' = min(cw+1, max_weight)
 *                                  counted in out[0]
 *   The colour word is read only by the voxels that reach the last step, and stored only when it changed.  A skipped voxel keeps its word.
 * Sample.  A world point p (3 floats), min_weight 1..255.  Per axis a:
 *      u = p_a / voxel;  u = u - 0.5f;  b = floorf(u);  f = u - b;  fi = (int)floorf(f * 256.0f)        (0..256; 256 when u - b rounds up to 1)
 *      no colour unless p_a is finite and -4194304.0f <= b <= 4194303.0f, compared as floats before any conversion to int
 *   The corners g = b + {0,1}^3 with the axis weight 256 - fi for offset 0 and fi for offset 1.  A corner COUNTS iff o_a <= g_a < o_a + n_a on every
 *   axis and its cw >= min_weight; its weight wgt is the product of its three axis weights.  Over the corners that count, in 64-bit integers:
 *   S = sum wgt (at most 2^24), C_c = sum wgt * c_c.  S == 0: rgba = (0, 0, 0, 0).  Else c = (2*C_c + S) / (2*S) and
 *   alpha = max(1, (255*S + (1 << 23)) >> 24): the share of the trilinear weight that had colour.
 *   NO OUT-OF-RANGE READS: every index is built from slot coordinates tested against n.
 * Render.  A depth image as vdo_raycast_render writes it (packed, z-depth, 0 for no surface) of any size, with the K = (fx, fy, cx, cy) and T it was
 *   rendered at.  Per pixel (x, y) with depth finite and > 0: the world point c_a + depth * r_a from the raycaster's camera centre c of T and ray r
 *   of the pixel (the point the aligner names), sampled as above.  Every other pixel is (0, 0, 0, 0). */
typedef struct vdo_colour vdo_colour;
typedef struct vdo_colour_params {
  float band;                       /* metres; 0 < band <= the map's trunc */
  int32_t max_weight;               /* 1..255 */
  int32_t stage_points;             /* >= 1: the points (or pixels) one window of a host sample (or render) holds on the device (16 bytes each) */
} vdo_colour_params;
/* A colourer for `map`.  ALL device memory is taken here (the colour volume, 4 bytes per voxel, cleared; the packed image, 4 bytes per pixel, and the
 * staging of a host image, 4 bytes per pixel; the counters; the window staging) - a host or strided depth and mask go through the MAP's staging
 * images; the other entries allocate nothing.  VDO_ERR_INVALID, the message naming the argument: a null map, params or out; a parameter outside the
 * range written beside it or not finite.  VDO_ERR_OOM when the device has no room. */
int vdo_colour_create(vdo_dense* map, const vdo_colour_params* params, vdo_colour** out);
int vdo_colour_destroy(vdo_colour* h);
/* One frame, host-synchronous, on the map's context stream: follow, pack, one fusion kernel.  depth, mask, their strides and T as
 * vdo_dense_integrate takes them; image: rows of `width` pixels of `channels` bytes, image_stride_bytes apart; all three images are host pointers,
 * or device pointers when src_is_device != 0.  out (host): voxels updated, voxels skipped by the label rule, voxels skipped by the band rule.
 * VDO_ERR_INVALID, the message naming the argument, and then NOTHING is written (the volume is not even followed): a null handle, depth, image, T or
 * out; a depth or mask stride smaller than the width; image_stride_bytes smaller than width * channels; channels not 1, 3 or 4; rgb_order not 0
 * or 1. */
int vdo_colour_integrate(vdo_colour* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, const uint8_t* image,
                         int64_t image_stride_bytes, int channels, int rgb_order, int src_is_device, int label, const float T[16], int64_t out[3]);
/* The same from the resident depth (after K1: metres) and mask of a vdo_frame_images of the map's image size, read where they lie and not written;
 * image_is_device says where `image` lives.  Refusals as above, and a null frame or one of another size. */
int vdo_colour_integrate_frame(vdo_colour* h, const vdo_frame_images* frame, const uint8_t* image, int64_t image_stride_bytes, int channels, int rgb_order,
                               int image_is_device, int label, const float T[16], int64_t out[3]);
/* The colour of the map at n world points: xyz float [n][3] in, rgba uint8 [n][4] out, both host pointers, or both device pointers when
 * is_device != 0 (host points go through the stage_points window).  *n_coloured (host): the points with S != 0.  VDO_ERR_INVALID, the message
 * naming the argument, and then NOTHING is written: a null handle or n_coloured; n < 0; a null xyz or rgba with n > 0; min_weight outside 1..255; a
 * device rgba that is not 4-byte aligned (a point's four bytes are written as one word; a host rgba may lie anywhere). */
int vdo_colour_sample(vdo_colour* h, int64_t n, const float* xyz, int min_weight, uint8_t* rgba, int is_device, int64_t* n_coloured);
/* The colour image of a depth image: depth float [height][width] in, rgba uint8 [height][width][4] out, both packed, both host pointers (through
 * the stage_points window) or both device pointers when is_device != 0.  K, T: host.  out (host): pixels coloured, pixels with depth but no colour.
 * VDO_ERR_INVALID, the message naming the argument, and then NOTHING is written: a null handle, depth, K, T, rgba or out; a size < 1; a K that is
 * not finite or has fx, fy <= 0; min_weight outside 1..255; a device rgba that is not 4-byte aligned.  VDO_ERR_UNSUPPORTED for an image over 2^26 pixels or 2^24 on a side.  A non-finite T
 * is not refused: its points have no colour. */
int vdo_colour_render(vdo_colour* h, const float* depth, int width, int height, const float K[4], const float T[16], int min_weight, uint8_t* rgba, int is_device,
                      int64_t out[2]);
/* Sets every colour word to 0 and remembers the map's present origin: a reused object handle after vdo_dense_clear. */
int vdo_colour_clear(vdo_colour* h);
/* Inspection, after following the map: the words in slot order (host, nx * ny * nz; may be NULL) and the origin (host; may be NULL; not both). */
int vdo_colour_get_volume(vdo_colour* h, uint32_t* words, int32_t origin[3]);
/* The reverse: nx * ny * nz host words in slot order replace the colour volume after it followed the map.  The caller keeps the format: cw = 0 only
 * with the whole word 0. */
int vdo_colour_set_volume(vdo_colour* h, const uint32_t* words);
/* The y-consecutive voxels one thread of the fusion kernel takes: 1, 2, 4 (the default) or 8.  No result depends on it. */
int vdo_colour_set_voxels_per_thread(vdo_colour* h, int voxels);
/* The last integrate, sample or render: ms[0] wall time of the call, ms[1] device time from the first command to the end of the last kernel. */
int vdo_colour_last_timing(vdo_colour* h, double ms[2]);

/* ---- Distance field: exact Euclidean clearance from a TSDF volume ------------------------------------------------------------------------
 * New (the reference keeps no dense map): how far a voxel of a vdo_dense - the static map or an object's volume - is from the mapped surface, as
 * the exact squared Euclidean distance, in voxels, to the nearest voxel at a zero crossing, and whether the voxel is free, inside or unknown.  The
 * TSDF itself cannot say: it is truncated, projective and 0 where nothing was seen.  Integer from end to end; the map is read only.  Notation as
 * above: the volume covers the global voxels o_a <= g_a < o_a + n_a, words t (int16) and w, cyclic slots.
 *
 * Valid, site, state.  min_weight 1..255.  A voxel is VALID iff w >= min_weight.  A valid voxel a is a SITE iff some 6-neighbour b = a +- e_k lies
 *   inside the VOLUME (not the box), is valid, and (ta < 0) != (tb < 0): the two ends of exactly the lattice edges Extract and the Mesher call
 *   crossings.  The STATE of a voxel: 0 unknown (not valid), 1 free (valid, t >= 0), 2 inside (valid, t < 0).
 * Field.  A box [lo, hi) in global voxels, clipped to the volume, as Extract takes it; radius R 1..8191 voxels.  One uint32 per voxel of the CLIPPED
 *   box in the order z, y, x (x fastest) - box order, not slot order: the field does not wrap.
 *      bits 0-27   d2: the smallest dx^2 + dy^2 + dz^2 (voxels^2) to a site INSIDE THE BOX if that is <= R^2, else FAR = 0x0FFFFFFF
 *      bits 28-29  the state
 *      bits 30-31  0
 *   d2 is exact: d2 == 0 iff the voxel is a site; d2 == R^2 is kept, R^2 + 1 is FAR.  Only the distance is stored, so ties between sites cannot
 *   show.  Sites outside the box do not count: a caller that wants the field exact up to R in a region pads its box by R.  3 * 4095^2 < 2^26 and
 *   8191^2 < 2^27: nothing overflows the 28 bits, and R >= 7093 caps nothing.
 * Snapshot.  The handle keeps the last field on the device with its clipped box in GLOBAL voxels and the map's voxel size.  Later integrations or
 *   moves of the map do not touch it; a sample after a recentre still names the right voxel.  An empty box, or one outside the volume, gives an
 *   empty snapshot: counts (0, 0, 0), and every sample is outside.
 * Sample.  A world point p (3 floats).  Per axis a:
 *      u = p_a / voxel;  b = floorf(u)                          (one rounded operation per step, no contraction)
 *      outside unless p_a is finite and -4194304.0f <= b <= 4194303.0f, compared as floats before any conversion to int;  then g_a = (int)b
 *   The result is the field word of g if g lies in the snapshot's box, else VDO_DISTANCE_OUTSIDE.  NO OUT-OF-RANGE READS: no address is formed
 *   before the compares have passed.
 * No result depends on launch shape, method, schedule or the slot alignment of the cyclic volume. */
#define VDO_DISTANCE_FAR 0x0FFFFFFFu
#define VDO_DISTANCE_OUTSIDE 0xFFFFFFFFu
#define VDO_DISTANCE_WINDOW 262144     /* the points one window of a host sample holds on the device (16 bytes each) */
typedef struct vdo_distance vdo_distance;
typedef struct vdo_distance_params {
  int32_t n[3];                     /* 1..4096 each, nx * ny * nz <= 2^31: the handle serves every clipped box with no more voxels than that product */
} vdo_distance_params;
/* ALL device memory is taken here (the field and one buffer of the same size for the passes, 4 bytes per voxel each; one site bit per voxel; the
 * counters; the sample window); the other entries allocate nothing.  One handle serves any vdo_dense of the same context: the static map and all
 * object volumes can share one.  VDO_ERR_INVALID, the message naming the argument: a null pointer, a size < 1.  VDO_ERR_UNSUPPORTED beyond the dense
 * mapper's limits (a side above 2^12, more than 2^31 voxels).  VDO_ERR_OOM when the device has no room. */
int vdo_distance_create(vdo_ctx* ctx, const vdo_distance_params* params, vdo_distance** out);
int vdo_distance_destroy(vdo_distance* h);
/* The field of `map` for the box, host-synchronous on the context's stream; it becomes the snapshot.  counts (host): sites in the box, voxels with
 * d2 != FAR, voxels of the clipped box.  VDO_ERR_INVALID, the message naming the argument, and then NOTHING is written and the previous snapshot
 * stays: a null handle, map, lo, hi or counts; min_weight outside 1..255; radius outside 1..8191; a map of another context; a clipped box with more
 * voxels than the handle holds. */
int vdo_distance_compute(vdo_distance* h, vdo_dense* map, const int32_t lo[3], const int32_t hi[3], int min_weight, int radius, int64_t counts[3]);
/* The snapshot, a plain copy: its words (host, or device when out_is_device != 0; may be NULL) and its clipped box (host; each may be NULL; an empty
 * snapshot has lo = hi = 0).  VDO_ERR_INVALID for a null handle and before the first compute. */
int vdo_distance_get(vdo_distance* h, uint32_t* words, int out_is_device, int32_t lo[3], int32_t hi[3]);
/* The snapshot at n world points: xyz float [n][3] in, words uint32 [n] out, both host pointers (through the window of VDO_DISTANCE_WINDOW points) or
 * both device pointers when is_device != 0.  *n_inside (host): the points that fell inside the box.  Before the first compute every point is
 * outside.  VDO_ERR_INVALID, the message naming the argument, and then NOTHING is written: a null handle or n_inside; n < 0; a null xyz or words
 * with n > 0. */
int vdo_distance_sample(vdo_distance* h, int64_t n, const float* xyz, uint32_t* words, int is_device, int64_t* n_inside);
/* The snapshot where it lives (a device pointer owned by the handle, valid until the next compute). */
int vdo_distance_device_field(vdo_distance* h, uint32_t** words);
/* How the y and z passes find their minima: 1 a windowed minimum over |q - p| <= R, 2 the lower envelope of parabolas, 0 (the default) the
 * handle's own choice between them.  No result depends on it.  VDO_ERR_INVALID for another value. */
int vdo_distance_set_method(vdo_distance* h, int method);
/* The last compute or sample: ms[0] wall time of the call, ms[1] device time from the first command to the end of the last kernel. */
int vdo_distance_last_timing(vdo_distance* h, double ms[2]);

/* ---- Photometric aligner: an intensity term beside the aligner's point-to-plane ICP, and their joint solve ------------------------------------
 * New (the reference has no dense pose estimator).  Point-to-plane ICP cannot see a motion that slides along the surface: in front of a road, a
 * facade or a corridor wall two or three of the six motions leave every residual of the Aligner unchanged.  The texture on the surface can see them.
 * A vdo_photo compares the grey value of every frame pixel with the bilinear grey value of a MODEL image at the pixel's projection, and gives the
 * normal equations of that residual in the Aligner's own form - the same twist about the camera, the same 28 sums, the same tree -, so that the two
 * systems add (vdo_photo_combine) and the Aligner's host step (vdo_align_step) solves their sum.  All per-sample arithmetic is fp32, one rounded
 * operation per step in the order written, no contraction (/ and floorf correctly rounded); every gathered address is bounded by float compares
 * made before any conversion to int (a NaN fails them); the 28 terms are exact double products; the sums are in double in ONE fixed tree.  No float
 * atomics.  No result depends on workgroup shape, on the launch shape or on the schedule; two runs give the same bits.
 *
 * Grey image.  The frame's image is uint8, `channels` 1, 3 or 4 (the fourth is ignored) per pixel, rows image_stride_bytes apart, rgb_order 0: R
 *   first, 1: B first - as vdo_colour_integrate takes it.  Y = (77*R + 150*G + 29*B + 128) >> 8 in integers (77 + 150 + 29 = 256: a grey pixel
 *   keeps its value, 0 and 255 stay 0 and 255); with 1 channel Y is the value.  Y is stored as a float, which is exact.  The handle owns ONE
 *   [H][W] float image I of the current frame, written by a pack kernel (vdo_photo_set_image).  An intensity is VALID iff it is finite and >= 0
 *   (a packed image is valid everywhere; a model's intensity image may hold anything).
 * Model.  The handle owns ONE packed image [Hm][Wm] of (depth, intensity) float pairs with its intrinsics Km = (fxm, fym, cxm, cym) and its pose
 *   Tm (world -> camera, as T); nothing is borrowed.  Its size and intrinsics may differ from the frame's; Wm * Hm is at most W * H.  Dm is a
 *   z-depth.  A model pixel is USABLE iff its depth is finite and > 0 and its intensity is valid.  vdo_photo_set_model packs any two float
 *   images unchanged.  vdo_photo_keep_as_model makes the current frame the model: the intensity is I, Km = K, Tm = T, and the depth is d where
 *   d passes the frame's depth test below and the mask is NULL or 0 there, else 0.0f - moving objects are left out of the model.
 * Inputs of a linearisation.  depth D[H][W], mask, K, T and the samples exactly as the Aligner has them; I as above.
 * Per sample (i, j), pixel (x, y) = (i*s, j*s):
 *      d = D(y,x);  iF = I(y,x);   skip[no depth] unless d finite, d > max(min_depth, 0) and d <= max_depth, and iF valid
 *                                  skip[masked] if mask != NULL and mask(y,x) != 0
 *      dx, dy, Pc, q, Pw, Xm, Ym, Zm as the Aligner;          skip[no model] unless Zm finite and Zm > FLT_MIN
 *      u = (fxm*Xm)/Zm + cxm;  v = (fym*Ym)/Zm + cym;  x0 = floorf(u);  y0 = floorf(v)
 *                                  skip[no model] unless u, v finite, 0 <= x0 <= (float)(Wm-2), 0 <= y0 <= (float)(Hm-2)
 *                                  (so u = Wm-1 exactly has no model, and a model with Wm < 2 or Hm < 2 skips every sample as no model)
 *      fa = u - x0;  fb = v - y0
 *      the model pixels (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1): depths d00 d10 d01 d11, intensities i00 i10 i01 i11
 *                                  skip[no model] unless all four are usable
 *                                  skip[far] unless fabsf(dk - Zm) <= max_dist for all four (the occlusion gate)
 *      top = i00 + fa*(i10 - i00);  bot = i01 + fa*(i11 - i01);  im = top + fb*(bot - top)
 *      gx = (i10 - i00) + fb*((i11 - i01) - (i10 - i00));  gy = bot - top
 *      e = im - iF;                skip[far] unless fabsf(e) <= max_diff
 *      iz = 1.0f/Zm;  ax = (fxm*gx)*iz;  ay = (fym*gy)*iz;  az = -(((ax*Xm) + (ay*Ym))*iz)      (the gradient of im by the point in the model's camera)
 *      gw_a = (Tm0a*ax + Tm1a*ay) + Tm2a*az                                                      (in the world)
 *      gc_a = (Ta0*gw0 + Ta1*gw1) + Ta2*gw2                                                      (in the frame's camera)
 *      J = (gc0, gc1, gc2,  Pc1*gc2 - Pc2*gc1,  Pc2*gc0 - Pc0*gc2,  Pc0*gc1 - Pc1*gc0);   w = 1
 *   e is in grey levels.  With T' = Exp(-xi) * T the residual changes by J . xi to first order, the Aligner's convention.
 * Terms, 28 per sample, in double and exact: A_ij = (double)J_i * (double)J_j, i <= j, row-major; b_i = (double)J_i * (double)e;
 *   chi2 = (double)e * (double)e.  A skipped sample contributes +0.0.
 * The sum: the Aligner's, word for word - 8 x 8 sample tiles, slot ((j/8)*tiles_x + i/8)*64 + (j%8)*8 + (i%8), padded with +0.0 to a power of two,
 *   the adjacent-pair tree in double.  Counts, int64: used, no depth, masked, no model, far; they add up to Ws*Hs.
 * Combine (vdo_photo_combine, pure host code).  lam = weight*weight; out[k] = geo[k] + lam*photo[k], two rounded operations in double, no
 *   contraction; a NULL geo stands for 28 values +0.0.  weight is in metres per grey level: it turns a grey residual into the Aligner's metres.
 * Solve.  Per round, at the same T: the photometric linearisation, and with a vdo_align its linearisation of the same depth and mask.  Status 1
 *   (T unchanged, xi = 0) if used_p < min_pixels or (a vdo_align is given and used_g < ITS min_pixels).  Otherwise combine and
 *   vdo_align_step(out, used_g + used_p, 6, T, ..).  The stop rules are vdo_align_solve's. */
typedef struct vdo_photo vdo_photo;
typedef struct vdo_photo_params {
  float K[4];                       /* fx, fy, cx, cy of the frame; fx, fy > 0, all finite */
  float min_depth, max_depth;       /* 0 <= min_depth < max_depth, finite, metres */
  float max_dist;                   /* > 0, finite, metres: the gate on |model depth - Zm| at each of the four model pixels */
  float max_diff;                   /* > 0, finite, grey levels: the gate on |e|; 255 turns it off */
  int32_t subsample;                /* 1..8 */
  int32_t min_pixels;               /* >= 6 */
  int32_t max_iterations;           /* 1..64 */
  float eps;                        /* >= 0, finite: a solve stops when every component of xi is at most eps in magnitude */
  int32_t keep_rows;                /* 0 / 1: keep the row image of the last linearisation (vdo_photo_get_rows) */
} vdo_photo_params;
typedef struct vdo_photo_report {
  int32_t iterations;               /* rounds done */
  int32_t status;                   /* of the last round: 0, 1, 2 */
  int64_t used_geo, used_photo;     /* samples used at the last round (used_geo 0 without a vdo_align) */
  double rms_geo_first, rms_geo_last;       /* sqrt(chi2_geo / used_geo), metres, 0 when used_geo is 0 */
  double rms_photo_first, rms_photo_last;   /* sqrt(chi2_photo / used_photo), grey levels, 0 when used_photo is 0 */
  double xi[6];                     /* of the last step (0 unless its status is 0) */
} vdo_photo_report;
#define VDO_PHOTO_TRACE_ROW (16 + 28 + 5 + 28 + 5)
/* A photometric aligner for width x height frames.  ALL device memory is taken here (staging for a host or strided depth and mask, 8 bytes per
 * pixel, and for a host image, 4; the grey image, 4; the model, 8 per pixel of the FRAME's size; the tile partials, 256 bytes per 8 x 8 sample
 * tile, and the levels above them; with keep_rows the row image, 32 bytes per sample); the other entries allocate nothing.  Refusals as
 * vdo_align_create, and max_diff not positive or not finite. */
int vdo_photo_create(vdo_ctx* ctx, int width, int height, const vdo_photo_params* params, vdo_photo** out);
int vdo_photo_destroy(vdo_photo* h);
/* The current frame's image -> I, host-synchronous.  image is a host pointer, or a device pointer when is_device != 0.  VDO_ERR_INVALID, the
 * message naming the argument, and then nothing changes: a null handle or image; image_stride_bytes smaller than width * channels; channels not
 * 1, 3 or 4; rgb_order not 0 or 1. */
int vdo_photo_set_image(vdo_photo* h, const uint8_t* image, int64_t image_stride_bytes, int channels, int rgb_order, int is_device);
/* The model from two packed float images [Hm][Wm], both host pointers or both device pointers (is_device != 0); they are copied (interleaved)
 * and not kept.  VDO_ERR_INVALID, the message naming the argument, and then nothing changes: a null pointer, a size < 1, a Km that is not finite
 * or has fxm, fym <= 0.  VDO_ERR_UNSUPPORTED when Wm * Hm exceeds width * height; the previous model stays.  A non-finite Tm is not refused:
 * every sample is then skipped. */
int vdo_photo_set_model(vdo_photo* h, const float* depth, const float* intensity, int model_width, int model_height, const float Km[4], const float Tm[16], int is_device);
/* The current frame becomes the model (see "Model"): depth, mask, strides and src_is_device as vdo_photo_linearise takes them, I as the last
 * vdo_photo_set_image left it, Km = K, Tm = T.  VDO_ERR_INVALID, and then nothing changes: a null handle, depth or T; a stride too small; no
 * image set. */
int vdo_photo_keep_as_model(vdo_photo* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device, const float T[16]);
/* The same from the resident depth (after K1: metres) and mask of a vdo_frame_images of the handle's size, read where they lie and not written. */
int vdo_photo_keep_as_model_frame(vdo_photo* h, const vdo_frame_images* frame, const float T[16]);
/* Inspection.  vdo_photo_get_image: I, [H][W] floats (host).  vdo_photo_get_model: the pairs, [Hm][Wm][2] floats (host, may be NULL), and the
 * model's size (host, each may be NULL).  VDO_ERR_INVALID for a null handle or grey, and before the first image / model. */
int vdo_photo_get_image(vdo_photo* h, float* grey);
int vdo_photo_get_model(vdo_photo* h, float* pairs, int* model_width, int* model_height);
/* The combine of the contract: pure host code, no device or context.  geo may be NULL; out may be geo or photo.  VDO_ERR_INVALID for a null
 * photo or out and for a weight that is not positive and finite; nothing is written then. */
int vdo_photo_combine(const double geo[28], const double photo[28], double weight, double out[28]);
/* One linearisation at T, host-synchronous on the context's stream.  depth, mask, strides and src_is_device as vdo_align_linearise takes them.
 * sums (host): the 28 sums.  counts (host): used, no depth, masked, no model, far.  VDO_ERR_INVALID, the message naming the argument, and then
 * NOTHING is written: a null handle, depth, T, sums or counts; a stride too small; no image set; no model set.  A non-finite T is not refused:
 * every sample is then skipped. */
int vdo_photo_linearise(vdo_photo* h, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device, const float T[16],
                        double sums[28], int64_t counts[5]);
int vdo_photo_linearise_frame(vdo_photo* h, const vdo_frame_images* frame, const float T[16], double sums[28], int64_t counts[5]);
/* Up to max_iterations rounds from T_init (see "Solve"); both models stay fixed.  geo: a vdo_align of the same frame size on the same device
 * with its model set, or NULL for the photometric term alone.  It stops after a round whose status is not 0 (T_out is then the T of that round)
 * or whose xi is at most eps in every component.  report (host, may be NULL).  trace (host, may be NULL): [max_iterations][VDO_PHOTO_TRACE_ROW]
 * doubles, per round the T it used, the geometric sums and counts (0 without geo) and the photometric sums and counts; later rows are not
 * written.  Refusals as vdo_photo_linearise, and: a null T_init or T_out; a weight that is not positive and finite; a geo of another frame
 * size or device, or without a model. */
int vdo_photo_solve(vdo_photo* h, vdo_align* geo, const float* depth, int64_t depth_stride_floats, const int32_t* mask, int64_t mask_stride_ints, int src_is_device, double weight,
                    const float T_init[16], float T_out[16], vdo_photo_report* report, double* trace);
int vdo_photo_solve_frame(vdo_photo* h, vdo_align* geo, const vdo_frame_images* frame, double weight, const float T_init[16], float T_out[16], vdo_photo_report* report,
                          double* trace);
/* With keep_rows: rows (host) [Hs][Ws][8] floats of the last photometric linearisation - J (6), e, w (1 where used), all 0 where the sample was
 * skipped.  Storing them changes no sum.  VDO_ERR_INVALID without keep_rows, before the first linearisation, or for a null pointer. */
int vdo_photo_get_rows(vdo_photo* h, float* rows);
/* The last linearise or solve: ms[0] wall time of the call, ms[1] device time of its PHOTOMETRIC linearisations, first command to last kernel. */
int vdo_photo_last_timing(vdo_photo* h, double ms[2]);

#ifdef __cplusplus
}
#endif
#endif /* VDO_SLAM_HIP_H_ */
