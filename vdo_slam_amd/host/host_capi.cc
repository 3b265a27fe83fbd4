// extern "C" hooks that let the Python test-suite drive the C++ host classes of this directory
// (ORBextractor / Frame / Optimizer with the reference's signatures).  Not part of the product
// ABI (that is include/vdo_slam_hip.h); they only marshal flat arrays into Map / Frame objects.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "Converter.h"
#include "DenseMapper.h"
#include "FlowMatcher.h"
#include "InstanceLabeler.h"
#include "Frame.h"
#include "Map.h"
#include "MotionSegmenter.h"
#include "ObjectMapper.h"
#include "ORBextractor.h"
#include "ORBmatcher.h"
#include "Optimizer.h"
#include "StereoMatcher.h"
#include "System.h"

using namespace VDO_SLAM;

extern "C" {

struct host_map_flat {
  int n_frames;
  const float* K;                                    // 3x3
  const float* cam_pose;                             // [F][16]
  const int* sta_cnt; const float *sta_uv, *sta_d, *sta_xw;
  int n_tr_sta; const int *tr_sta_len, *tr_sta_pairs;
  const int* dyn_cnt; const float *dyn_uv, *dyn_d, *dyn_xw;
  int n_tr_dyn; const int *tr_dyn_len, *tr_dyn_pairs, *obj_of_dyn;
  const int* rm_cnt; const float* rm; const int* rm_label;
};

static cv::Mat mat44(const float* p) { cv::Mat m(4, 4, cv::CV_32F); std::memcpy(m.data, p, 64); return m; }
static cv::Mat mat31(const float* p) { cv::Mat m(3, 1, cv::CV_32F); std::memcpy(m.data, p, 12); return m; }

int host_batch_optimization(const host_map_flat* f, int partial_window, float* cam_pose_out, float* rm_out,
                            float* sta_xw_out, float* dyn_xw_out, vdo_lm_stats* st) {
  Map map;
  const int F = f->n_frames;
  cv::Mat K(3, 3, cv::CV_32F);
  std::memcpy(K.data, f->K, 36);
  size_t so = 0, dof = 0, ro = 0;
  map.vpFeatSta.resize(F); map.vfDepSta.resize(F); map.vp3DPointSta.resize(F);
  map.vpFeatDyn.resize(F); map.vfDepDyn.resize(F); map.vp3DPointDyn.resize(F);
  for (int i = 0; i < F; ++i) {
    map.vmCameraPose.push_back(mat44(f->cam_pose + 16 * i));
    for (int j = 0; j < f->sta_cnt[i]; ++j, ++so) {
      map.vpFeatSta[i].push_back(cv::KeyPoint(f->sta_uv[2 * so], f->sta_uv[2 * so + 1], 0));
      map.vfDepSta[i].push_back(f->sta_d[so]);
      map.vp3DPointSta[i].push_back(mat31(f->sta_xw + 3 * so));
    }
    for (int j = 0; j < f->dyn_cnt[i]; ++j, ++dof) {
      map.vpFeatDyn[i].push_back(cv::KeyPoint(f->dyn_uv[2 * dof], f->dyn_uv[2 * dof + 1], 0));
      map.vfDepDyn[i].push_back(f->dyn_d[dof]);
      map.vp3DPointDyn[i].push_back(mat31(f->dyn_xw + 3 * dof));
    }
    if (i < F - 1) {
      std::vector<cv::Mat> mots; std::vector<int> labs;
      for (int j = 0; j < f->rm_cnt[i]; ++j, ++ro) { mots.push_back(mat44(f->rm + 16 * ro)); labs.push_back(f->rm_label[ro]); }
      map.vmRigidMotion.push_back(mots); map.vnRMLabel.push_back(labs);
    }
  }
  map.vmCameraPose_RF = map.vmCameraPose; map.vmRigidMotion_RF = map.vmRigidMotion;
  size_t po = 0;
  for (int t = 0; t < f->n_tr_sta; ++t) {
    std::vector<std::pair<int, int> > tr;
    for (int k = 0; k < f->tr_sta_len[t]; ++k, ++po) tr.push_back(std::make_pair(f->tr_sta_pairs[2 * po], f->tr_sta_pairs[2 * po + 1]));
    map.TrackletSta.push_back(tr);
  }
  po = 0;
  for (int t = 0; t < f->n_tr_dyn; ++t) {
    std::vector<std::pair<int, int> > tr;
    for (int k = 0; k < f->tr_dyn_len[t]; ++k, ++po) tr.push_back(std::make_pair(f->tr_dyn_pairs[2 * po], f->tr_dyn_pairs[2 * po + 1]));
    map.TrackletDyn.push_back(tr);
    map.nObjID.push_back(f->obj_of_dyn[t]);
  }
  try {
    if (partial_window > 0) Optimizer::PartialBatchOptimization(&map, K, partial_window);
    else Optimizer::FullBatchOptimization(&map, K);
  } catch (const std::exception& e) { std::fprintf(stderr, "host_batch_optimization: %s\n", e.what()); return -1; }
  if (st) *st = Optimizer::last_batch_stats;
  so = dof = ro = 0;
  for (int i = 0; i < F; ++i) {
    const cv::Mat& T = partial_window > 0 ? map.vmCameraPose[i] : map.vmCameraPose_RF[i];
    std::memcpy(cam_pose_out + 16 * i, T.data, 64);
    for (int j = 0; j < f->sta_cnt[i]; ++j, ++so) std::memcpy(sta_xw_out + 3 * so, map.vp3DPointSta[i][j].data, 12);
    for (int j = 0; j < f->dyn_cnt[i]; ++j, ++dof) std::memcpy(dyn_xw_out + 3 * dof, map.vp3DPointDyn[i][j].data, 12);
    if (i < F - 1)
      for (int j = 0; j < f->rm_cnt[i]; ++j, ++ro) {
        const cv::Mat& M = partial_window > 0 ? map.vmRigidMotion[i][j] : map.vmRigidMotion_RF[i][j];
        std::memcpy(rm_out + 16 * ro, M.data, 64);
      }
  }
  return 0;
}

// Frame::Frame through the host classes (after GrabImageRGBD's depth preprocessing).  Returns N (ORB keypoints).
int host_frame(const unsigned char* gray, float* depth_raw_inout, const float* flow, const int* mask, int w, int h,
               float bf, float depth_factor, float th_bg, float th_obj,
               float* kx, float* ky, int* koct, int cap,
               int* n_stat, float* stat_corr /*[cap][2]*/, float* stat_depth, int* n_obj, float* obj_key /*[capo][2]*/, int* obj_label, int capo) {
  try {
  static ORBextractor* orb = nullptr;
  if (!orb) orb = new ORBextractor(2500, 1.2f, 8, 20, 7);
  if (vdo_depth_preprocess(HostContext(), depth_raw_inout, (int64_t)w * h, bf, depth_factor, 0) != VDO_OK) return -1;   // Tracking.cc:180-204
  cv::Mat G(h, w, cv::CV_8UC1, (void*)gray), D(h, w, cv::CV_32FC1, depth_raw_inout), Fl(h, w, cv::CV_32FC2, (void*)flow), M(h, w, cv::CV_32SC1, (void*)mask);
  cv::Mat K = cv::Mat::eye(3, 3, cv::CV_32F), dist = cv::Mat::zeros(4, 1, cv::CV_32F);
  K.at<float>(0, 0) = 721.5377f; K.at<float>(1, 1) = 721.5377f; K.at<float>(0, 2) = 609.5593f; K.at<float>(1, 2) = 172.854f;
  Frame fr(G, D, Fl, M, 0.0, orb, K, dist, bf, th_bg, th_obj, 0);
  for (int i = 0; i < fr.N && i < cap; ++i) { kx[i] = fr.mvKeys[i].pt.x; ky[i] = fr.mvKeys[i].pt.y; koct[i] = fr.mvKeys[i].octave; }
  *n_stat = fr.N_s_tmp;
  for (int i = 0; i < fr.N_s_tmp && i < cap; ++i) { stat_corr[2 * i] = fr.mvCorres[i].pt.x; stat_corr[2 * i + 1] = fr.mvCorres[i].pt.y; stat_depth[i] = fr.mvStatDepthTmp[i]; }
  *n_obj = (int)fr.mvObjKeys.size();
  for (int i = 0; i < *n_obj && i < capo; ++i) { obj_key[2 * i] = fr.mvObjKeys[i].pt.x; obj_key[2 * i + 1] = fr.mvObjKeys[i].pt.y; obj_label[i] = fr.vSemObjLabel[i]; }
  return fr.N;
  } catch (const std::exception& e) { std::fprintf(stderr, "host_frame: %s\n", e.what()); return -1; }
}

// Optimizer::PoseOptimizationFlow2Cam through the host classes.  Tcw_last / Tcw_init: 4x4 float row-major.
int host_pose_optimization_flow2cam(int n, const float* last_xy, const float* flow, const float* depth, const float* Tcw_last,
                                    const float* Tcw_init, float* Tcw_out, int* match_out, float* cur_xy_out) {
  Frame last, cur;
  Frame::fx = 721.5377f; Frame::fy = 721.5377f; Frame::cx = 609.5593f; Frame::cy = 172.854f;
  last.mTcw = mat44(Tcw_last); cur.mTcw = mat44(Tcw_init);
  std::vector<int> match(n);
  for (int i = 0; i < n; ++i) {
    last.mvStatKeys.push_back(cv::KeyPoint(last_xy[2 * i], last_xy[2 * i + 1], 0));
    last.mvFlowNext.push_back(cv::Point2f(flow[2 * i], flow[2 * i + 1]));
    last.mvStatDepth.push_back(depth[i]);
    cur.mvStatKeys.push_back(cv::KeyPoint(last_xy[2 * i] + flow[2 * i], last_xy[2 * i + 1] + flow[2 * i + 1], 0));
    match[i] = i;
  }
  int inl;
  try { inl = Optimizer::PoseOptimizationFlow2Cam(&cur, &last, match); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return -1; }
  std::memcpy(Tcw_out, cur.mTcw.data, 64);
  for (int i = 0; i < n; ++i) { match_out[i] = match[i]; cur_xy_out[2 * i] = cur.mvStatKeys[i].pt.x; cur_xy_out[2 * i + 1] = cur.mvStatKeys[i].pt.y; }
  return inl;
}

// Optimizer::PoseOptimizationNew through the host classes: the last frame's static keys + depths are back-projected with its
// pose (UnprojectStereoStat), the current frame's keys are the observations.  Returns the inlier count.
int host_pose_optimization_new(int n, const float* last_xy, const float* depth, const float* cur_xy, const float* Tcw_last, const float* Tcw_init,
                               float* Tcw_out, int* match_out) {
  Frame last, cur;
  Frame::fx = 721.5377f; Frame::fy = 721.5377f; Frame::cx = 609.5593f; Frame::cy = 172.854f; Frame::invfx = 1.0f / Frame::fx; Frame::invfy = 1.0f / Frame::fy;
  last.mTcw = mat44(Tcw_last); cur.mTcw = mat44(Tcw_init);
  std::vector<int> match(n);
  for (int i = 0; i < n; ++i) {
    last.mvStatKeys.push_back(cv::KeyPoint(last_xy[2 * i], last_xy[2 * i + 1], 0));
    last.mvStatDepth.push_back(depth[i]);
    cur.mvStatKeys.push_back(cv::KeyPoint(cur_xy[2 * i], cur_xy[2 * i + 1], 0));
    match[i] = i;
  }
  int inl = -1;
  try { inl = Optimizer::PoseOptimizationNew(&cur, &last, match); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return -1; }
  std::memcpy(Tcw_out, cur.mTcw.data, 64);
  for (int i = 0; i < n; ++i) match_out[i] = match[i];
  return inl;
}

// Optimizer::PoseOptimizationObjMot through the host classes.  Returns the number of inliers; H_out = the returned motion.
int host_pose_optimization_objmot(int n, const float* last_xy, const float* depth, const float* cur_xy, const float* Tcw_last, const float* Tcw_cur,
                                  const float* init_model, float* H_out, int* inlier_flag, int* obj_label_out) {
  Frame last, cur;
  Frame::fx = 721.5377f; Frame::fy = 721.5377f; Frame::cx = 609.5593f; Frame::cy = 172.854f; Frame::invfx = 1.0f / Frame::fx; Frame::invfy = 1.0f / Frame::fy;
  last.mTcw = mat44(Tcw_last); cur.mTcw = mat44(Tcw_cur); cur.mInitModel = mat44(init_model);
  std::vector<int> ids(n), inliers;
  for (int i = 0; i < n; ++i) {
    last.mvObjKeys.push_back(cv::KeyPoint(last_xy[2 * i], last_xy[2 * i + 1], 0));
    last.mvObjDepth.push_back(depth[i]);
    cur.mvObjKeys.push_back(cv::KeyPoint(cur_xy[2 * i], cur_xy[2 * i + 1], 0));
    cur.vObjLabel.push_back(7);
    ids[i] = i;
  }
  cv::Mat H;
  try { H = Optimizer::PoseOptimizationObjMot(&cur, &last, ids, inliers); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return -1; }
  std::memcpy(H_out, H.data, 64);
  for (int i = 0; i < n; ++i) { inlier_flag[i] = 0; obj_label_out[i] = cur.vObjLabel[i]; }
  for (int id : inliers) inlier_flag[id] = 1;
  return (int)inliers.size();
}

// ORBmatcher::DescriptorDistance of two 32-byte rows (host only: no device call)
int host_descriptor_distance(const unsigned char* a, const unsigned char* b) {
  cv::Mat A(1, 32, cv::CV_8UC1, (void*)a), B(1, 32, cv::CV_8UC1, (void*)b);
  return ORBmatcher::DescriptorDistance(A, B);
}

// ORBmatcher::Match over flat keypoint arrays.  desc: [n][32]; matches / dist: [nq].  Returns the number of matches, -1 on a failure.
int host_orb_match(int nq, const float* qx, const float* qy, const int* qoct, const unsigned char* qdesc, int nt, const float* tx, const float* ty, const int* toct,
                   const unsigned char* tdesc, float nnratio, int cross_check, float window, int max_octave_diff, int max_distance, int* matches, int* dist) {
  try {
    std::vector<cv::KeyPoint> kq, kt;
    for (int i = 0; i < nq; ++i) kq.push_back(cv::KeyPoint(qx[i], qy[i], 31.f, -1, 0, qoct[i]));
    for (int i = 0; i < nt; ++i) kt.push_back(cv::KeyPoint(tx[i], ty[i], 31.f, -1, 0, toct[i]));
    cv::Mat dq(nq, 32, cv::CV_8UC1, (void*)qdesc), dt(nt, 32, cv::CV_8UC1, (void*)tdesc);
    ORBmatcher matcher(nnratio, cross_check != 0);
    std::vector<int> m, d;
    const int n = matcher.Match(kq, dq, kt, dt, window, max_octave_diff, max_distance, m, &d);
    for (int i = 0; i < nq; ++i) { matches[i] = m[i]; dist[i] = d[i]; }
    return n;
  } catch (const std::exception& e) { std::fprintf(stderr, "host_orb_match: %s\n", e.what()); return -1; }
}

// Two ORBextractor objects (2500, 1.2, 8, 20, 7) on two gray images of one size, then ORBmatcher::Match(extractor, extractor): the device-resident
// path.  *nq_out = keypoints of the first image; matches / dist: [cap].  Returns the number of matches, -1 on a failure (a too small cap included).
int host_orb_match_extractors(const unsigned char* gray_q, const unsigned char* gray_t, int w, int h, float nnratio, int cross_check, float window,
                              int max_octave_diff, int max_distance, int* matches, int* dist, int cap, int* nq_out) {
  try {
    ORBextractor eq(2500, 1.2f, 8, 20, 7), et(2500, 1.2f, 8, 20, 7);
    cv::Mat Gq(h, w, cv::CV_8UC1, (void*)gray_q), Gt(h, w, cv::CV_8UC1, (void*)gray_t), none, dq, dt;
    std::vector<cv::KeyPoint> kq, kt;
    eq(Gq, none, kq, dq); et(Gt, none, kt, dt);
    ORBmatcher matcher(nnratio, cross_check != 0);
    std::vector<int> m, d;
    const int n = matcher.Match(eq, et, window, max_octave_diff, max_distance, m, &d);
    *nq_out = (int)m.size();
    if ((int)m.size() > cap || m.size() != kq.size()) return -1;
    for (size_t i = 0; i < m.size(); ++i) { matches[i] = m[i]; dist[i] = d[i]; }
    return n;
  } catch (const std::exception& e) { std::fprintf(stderr, "host_orb_match_extractors: %s\n", e.what()); return -1; }
}

// System::TrackRGBDFromFiles on one frame's four files (identity ground-truth pose; ground-truth object rows [n_rows][row_len] as in
// host_system_track); Tcw_out 16 floats.  Returns 0, -1 when the tracker returned an empty pose, -2 on a GPU failure.
int host_system_track_files(System* s, const char* rgb, const char* depth, const char* flow, const char* mask, const float* obj_rows, int n_rows, int row_len,
                            int n_images, float* Tcw_out) {
  cv::Mat gt = cv::Mat::eye(4, 4, cv::CV_32F);
  std::vector<std::vector<float> > rows(n_rows);
  for (int i = 0; i < n_rows; ++i) rows[i].assign(obj_rows + (size_t)i * row_len, obj_rows + (size_t)(i + 1) * row_len);
  try {
    cv::Mat T = s->TrackRGBDFromFiles(rgb, depth, flow, mask, gt, rows, 0.0, n_images);
    if (T.empty()) return -1;
    std::memcpy(Tcw_out, T.data, 64);
  } catch (const std::exception& e) { std::fprintf(stderr, "host_system_track_files: %s\n", e.what()); return -2; }
  return 0;
}
// Tracking::SyncFrameState() + its converted depth map and repaired mask (mDepthMap, mSegMap; h x w each).  0, or -1 before the first frame.
int host_system_frame_images(System* s, float* depth, int* mask) {
  try {
    Tracking* T = s->tracker();
    T->SyncFrameState();
    if (T->mDepthMap.empty() || T->mSegMap.empty()) return -1;
    std::memcpy(depth, T->mDepthMap.data, T->mDepthMap.step * (size_t)T->mDepthMap.rows);
    std::memcpy(mask, T->mSegMap.data, T->mSegMap.step * (size_t)T->mSegMap.rows);
  } catch (const std::exception& e) { std::fprintf(stderr, "host_system_frame_images: %s\n", e.what()); return -1; }
  return 0;
}

// StereoMatcher::Compute on a host pair (rows left_step / right_step bytes apart).  params7: max_disparity, p1, p2, paths, uniqueness, lr_max_diff,
// subpixel.  disparity256: [h][w].  Returns the number of valid pixels, -1 on a failure.
int host_stereo_compute(const unsigned char* left, int left_step, const unsigned char* right, int right_step, int w, int h, const int* params7, float* disparity256) {
  try {
    const vdo_stereo_params p{params7[0], params7[1], params7[2], params7[3], params7[4], params7[5], params7[6]};
    StereoMatcher m(nullptr, w, h, p);
    cv::Mat L(h, w, cv::CV_8UC1, (void*)left), R(h, w, cv::CV_8UC1, (void*)right);
    L.step = (size_t)left_step; R.step = (size_t)right_step;
    int n = 0;
    cv::Mat D = m.Compute(L, R, &n);
    std::memcpy(disparity256, D.data, (size_t)w * h * sizeof(float));
    return n;
  } catch (const std::exception& e) { std::fprintf(stderr, "host_stereo_compute: %s\n", e.what()); return -1; }
}

// one TrackStereo call on host images, as host_system_track with a right image in place of the depth map
int host_system_track_stereo(System* s, const unsigned char* left, const unsigned char* right, int channels, const float* flow, int* mask, int w, int h,
                             const float* obj_rows, int n_rows, int row_len, int n_images, float* Tcw_out) {
  cv::Mat L(h, w, VDO_CV_MAKETYPE(cv::CV_8U, channels), (void*)left), R(h, w, VDO_CV_MAKETYPE(cv::CV_8U, channels), (void*)right), Fl(h, w, cv::CV_32FC2, (void*)flow),
      M(h, w, cv::CV_32SC1, mask);
  cv::Mat gt = cv::Mat::eye(4, 4, cv::CV_32F), traj;
  std::vector<std::vector<float> > rows(n_rows);
  for (int i = 0; i < n_rows; ++i) rows[i].assign(obj_rows + (size_t)i * row_len, obj_rows + (size_t)(i + 1) * row_len);
  try {
    cv::Mat T = s->TrackStereo(L, R, Fl, M, gt, rows, 0.0, traj, n_images);
    if (T.empty()) return -1;
    std::memcpy(Tcw_out, T.data, 64);
  } catch (const std::exception& e) { std::fprintf(stderr, "host_system_track_stereo: %s\n", e.what()); return -2; }
  return 0;
}

// FlowMatcher::Compute on a host pair (rows step0 / step1 bytes apart).  params6: levels, radius, window, median, fb_max_diff, subpixel.
// flow: [h][w][2], valid: [h][w] (may be null).  Returns the number of valid pixels, -1 on a failure.
int host_optflow_compute(const unsigned char* im0, int step0, const unsigned char* im1, int step1, int w, int h, const int* params6, float* flow, unsigned char* valid) {
  try {
    const vdo_optflow_params p{params6[0], params6[1], params6[2], params6[3], params6[4], params6[5]};
    FlowMatcher m(nullptr, w, h, p);
    cv::Mat A(h, w, cv::CV_8UC1, (void*)im0), B(h, w, cv::CV_8UC1, (void*)im1);
    A.step = (size_t)step0; B.step = (size_t)step1;
    int n = 0;
    cv::Mat V;
    cv::Mat F = m.Compute(A, B, valid ? &V : nullptr, &n);
    std::memcpy(flow, F.data, (size_t)w * h * 2 * sizeof(float));
    if (valid) std::memcpy(valid, V.data, (size_t)w * h);
    return n;
  } catch (const std::exception& e) { std::fprintf(stderr, "host_optflow_compute: %s\n", e.what()); return -1; }
}

// one TrackStereoPair call on host images, as host_system_track_stereo with the next left image in place of the flow image
int host_system_track_stereo_pair(System* s, const unsigned char* left, const unsigned char* right, const unsigned char* left_next, int channels, int* mask, int w, int h,
                                  const float* obj_rows, int n_rows, int row_len, int n_images, float* Tcw_out) {
  const int type = VDO_CV_MAKETYPE(cv::CV_8U, channels);
  cv::Mat L(h, w, type, (void*)left), R(h, w, type, (void*)right), N(h, w, type, (void*)left_next), M(h, w, cv::CV_32SC1, mask);
  cv::Mat gt = cv::Mat::eye(4, 4, cv::CV_32F), traj;
  std::vector<std::vector<float> > rows(n_rows);
  for (int i = 0; i < n_rows; ++i) rows[i].assign(obj_rows + (size_t)i * row_len, obj_rows + (size_t)(i + 1) * row_len);
  try {
    cv::Mat T = s->TrackStereoPair(L, R, N, M, gt, rows, 0.0, traj, n_images);
    if (T.empty()) return -1;
    std::memcpy(Tcw_out, T.data, 64);
  } catch (const std::exception& e) { std::fprintf(stderr, "host_system_track_stereo_pair: %s\n", e.what()); return -2; }
  return 0;
}

// InstanceLabeler::Compute on host images (class rows cls_step bytes apart; disparity rows disp_step_floats floats apart, null allowed when
// params4[1] is -1).  params4: connectivity, max_disp_diff, min_area, max_labels.  mask: [h][w]; counts3: n_labels, n_components, area_threshold.
// Returns n_labels, -1 on a failure.
int host_labels_compute(const unsigned char* cls, int cls_step, const float* disp, int disp_step_floats, int w, int h, const int* params4, int* mask, int* counts3) {
  try {
    const vdo_labels_params p{params4[0], params4[1], params4[2], params4[3]};
    InstanceLabeler m(nullptr, w, h, p);
    cv::Mat Cm(h, w, cv::CV_8UC1, (void*)cls), D;
    Cm.step = (size_t)cls_step;
    if (disp) { D = cv::Mat(h, w, cv::CV_32FC1, (void*)disp); D.step = (size_t)disp_step_floats * sizeof(float); }
    int counts[3] = {0, 0, 0};
    cv::Mat M = m.Compute(Cm, D, counts);
    std::memcpy(mask, M.data, (size_t)w * h * sizeof(int));
    if (counts3) std::memcpy(counts3, counts, sizeof counts);
    return counts[0];
  } catch (const std::exception& e) { std::fprintf(stderr, "host_labels_compute: %s\n", e.what()); return -1; }
}

// one TrackStereoPairSemantic call on host images, as host_system_track_stereo_pair with a class image (uint8, one channel) in place of the mask
int host_system_track_stereo_pair_semantic(System* s, const unsigned char* left, const unsigned char* right, const unsigned char* left_next, int channels,
                                           const unsigned char* classes, int w, int h, const float* obj_rows, int n_rows, int row_len, int n_images, float* Tcw_out) {
  const int type = VDO_CV_MAKETYPE(cv::CV_8U, channels);
  cv::Mat L(h, w, type, (void*)left), R(h, w, type, (void*)right), N(h, w, type, (void*)left_next), Cm(h, w, cv::CV_8UC1, (void*)classes);
  cv::Mat gt = cv::Mat::eye(4, 4, cv::CV_32F), traj;
  std::vector<std::vector<float> > rows(n_rows);
  for (int i = 0; i < n_rows; ++i) rows[i].assign(obj_rows + (size_t)i * row_len, obj_rows + (size_t)(i + 1) * row_len);
  try {
    cv::Mat T = s->TrackStereoPairSemantic(L, R, N, Cm, gt, rows, 0.0, traj, n_images);
    if (T.empty()) return -1;
    std::memcpy(Tcw_out, T.data, 64);
  } catch (const std::exception& e) { std::fprintf(stderr, "host_system_track_stereo_pair_semantic: %s\n", e.what()); return -2; }
  return 0;
}

// MotionSegmenter on host images (rows *_step_floats floats / valid_step bytes apart; valid may be null).  params: the library's struct.  ego3 (may be
// null): step, max_iterations, min_inliers, with threshold and confidence as doubles in ego2 - with them the camera motion comes from
// MotionSegmenter::EgoMotion (T16 is written, ego_counts3 filled); without them T16 is read.  cls: [h][w]; counts3: moving, static, unknown.
// Returns the moving pixel count, -1 on a failure.
int host_motionseg_compute(const float* disp0, int disp0_step_floats, const float* disp1, int disp1_step_floats, const float* flow, int flow_step_floats,
                           const unsigned char* valid, int valid_step, int w, int h, const vdo_motionseg_params* params, const int* ego3, const double* ego2, float* T16,
                           unsigned char* cls, int* counts3, int* ego_counts3) {
  try {
    MotionSegmenter m(nullptr, w, h, *params);
    cv::Mat D0(h, w, cv::CV_32FC1, (void*)disp0), D1(h, w, cv::CV_32FC1, (void*)disp1), F(h, w, cv::CV_32FC2, (void*)flow), V;
    D0.step = (size_t)disp0_step_floats * sizeof(float); D1.step = (size_t)disp1_step_floats * sizeof(float); F.step = (size_t)flow_step_floats * sizeof(float);
    if (valid) { V = cv::Mat(h, w, cv::CV_8UC1, (void*)valid); V.step = (size_t)valid_step; }
    cv::Mat T(4, 4, cv::CV_32F);
    if (ego3) {
      MotionSegmenter::EgoParams e;
      e.step = ego3[0]; e.iterations = ego3[1]; e.minInliers = ego3[2]; e.threshold = ego2[0]; e.confidence = ego2[1];
      int ec[3] = {0, 0, 0};
      T = m.EgoMotion(D0, F, V, e, ec);
      std::memcpy(T16, T.data, 64);
      if (ego_counts3) std::memcpy(ego_counts3, ec, sizeof ec);
    } else {
      std::memcpy(T.data, T16, 64);
    }
    int counts[3] = {0, 0, 0};
    cv::Mat Cm = m.Compute(D0, D1, F, V, T, counts);
    std::memcpy(cls, Cm.data, (size_t)w * h);
    if (counts3) std::memcpy(counts3, counts, sizeof counts);
    return counts[0];
  } catch (const std::exception& e) { std::fprintf(stderr, "host_motionseg_compute: %s\n", e.what()); return -1; }
}

// DenseMapper::Fuse on k host frames (depth [k][h][w] metres, mask [k][h][w] or null, Tcw [k][16] world -> camera).  params: the library's struct;
// anchor3, margin, min_weight: DenseMapper::Settings.  ply_path (may be null): DenseMapper::SavePLY after the last frame.  info2 (may be null):
// recentrings, points kept on the host.  Returns the number of points of AllPoints(), -1 on a failure.
long long host_dense_fuse(const float* depth, const int* mask, const float* Tcw, int k, int w, int h, const vdo_dense_params* params, const double* anchor3, int margin,
                          int min_weight, const char* ply_path, long long* info2) {
  try {
    DenseMapper::Settings s;
    s.params = *params; s.margin = margin; s.minWeight = min_weight;
    for (int a = 0; a < 3; ++a) s.anchor[a] = anchor3[a];
    DenseMapper m(nullptr, w, h, s);
    for (int i = 0; i < k; ++i) {
      cv::Mat D(h, w, cv::CV_32FC1, (void*)(depth + (size_t)i * w * h)), M;
      if (mask) M = cv::Mat(h, w, cv::CV_32SC1, (void*)(mask + (size_t)i * w * h));
      m.Fuse(D, M, Tcw + 16 * (size_t)i);
    }
    if (ply_path && !m.SavePLY(ply_path)) return -1;
    if (info2) { info2[0] = m.recenters(); info2[1] = (long long)m.kept().size(); }
    return (long long)m.AllPoints().size();
  } catch (const std::exception& e) { std::fprintf(stderr, "host_dense_fuse: %s\n", e.what()); return -1; }
}

// ObjectMapper::Fuse on k host frames (depth [k][h][w] metres, mask [k][h][w], Tcw [k][16] world -> camera).  Frame i has n_mot[i] motions, one after
// the other in mod_label / sem_label / H ([16] each, float).  params: every object's volume (the origin is not read); life5: MaxObjects, MinPixels,
// MinFrames, MinWeight, MaxLabels.  prefix (may be null): ObjectMapper::SaveModels after the last frame.  rows [cap][4] (may be null): mod_label, live,
// frames fused, points of every model after the last frame; counts2 (may be null): dropped, skipped.  Returns the number of models, -1 on a failure.
int host_objects_fuse(const float* depth, const int* mask, const float* Tcw, int k, int w, int h, const vdo_dense_params* params, const int* life5, const int* n_mot,
                      const int* mod_label, const int* sem_label, const float* H, const char* prefix, int cap, long long* rows, long long* counts2) {
  try {
    ObjectMapper::Settings s;
    s.params = *params; s.maxObjects = life5[0]; s.minPixels = life5[1]; s.minFrames = life5[2]; s.minWeight = life5[3]; s.maxLabels = life5[4];
    ObjectMapper m(nullptr, w, h, s);
    size_t at = 0;
    for (int i = 0; i < k; ++i) {
      cv::Mat D(h, w, cv::CV_32FC1, (void*)(depth + (size_t)i * w * h)), M(h, w, cv::CV_32SC1, (void*)(mask + (size_t)i * w * h));
      std::vector<ObjectMapper::Motion> motions((size_t)n_mot[i]);
      for (int a = 0; a < n_mot[i]; ++a, ++at) {
        motions[a].mod_label = mod_label[at]; motions[a].sem_label = sem_label[at];
        for (int q = 0; q < 16; ++q) motions[a].H[q] = (double)H[16 * at + q];
      }
      m.Fuse(i, D, M, Tcw + 16 * (size_t)i, motions);
    }
    if (prefix && !m.SaveModels(prefix)) return -1;
    const std::vector<ObjectMapper::Model> all = m.Models();
    for (size_t i = 0; rows && i < all.size() && (int)i < cap; ++i) {
      rows[4 * i] = all[i].mod_label; rows[4 * i + 1] = all[i].live ? 1 : 0; rows[4 * i + 2] = all[i].frames; rows[4 * i + 3] = (long long)all[i].points.size();
    }
    if (counts2) { counts2[0] = m.dropped(); counts2[1] = m.skipped(); }
    return (int)all.size();
  } catch (const std::exception& e) { std::fprintf(stderr, "host_objects_fuse: %s\n", e.what()); return -1; }
}

// host_dense_fuse's frames, then DenseMapper::Render at T_view (16 floats, world -> camera): depth [h][w], normals [h][w][3], weight [h][w] (may be
// null), counts3 (may be null).  view3 (may be null: DenseMapper::ViewDefaults): Near, Step, MinWeight.  0, -1 on a failure.
int host_dense_render(const float* depth, const int* mask, const float* Tcw, int k, int w, int h, const vdo_dense_params* params, const double* anchor3, int margin, int min_weight,
                      const double* view3, const float* T_view, float* out_depth, float* out_normals, int* out_weight, long long* counts3) {
  try {
    DenseMapper::Settings s;
    s.params = *params; s.margin = margin; s.minWeight = min_weight;
    for (int a = 0; a < 3; ++a) s.anchor[a] = anchor3[a];
    DenseMapper::ViewDefaults(s);
    if (view3) { s.viewNear = (float)view3[0]; s.viewStep = (float)view3[1]; s.viewMinWeight = (int)view3[2]; }
    const std::string err = DenseMapper::CheckView(s);
    if (!err.empty()) { std::fprintf(stderr, "host_dense_render: %s\n", err.c_str()); return -1; }
    DenseMapper m(nullptr, w, h, s);
    for (int i = 0; i < k; ++i) {
      cv::Mat D(h, w, cv::CV_32FC1, (void*)(depth + (size_t)i * w * h)), M;
      if (mask) M = cv::Mat(h, w, cv::CV_32SC1, (void*)(mask + (size_t)i * w * h));
      m.Fuse(D, M, Tcw + 16 * (size_t)i);
    }
    cv::Mat rd, rn, rw;
    int64_t counts[3];
    m.Render(T_view, rd, rn, out_weight ? &rw : nullptr, counts);
    std::memcpy(out_depth, rd.data, (size_t)w * h * sizeof(float));
    std::memcpy(out_normals, rn.data, (size_t)w * h * 3 * sizeof(float));
    if (out_weight) std::memcpy(out_weight, rw.data, (size_t)w * h * sizeof(int));
    if (counts3) for (int a = 0; a < 3; ++a) counts3[a] = counts[a];
    return 0;
  } catch (const std::exception& e) { std::fprintf(stderr, "host_dense_render: %s\n", e.what()); return -1; }
}

// host_dense_fuse's frames, then DenseMapper::Align of one more frame (a_depth [h][w], a_mask [h][w] or null) at T_init (16 floats, world -> camera).
// align5: Iterations (0: the class default), MaxDist (0: trunc), Subsample, MinPixels (0: the default), unused.  T_out [16]; report11: iterations,
// status, used, rms_first, rms_last, xi (6).  words (may be null): the volume afterwards, nx * ny * nz in slot order - Align changes nothing of it.
// 0, -1 on a failure.
int host_dense_align(const float* depth, const int* mask, const float* Tcw, int k, int w, int h, const vdo_dense_params* params, const double* anchor3, int margin, int min_weight,
                     const double* align5, const float* a_depth, const int* a_mask, const float* T_init, float* T_out, double* report11, unsigned int* words) {
  try {
    DenseMapper::Settings s;
    s.params = *params; s.margin = margin; s.minWeight = min_weight;
    for (int a = 0; a < 3; ++a) s.anchor[a] = anchor3[a];
    s.alignIterations = (int)align5[0]; s.alignMaxDist = (float)align5[1]; s.alignSubsample = (int)align5[2]; s.alignMinPixels = (int)align5[3];
    const std::string err = DenseMapper::CheckAlign(s);
    if (!err.empty()) { std::fprintf(stderr, "host_dense_align: %s\n", err.c_str()); return -1; }
    DenseMapper m(nullptr, w, h, s);
    for (int i = 0; i < k; ++i) {
      cv::Mat D(h, w, cv::CV_32FC1, (void*)(depth + (size_t)i * w * h)), M;
      if (mask) M = cv::Mat(h, w, cv::CV_32SC1, (void*)(mask + (size_t)i * w * h));
      m.Fuse(D, M, Tcw + 16 * (size_t)i);
    }
    cv::Mat D(h, w, cv::CV_32FC1, (void*)a_depth), M;
    if (a_mask) M = cv::Mat(h, w, cv::CV_32SC1, (void*)a_mask);
    vdo_align_report r{};
    m.Align(D, M, T_init, T_out, &r);
    report11[0] = r.iterations; report11[1] = r.status; report11[2] = (double)r.used; report11[3] = r.rms_first; report11[4] = r.rms_last;
    for (int a = 0; a < 6; ++a) report11[5 + a] = r.xi[a];
    if (words && vdo_dense_get_volume(m.handle(), words, nullptr) != VDO_OK) return -1;
    return 0;
  } catch (const std::exception& e) { std::fprintf(stderr, "host_dense_align: %s\n", e.what()); return -1; }
}

// one TrackStereoVideo call on host images: the current and the next pair (all four of `channels` channels), nothing else
int host_system_track_stereo_video(System* s, const unsigned char* left, const unsigned char* right, const unsigned char* left_next, const unsigned char* right_next, int channels,
                                   int w, int h, const float* obj_rows, int n_rows, int row_len, int n_images, float* Tcw_out) {
  const int type = VDO_CV_MAKETYPE(cv::CV_8U, channels);
  cv::Mat L(h, w, type, (void*)left), R(h, w, type, (void*)right), N(h, w, type, (void*)left_next), NR(h, w, type, (void*)right_next);
  cv::Mat gt = cv::Mat::eye(4, 4, cv::CV_32F), traj;
  std::vector<std::vector<float> > rows(n_rows);
  for (int i = 0; i < n_rows; ++i) rows[i].assign(obj_rows + (size_t)i * row_len, obj_rows + (size_t)(i + 1) * row_len);
  try {
    cv::Mat T = s->TrackStereoVideo(L, R, N, NR, gt, rows, 0.0, traj, n_images);
    if (T.empty()) return -1;
    std::memcpy(Tcw_out, T.data, 64);
  } catch (const std::exception& e) { std::fprintf(stderr, "host_system_track_stereo_video: %s\n", e.what()); return -2; }
  return 0;
}

// StereoRectifier::Rectify on n = 1..4 host images (image k: rows steps[k] bytes apart, channels[k] channels, camera cams[k], nearest[k]) in one call;
// out[k]: [height][width] of the destination.  gate_image (may be null): a [height][width] float image gated in place through camera gate_cam after the
// remap; its cleared count comes back in *n_cleared.  Returns 0, -1 on a failure.
int host_rectify_compute(const vdo_rectify_params* p, int n, const unsigned char* const* src, const int* steps, const int* channels, const int* cams, const int* nearest,
                         int rgb_order, int border, unsigned char* const* out, float* gate_image, int gate_cam, int* n_cleared) {
  try {
    StereoRectifier r(nullptr, *p);
    std::vector<cv::Mat> raw(n);
    std::vector<int> cam(cams, cams + n), nn(nearest, nearest + n);
    for (int k = 0; k < n; ++k) {
      raw[k] = cv::Mat(r.srcHeight(cams[k]), r.srcWidth(cams[k]), VDO_CV_MAKETYPE(cv::CV_8U, channels[k]), (void*)src[k]);
      raw[k].step = (size_t)steps[k];
    }
    const std::vector<cv::Mat> res = r.Rectify(raw, cam, rgb_order != 0, nn, border);
    for (int k = 0; k < n; ++k) std::memcpy(out[k], res[k].data, (size_t)r.width() * r.height());
    if (gate_image) {
      cv::Mat G(r.height(), r.width(), cv::CV_32FC1, gate_image);
      const int c = r.Gate(G, gate_cam);
      if (n_cleared) *n_cleared = c;
    }
    return 0;
  } catch (const std::exception& e) { std::fprintf(stderr, "host_rectify_compute: %s\n", e.what()); return -1; }
}

}  // extern "C"
