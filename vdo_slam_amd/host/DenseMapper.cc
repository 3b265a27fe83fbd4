// DenseMapper host class: follows the camera with the device volume (vdo_dense_recenter), keeps what leaves it as points (vdo_dense_extract) and
// fuses the frames (vdo_dense_integrate / vdo_dense_integrate_frame).
#include "DenseMapper.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

namespace VDO_SLAM {

static void die(const char* what) {   // (as MotionSegmenter.cc: a failure surfaces as an exception the flat hooks turn into a return code)
  throw std::runtime_error(std::string("VDO_SLAM::DenseMapper: ") + what + ": " + vdo_last_error());
}

DenseMapper::DenseMapper(vdo_ctx* ctx, int width, int height, const Settings& settings) : s_(settings), w_(width), h_px_(height) {
  if (vdo_dense_create(ctx ? ctx : HostContext(), width, height, &s_.params, &h_) != VDO_OK) die("vdo_dense_create");
}

DenseMapper::~DenseMapper() { vdo_dense_destroy(h_); }

void DenseMapper::origin(int32_t out[3]) const {
  if (vdo_dense_get_volume(h_, nullptr, out) != VDO_OK) die("vdo_dense_get_volume");
}

void DenseMapper::Append(const int32_t lo[3], const int32_t hi[3], Points& to) {
  int64_t n = 0;
  if (vdo_dense_extract(h_, lo, hi, s_.minWeight, 0, nullptr, nullptr, nullptr, 0, &n) != VDO_OK) die("vdo_dense_extract");
  if (n == 0) return;
  const size_t at = to.size();
  to.xyz.resize(3 * (at + (size_t)n)); to.grad.resize(3 * (at + (size_t)n)); to.weight.resize(at + (size_t)n);
  if (vdo_dense_extract(h_, lo, hi, s_.minWeight, n, to.xyz.data() + 3 * at, to.grad.data() + 3 * at, to.weight.data() + at, 0, &n) != VDO_OK) die("vdo_dense_extract");
}

void DenseMapper::Follow(const float Tcw[16]) {
  const int32_t* n = s_.params.n;
  const double voxel = (double)s_.params.voxel;
  int32_t o[3], c[3], want[3];
  origin(o);
  bool move = !started_;
  for (int a = 0; a < 3; ++a) {
    // the camera centre -R^T t, one axis at a time
    const double centre = -((double)Tcw[a] * (double)Tcw[3] + (double)Tcw[4 + a] * (double)Tcw[7] + (double)Tcw[8 + a] * (double)Tcw[11]);
    const double v = std::floor(centre / voxel);
    if (!(std::fabs(v) < 1e9)) throw std::runtime_error("VDO_SLAM::DenseMapper: the camera pose is not finite");
    const int target = (int)std::floor(s_.anchor[a] * n[a]);
    c[a] = (int32_t)v;
    want[a] = c[a] - target;
    if (std::abs((long long)c[a] - ((long long)o[a] + target)) > s_.margin) move = true;
  }
  if (!move) return;
  if (started_) {
    bool all = false;
    for (int a = 0; a < 3; ++a) all = all || std::abs((long long)want[a] - o[a]) >= n[a];
    int32_t lo[3] = {o[0], o[1], o[2]}, hi[3] = {o[0] + n[0], o[1] + n[1], o[2] + n[2]};
    if (all) {
      Append(lo, hi, kept_);
    } else {
      for (int a = 0; a < 3; ++a) {
        const int d = want[a] - o[a];
        if (d == 0) continue;
        int32_t blo[3] = {lo[0], lo[1], lo[2]}, bhi[3] = {hi[0], hi[1], hi[2]};
        if (d > 0) { bhi[a] = o[a] + d; lo[a] = o[a] + d; }
        else { blo[a] = o[a] + n[a] + d; hi[a] = o[a] + n[a] + d; }
        Append(blo, bhi, kept_);
      }
    }
    ++recenters_;
  }
  if (vdo_dense_recenter(h_, want) != VDO_OK) die("vdo_dense_recenter");
  started_ = true;
}

void DenseMapper::FuseFrame(const vdo_frame_images* frame, const float Tcw[16], int64_t counts[3]) {
  Follow(Tcw);
  int64_t out[3] = {0, 0, 0};
  if (vdo_dense_integrate_frame(h_, frame, Tcw, out) != VDO_OK) die("vdo_dense_integrate_frame");
  if (counts) for (int k = 0; k < 3; ++k) counts[k] = out[k];
}

void DenseMapper::Fuse(const cv::Mat& depth, const cv::Mat& mask, const float Tcw[16], int64_t counts[3]) {
  auto image = [&](const cv::Mat& m, int type) { return !m.empty() && m.rows == h_px_ && m.cols == w_ && m.depth() == type && m.channels() == 1 && m.step % 4 == 0; };
  if (!image(depth, cv::CV_32F)) throw std::runtime_error("VDO_SLAM::DenseMapper: depth must be CV_32FC1 of the mapper's size");
  if (!mask.empty() && !image(mask, cv::CV_32S)) throw std::runtime_error("VDO_SLAM::DenseMapper: mask must be empty or CV_32SC1 of the mapper's size");
  Follow(Tcw);
  int64_t out[3] = {0, 0, 0};
  if (vdo_dense_integrate(h_, (const float*)depth.data, (int64_t)(depth.step / 4), mask.empty() ? nullptr : (const int32_t*)mask.data, mask.empty() ? 0 : (int64_t)(mask.step / 4), 0, Tcw,
                          out) != VDO_OK)
    die("vdo_dense_integrate");
  if (counts) for (int k = 0; k < 3; ++k) counts[k] = out[k];
}

DenseMapper::Points DenseMapper::AllPoints() {
  Points all = kept_;
  int32_t o[3];
  origin(o);
  const int32_t hi[3] = {o[0] + s_.params.n[0], o[1] + s_.params.n[1], o[2] + s_.params.n[2]};
  Append(o, hi, all);
  return all;
}

bool DenseMapper::SavePLY(const std::string& path) {
  const Points all = AllPoints();
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  std::fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment static scene, TSDF zero crossings\nelement vertex %zu\n", all.size());
  std::fprintf(f, "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty int weight\nend_header\n");
  bool ok = true;
  for (size_t i = 0; i < all.size() && ok; ++i) {
    const double g[3] = {(double)all.grad[3 * i], (double)all.grad[3 * i + 1], (double)all.grad[3 * i + 2]};
    const double len = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    char rec[28];                                                          // (x86-64 is little-endian: the records are written as they lie)
    float v[6] = {all.xyz[3 * i], all.xyz[3 * i + 1], all.xyz[3 * i + 2], 0.f, 0.f, 0.f};
    if (len > 0) for (int k = 0; k < 3; ++k) v[3 + k] = (float)(g[k] / len);
    std::memcpy(rec, v, 24); std::memcpy(rec + 24, &all.weight[i], 4);
    ok = std::fwrite(rec, 1, 28, f) == 28;
  }
  return std::fclose(f) == 0 && ok;
}

}  // namespace VDO_SLAM
