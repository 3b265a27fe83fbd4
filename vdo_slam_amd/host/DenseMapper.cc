// DenseMapper host class: follows the camera with the device volume (vdo_dense_recenter), keeps what leaves it as points (vdo_dense_extract) and
// fuses the frames (vdo_dense_integrate / vdo_dense_integrate_frame).
#include "DenseMapper.h"

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

namespace VDO_SLAM {

static void die(const char* what) {   // (as MotionSegmenter.cc: a failure surfaces as an exception the flat hooks turn into a return code)
  throw std::runtime_error(std::string("VDO_SLAM::DenseMapper: ") + what + ": " + vdo_last_error());
}

DenseMapper::DenseMapper(vdo_ctx* ctx, int width, int height, const Settings& settings) : ctx_(ctx ? ctx : HostContext()), s_(settings), w_(width), h_px_(height) {
  if (vdo_dense_create(ctx_, width, height, &s_.params, &h_) != VDO_OK) die("vdo_dense_create");
  if (s_.mesh) {
    const vdo_mesh_params mp{{s_.params.n[0], s_.params.n[1], s_.params.n[2]}, 1 << 20, 1 << 21};
    if (vdo_mesh_create(ctx_, &mp, &mesher_) != VDO_OK) { vdo_dense_destroy(h_); die("vdo_mesh_create"); }
  }
  if (s_.colour) {
    if (s_.colourBand == 0.f) s_.colourBand = s_.params.trunc / 2.f;
    if (s_.colourMaxWeight == 0) s_.colourMaxWeight = s_.params.max_weight;
    const std::string err = CheckColour(s_);
    const vdo_colour_params cp{s_.colourBand, s_.colourMaxWeight, 1 << 20};
    if (!err.empty() || vdo_colour_create(h_, &cp, &colour_) != VDO_OK) {
      vdo_mesh_destroy(mesher_); vdo_dense_destroy(h_);
      if (!err.empty()) throw std::runtime_error("VDO_SLAM::DenseMapper: " + err);
      die("vdo_colour_create");
    }
    kept_.coloured = keptMeshV_.coloured = true;            // what is copied from them and appended to carries colours, also while it is empty
  }
  if (s_.distance) {
    if (s_.distanceMinWeight == 0) s_.distanceMinWeight = s_.minWeight;
    const std::string err = CheckDistance(s_);
    const vdo_distance_params dp{{s_.params.n[0], s_.params.n[1], s_.params.n[2]}};
    if (!err.empty() || vdo_distance_create(ctx_, &dp, &dist_) != VDO_OK) {
      vdo_colour_destroy(colour_); vdo_mesh_destroy(mesher_); vdo_dense_destroy(h_);
      if (!err.empty()) throw std::runtime_error("VDO_SLAM::DenseMapper: " + err);
      die("vdo_distance_create");
    }
  }
}

DenseMapper::~DenseMapper() {
  vdo_distance_destroy(dist_);
  vdo_colour_destroy(colour_);                            // the colourer borrows the map
  vdo_mesh_destroy(mesher_);
  vdo_photo_destroy(photo_);
  vdo_align_destroy(align_);
  vdo_raycast_destroy(view_);                             // the view borrows the map
  vdo_dense_destroy(h_);
}

void DenseMapper::ViewDefaults(Settings& s) {
  const vdo_dense_params& p = s.params;
  s.viewNear = p.min_depth > p.voxel ? p.min_depth : p.voxel;
  s.viewStep = p.trunc / 2.f;
  s.viewMinWeight = s.minWeight;
}

std::string DenseMapper::CheckView(Settings& s) {
  const vdo_dense_params& p = s.params;
  if (!std::isfinite(s.viewNear) || !(s.viewNear >= 0.f)) return "settings: Dense.View.Near must not be negative";
  if (!(s.viewNear < p.max_depth)) return "settings: Dense.View.Near must be below Dense.MaxDepth";
  if (!std::isfinite(s.viewStep) || !(s.viewStep > 0.f)) return "settings: Dense.View.Step must be positive";
  if (s.viewMinWeight < 1 || s.viewMinWeight > 255) return "settings: Dense.View.MinWeight outside 1..255";
  const double steps = std::ceil(((double)p.max_depth - (double)s.viewNear) / (double)s.viewStep) + 1.0;
  if (!(steps <= 65536.0)) return "settings: Dense.View.Step: more than 65536 samples per ray between Dense.View.Near and Dense.MaxDepth";
  s.viewSteps = (int)steps;
  return "";
}

std::string DenseMapper::CheckAlign(const Settings& s) {
  if (s.alignIterations < 0 || s.alignIterations > 64) return "settings: Dense.Align.Iterations outside 0..64";
  if (!std::isfinite(s.alignMaxDist) || !(s.alignMaxDist >= 0.f)) return "settings: Dense.Align.MaxDist must be finite and not negative (0 stands for Dense.Truncation)";
  if (s.alignSubsample < 1 || s.alignSubsample > 8) return "settings: Dense.Align.Subsample outside 1..8";
  if (s.alignMinPixels != 0 && s.alignMinPixels < 6) return "settings: Dense.Align.MinPixels must be at least 6";
  return "";
}

std::string DenseMapper::CheckAlignPhoto(const Settings& s) {
  if (!std::isfinite(s.alignPhoto) || !(s.alignPhoto >= 0.f)) return "settings: Dense.Align.Photo must be finite and not negative (0: off)";
  if (!std::isfinite(s.alignPhotoMaxDiff) || !(s.alignPhotoMaxDiff > 0.f) || !(s.alignPhotoMaxDiff <= 255.f)) return "settings: Dense.Align.Photo.MaxDiff outside (0, 255]";
  if (s.alignPhotoMinPixels != 0 && s.alignPhotoMinPixels < 6) return "settings: Dense.Align.Photo.MinPixels must be at least 6";
  return "";
}

int DenseMapper::AlignPhotoMinPixels(const Settings& s, int width, int height) { return s.alignPhotoMinPixels > 0 ? s.alignPhotoMinPixels : AlignMinPixels(s, width, height); }

std::string DenseMapper::CheckColour(const Settings& s) {
  if (!std::isfinite(s.colourBand) || !(s.colourBand > 0.f)) return "settings: Dense.Colour.Band must be positive";
  if (!(s.colourBand <= s.params.trunc)) return "settings: Dense.Colour.Band must not exceed Dense.Truncation";
  if (s.colourMaxWeight < 1 || s.colourMaxWeight > 255) return "settings: Dense.Colour.MaxWeight outside 1..255";
  if (s.colourMinWeight < 1 || s.colourMinWeight > 255) return "settings: Dense.Colour.MinWeight outside 1..255";
  return "";
}

int DenseMapper::DistanceRadiusVoxels(const Settings& s) {
  if (!std::isfinite(s.distanceRadius) || !(s.distanceRadius > 0.f)) return 0;
  const double v = std::ceil((double)s.distanceRadius / (double)s.params.voxel);
  return v >= 1.0 && v <= 8191.0 ? (int)v : 0;
}

std::string DenseMapper::CheckDistance(const Settings& s) {
  if (!std::isfinite(s.distanceRadius) || !(s.distanceRadius > 0.f)) return "settings: Dense.Distance.Radius must be positive";
  if (DistanceRadiusVoxels(s) == 0) return "settings: Dense.Distance.Radius outside 1..8191 voxels of Dense.VoxelSize";
  if (s.distanceMinWeight != 0 && (s.distanceMinWeight < 1 || s.distanceMinWeight > 255)) return "settings: Dense.Distance.MinWeight outside 1..255";
  return "";
}

void DenseMapper::Distance(const int32_t lo[3], const int32_t hi[3], int64_t counts[3]) {
  if (!dist_) throw std::runtime_error("VDO_SLAM::DenseMapper: Distance without Dense.Distance");
  const bool whole = !lo && !hi;
  int32_t o[3], wlo[3], whi[3];
  if (whole) {
    origin(o);
    for (int a = 0; a < 3; ++a) { wlo[a] = o[a]; whi[a] = o[a] + s_.params.n[a]; }
  } else if (!lo || !hi) {
    throw std::runtime_error("VDO_SLAM::DenseMapper: Distance takes both corners of a box or neither");
  }
  int64_t out[3] = {0, 0, 0};
  if (vdo_distance_compute(dist_, h_, whole ? wlo : lo, whole ? whi : hi, s_.distanceMinWeight, DistanceRadiusVoxels(s_), out) != VDO_OK) die("vdo_distance_compute");
  ++distComputes_;
  distGeneration_ = whole ? generation_ : 0;
  if (counts) for (int k = 0; k < 3; ++k) counts[k] = out[k];
}

void DenseMapper::Clearance(const float* xyz, int64_t n, uint32_t* words) {
  if (!dist_) throw std::runtime_error("VDO_SLAM::DenseMapper: Clearance without Dense.Distance");
  if (distGeneration_ != generation_) Distance(nullptr, nullptr);
  int64_t inside = 0;
  if (vdo_distance_sample(dist_, n, xyz, words, 0, &inside) != VDO_OK) die("vdo_distance_sample");
}

int DenseMapper::AlignMinPixels(const Settings& s, int width, int height) {
  if (s.alignMinPixels > 0) return s.alignMinPixels;
  const int64_t ws = (width + s.alignSubsample - 1) / s.alignSubsample, hs = (height + s.alignSubsample - 1) / s.alignSubsample;
  const int64_t n = ws * hs / 16;
  return n < 6 ? 6 : (int)n;
}

void DenseMapper::EnsureView() {
  if (view_) return;
  if (s_.viewSteps == 0) ViewDefaults(s_);
  const std::string err = CheckView(s_);
  if (!err.empty()) throw std::runtime_error("VDO_SLAM::DenseMapper: " + err);
  const vdo_raycast_params rp{{s_.params.K[0], s_.params.K[1], s_.params.K[2], s_.params.K[3]}, s_.viewNear, s_.viewStep, s_.viewSteps, s_.viewMinWeight};
  if (vdo_raycast_create(h_, w_, h_px_, &rp, &view_) != VDO_OK) die("vdo_raycast_create");
  grad_.resize((size_t)w_ * h_px_ * 3);
}

void DenseMapper::EnsureAligner(const float Tcw_init[16]) {
  EnsureView();
  if (!align_) {
    const std::string err = CheckAlign(s_);
    if (!err.empty()) throw std::runtime_error("VDO_SLAM::DenseMapper: " + err);
    const vdo_dense_params& p = s_.params;
    const vdo_align_params ap{{p.K[0], p.K[1], p.K[2], p.K[3]}, p.min_depth, p.max_depth, s_.alignMaxDist > 0.f ? s_.alignMaxDist : p.trunc, s_.alignSubsample,
                              AlignMinPixels(s_, w_, h_px_), s_.alignIterations > 0 ? s_.alignIterations : 10, 1e-5f, 0};
    if (vdo_align_create(ctx_, w_, h_px_, &ap, &align_) != VDO_OK) die("vdo_align_create");
  }
  if (vdo_align_set_model_from_view(align_, view_, Tcw_init, nullptr) != VDO_OK) die("vdo_align_set_model_from_view");
}

void DenseMapper::Align(const cv::Mat& depth, const cv::Mat& mask, const float Tcw_init[16], float Tcw_out[16], vdo_align_report* report) {
  auto image = [&](const cv::Mat& m, int type) { return !m.empty() && m.rows == h_px_ && m.cols == w_ && m.depth() == type && m.channels() == 1 && m.step % 4 == 0; };
  if (!image(depth, cv::CV_32F)) throw std::runtime_error("VDO_SLAM::DenseMapper: depth must be CV_32FC1 of the mapper's size");
  if (!mask.empty() && !image(mask, cv::CV_32S)) throw std::runtime_error("VDO_SLAM::DenseMapper: mask must be empty or CV_32SC1 of the mapper's size");
  EnsureAligner(Tcw_init);
  if (vdo_align_solve(align_, (const float*)depth.data, (int64_t)(depth.step / 4), mask.empty() ? nullptr : (const int32_t*)mask.data, mask.empty() ? 0 : (int64_t)(mask.step / 4), 0,
                      Tcw_init, Tcw_out, report, nullptr) != VDO_OK)
    die("vdo_align_solve");
}

void DenseMapper::AlignFrame(const vdo_frame_images* frame, const float Tcw_init[16], float Tcw_out[16], vdo_align_report* report) {
  EnsureAligner(Tcw_init);
  if (vdo_align_solve_frame(align_, frame, Tcw_init, Tcw_out, report, nullptr) != VDO_OK) die("vdo_align_solve_frame");
}

void DenseMapper::EnsurePhoto(const Image& image) {
  if (!(s_.alignPhoto > 0.f)) throw std::runtime_error("VDO_SLAM::DenseMapper: AlignPhoto without Dense.Align.Photo");
  if (!image.data) throw std::runtime_error("VDO_SLAM::DenseMapper: AlignPhoto without an image");
  if (!photo_) {
    const std::string err = CheckAlignPhoto(s_);
    if (!err.empty()) throw std::runtime_error("VDO_SLAM::DenseMapper: " + err);
    const vdo_dense_params& p = s_.params;
    const vdo_photo_params pp{{p.K[0], p.K[1], p.K[2], p.K[3]}, p.min_depth, p.max_depth, s_.alignMaxDist > 0.f ? s_.alignMaxDist : p.trunc, s_.alignPhotoMaxDiff, s_.alignSubsample,
                              AlignPhotoMinPixels(s_, w_, h_px_), s_.alignIterations > 0 ? s_.alignIterations : 10, 1e-5f, 0};
    if (vdo_photo_create(ctx_, w_, h_px_, &pp, &photo_) != VDO_OK) die("vdo_photo_create");
  }
  if (vdo_photo_set_image(photo_, image.data, image.step, image.channels, image.bgr ? 1 : 0, image.device ? 1 : 0) != VDO_OK) die("vdo_photo_set_image");
}

void DenseMapper::SolvePhoto(const vdo_frame_images* frame, const cv::Mat* depth, const cv::Mat* mask, const float Tcw_init[16], float Tcw_out[16], vdo_photo_report* report) {
  const float* d = frame ? nullptr : (const float*)depth->data;
  const int64_t ds = frame ? 0 : (int64_t)(depth->step / 4);
  const int32_t* m = frame || mask->empty() ? nullptr : (const int32_t*)mask->data;
  const int64_t ms = m ? (int64_t)(mask->step / 4) : 0;
  vdo_photo_report rep{};
  bool joint = photoModel_;
  if (joint) {
    const int rc = frame ? vdo_photo_solve_frame(photo_, align_, frame, (double)s_.alignPhoto, Tcw_init, Tcw_out, &rep, nullptr)
                         : vdo_photo_solve(photo_, align_, d, ds, m, ms, 0, (double)s_.alignPhoto, Tcw_init, Tcw_out, &rep, nullptr);
    if (rc != VDO_OK) die("vdo_photo_solve");
    joint = rep.status != 1;
  }
  if (!joint) {                                            // the geometry alone, as Align does it
    vdo_align_report a{};
    const int rc = frame ? vdo_align_solve_frame(align_, frame, Tcw_init, Tcw_out, &a, nullptr) : vdo_align_solve(align_, d, ds, m, ms, 0, Tcw_init, Tcw_out, &a, nullptr);
    if (rc != VDO_OK) die("vdo_align_solve");
    rep = vdo_photo_report{};
    rep.iterations = a.iterations; rep.status = a.status; rep.used_geo = a.used; rep.rms_geo_first = a.rms_first; rep.rms_geo_last = a.rms_last;
    for (int k = 0; k < 6; ++k) rep.xi[k] = a.xi[k];
  }
  if (report) *report = rep;
}

void DenseMapper::AlignPhoto(const cv::Mat& depth, const cv::Mat& mask, const Image& image, const float Tcw_init[16], float Tcw_out[16], vdo_photo_report* report) {
  auto img = [&](const cv::Mat& m, int type) { return !m.empty() && m.rows == h_px_ && m.cols == w_ && m.depth() == type && m.channels() == 1 && m.step % 4 == 0; };
  if (!img(depth, cv::CV_32F)) throw std::runtime_error("VDO_SLAM::DenseMapper: depth must be CV_32FC1 of the mapper's size");
  if (!mask.empty() && !img(mask, cv::CV_32S)) throw std::runtime_error("VDO_SLAM::DenseMapper: mask must be empty or CV_32SC1 of the mapper's size");
  EnsurePhoto(image);
  EnsureAligner(Tcw_init);
  SolvePhoto(nullptr, &depth, &mask, Tcw_init, Tcw_out, report);
}

void DenseMapper::AlignPhotoFrame(const vdo_frame_images* frame, const Image& image, const float Tcw_init[16], float Tcw_out[16], vdo_photo_report* report) {
  EnsurePhoto(image);
  EnsureAligner(Tcw_init);
  SolvePhoto(frame, nullptr, nullptr, Tcw_init, Tcw_out, report);
}

void DenseMapper::KeepPhotoModel(const vdo_frame_images* frame, const float Tcw[16]) {
  if (!photo_) throw std::runtime_error("VDO_SLAM::DenseMapper: KeepPhotoModel before AlignPhoto");
  if (vdo_photo_keep_as_model_frame(photo_, frame, Tcw) != VDO_OK) die("vdo_photo_keep_as_model_frame");
  photoModel_ = true;
}

void DenseMapper::Render(const float Tcw[16], cv::Mat& depth, cv::Mat& normals, cv::Mat* weight, int64_t counts[3]) {
  EnsureView();
  depth.create(h_px_, w_, cv::CV_32FC1);
  normals.create(h_px_, w_, cv::CV_32FC3);
  if (weight) weight->create(h_px_, w_, cv::CV_32SC1);
  int64_t out[3] = {0, 0, 0};
  if (vdo_raycast_render(view_, Tcw, (float*)depth.data, grad_.data(), weight ? (int32_t*)weight->data : nullptr, 0, out) != VDO_OK) die("vdo_raycast_render");
  float* nrm = (float*)normals.data;
  for (size_t i = 0; i < (size_t)w_ * h_px_; ++i) {
    const double g[3] = {(double)grad_[3 * i], (double)grad_[3 * i + 1], (double)grad_[3 * i + 2]};
    const double len = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    for (int k = 0; k < 3; ++k) nrm[3 * i + k] = len > 0 ? (float)(g[k] / len) : 0.f;
  }
  if (counts) for (int k = 0; k < 3; ++k) counts[k] = out[k];
}

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
  Colour(to, at);
}

void DenseMapper::Colour(Points& p, size_t from) {
  if (!colour_) return;
  p.coloured = true;
  const size_t n = p.size();
  p.rgba.resize(4 * n);
  if (n == from) return;
  int64_t coloured = 0;
  if (vdo_colour_sample(colour_, (int64_t)(n - from), p.xyz.data() + 3 * from, s_.colourMinWeight, p.rgba.data() + 4 * from, 0, &coloured) != VDO_OK) die("vdo_colour_sample");
}

void DenseMapper::AppendMeshOf(vdo_mesh* mesher, vdo_dense* map, const int32_t lo[3], const int32_t hi[3], int outside, int min_weight, int64_t guess[2], Points& v,
                               std::vector<int32_t>& tri) {
  const size_t at = v.size(), tat = tri.size();
  int64_t c[2] = {0, 0};
  for (int pass = 0; pass < 2; ++pass) {
    const size_t cv = (size_t)guess[0], ct = (size_t)guess[1];
    v.xyz.resize(3 * (at + cv)); v.grad.resize(3 * (at + cv)); v.weight.resize(at + cv); tri.resize(tat + 3 * ct);
    if (vdo_mesh_extract(mesher, map, lo, hi, outside, min_weight, guess[0], cv ? v.xyz.data() + 3 * at : nullptr, cv ? v.grad.data() + 3 * at : nullptr,
                         cv ? v.weight.data() + at : nullptr, guess[1], ct ? tri.data() + tat : nullptr, 0, c) != VDO_OK)
      die("vdo_mesh_extract");
    const bool fits = c[0] <= guess[0] && c[1] <= guess[1];
    if (c[0] > guess[0]) guess[0] = c[0] + c[0] / 4;                          // room for a surface that grows from call to call
    if (c[1] > guess[1]) guess[1] = c[1] + c[1] / 4;
    if (fits) break;
  }
  const size_t nv = (size_t)c[0], nt = (size_t)c[1];
  if (at + nv > (size_t)INT32_MAX) throw std::runtime_error("VDO_SLAM::DenseMapper: the mesh passes 2^31 - 1 vertices");
  v.xyz.resize(3 * (at + nv)); v.grad.resize(3 * (at + nv)); v.weight.resize(at + nv); tri.resize(tat + 3 * nt);
  for (size_t i = tat; i < tri.size(); ++i) tri[i] += (int32_t)at;             // the piece's indices start at the running vertex count
}

void DenseMapper::AppendMesh(const int32_t lo[3], const int32_t hi[3], int outside, Points& v, std::vector<int32_t>& tri) {
  const size_t at = v.size();
  AppendMeshOf(mesher_, h_, lo, hi, outside, s_.minWeight, meshGuess_, v, tri);
  Colour(v, at);
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
  if (started_ && mesher_) {
    // the staying box: what both the old and the new volume cover (empty after a move of n or more, and then everything is kept)
    int32_t slo[3], shi[3];
    bool none = false;
    for (int a = 0; a < 3; ++a) {
      slo[a] = o[a] > want[a] ? o[a] : want[a]; shi[a] = (o[a] < want[a] ? o[a] : want[a]) + n[a];
      none = none || shi[a] <= slo[a];
    }
    if (none) for (int a = 0; a < 3; ++a) slo[a] = shi[a] = 0;
    AppendMesh(slo, shi, 1, keptMeshV_, keptMeshT_);
  }
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
  ++generation_;
}

void DenseMapper::FuseFrame(const vdo_frame_images* frame, const float Tcw[16], int64_t counts[3]) {
  Follow(Tcw);
  int64_t out[3] = {0, 0, 0};
  if (vdo_dense_integrate_frame(h_, frame, Tcw, out) != VDO_OK) die("vdo_dense_integrate_frame");
  ++generation_;
  lastFrame_ = frame;
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
  ++generation_;
  lastFrame_ = nullptr;
  if (counts) for (int k = 0; k < 3; ++k) counts[k] = out[k];
}

void DenseMapper::FuseColour(const Image& im, const float Tcw[16], int64_t counts[3]) {
  if (!colour_) throw std::runtime_error("VDO_SLAM::DenseMapper: FuseColour without Dense.Colour");
  if (!lastFrame_) throw std::runtime_error("VDO_SLAM::DenseMapper: FuseColour follows a FuseFrame");
  int64_t out[3] = {0, 0, 0};
  if (vdo_colour_integrate_frame(colour_, lastFrame_, im.data, im.step, im.channels, im.bgr ? 1 : 0, im.device ? 1 : 0, 0, Tcw, out) != VDO_OK) die("vdo_colour_integrate_frame");
  if (counts) for (int k = 0; k < 3; ++k) counts[k] = out[k];
}

void DenseMapper::RenderColour(const float Tcw[16], cv::Mat& rgba) {
  if (!colour_) throw std::runtime_error("VDO_SLAM::DenseMapper: RenderColour without Dense.Colour");
  cv::Mat depth, normals;
  Render(Tcw, depth, normals);
  rgba.create(h_px_, w_, cv::CV_8UC4);
  int64_t out[2] = {0, 0};
  if (vdo_colour_render(colour_, (const float*)depth.data, w_, h_px_, s_.params.K, Tcw, s_.colourMinWeight, rgba.data, 0, out) != VDO_OK) die("vdo_colour_render");
}

DenseMapper::Points DenseMapper::AllPoints() {
  Points all = kept_;
  int32_t o[3];
  origin(o);
  const int32_t hi[3] = {o[0] + s_.params.n[0], o[1] + s_.params.n[1], o[2] + s_.params.n[2]};
  Append(o, hi, all);
  return all;
}

void DenseMapper::Mesh(Points& v, std::vector<int32_t>& tri) {
  if (!mesher_) throw std::runtime_error("VDO_SLAM::DenseMapper: Mesh without Dense.Mesh");
  v = keptMeshV_; tri = keptMeshT_;
  int32_t o[3];
  origin(o);
  const int32_t hi[3] = {o[0] + s_.params.n[0], o[1] + s_.params.n[1], o[2] + s_.params.n[2]};
  AppendMesh(o, hi, 0, v, tri);
}

// one vertex record as SavePLY and SaveMeshPLY write it: x, y, z, the gradient normalised in double and narrowed (or 0), the weight and, when the
// points carry colours (the caller decides, once per file), red, green, blue, alpha
static bool write_vertex(FILE* f, const DenseMapper::Points& p, size_t i, bool coloured) {
  const double g[3] = {(double)p.grad[3 * i], (double)p.grad[3 * i + 1], (double)p.grad[3 * i + 2]};
  const double len = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
  char rec[32];                                                            // (x86-64 is little-endian: the records are written as they lie)
  float v[6] = {p.xyz[3 * i], p.xyz[3 * i + 1], p.xyz[3 * i + 2], 0.f, 0.f, 0.f};
  if (len > 0) for (int k = 0; k < 3; ++k) v[3 + k] = (float)(g[k] / len);
  std::memcpy(rec, v, 24); std::memcpy(rec + 24, &p.weight[i], 4);
  if (coloured) std::memcpy(rec + 28, &p.rgba[4 * i], 4);
  const size_t len_rec = coloured ? 32 : 28;
  return std::fwrite(rec, 1, len_rec, f) == len_rec;
}

static const char* kVertexProperties = "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty int weight\n";
static const char* kColourProperties = "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n";

bool DenseMapper::SaveMeshPLY(const std::string& path) {
  Points v;
  std::vector<int32_t> tri;
  Mesh(v, tri);
  return WriteMeshPLY(path, v, tri);
}

bool DenseMapper::WriteMeshPLY(const std::string& path, const Points& v, const std::vector<int32_t>& tri) {
  if (v.coloured && v.rgba.size() != 4 * v.size()) return false;
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  std::fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\n", v.size());
  std::fprintf(f, "%s%s", kVertexProperties, v.coloured ? kColourProperties : "");
  std::fprintf(f, "element face %zu\nproperty list uchar int vertex_indices\nend_header\n", tri.size() / 3);
  bool ok = true;
  for (size_t i = 0; i < v.size() && ok; ++i) ok = write_vertex(f, v, i, v.coloured);
  for (size_t t = 0; t < tri.size() / 3 && ok; ++t) {
    char rec[13] = {3};
    std::memcpy(rec + 1, &tri[3 * t], 12);
    ok = std::fwrite(rec, 1, 13, f) == 13;
  }
  return std::fclose(f) == 0 && ok;
}

bool DenseMapper::SavePLY(const std::string& path) {
  const Points all = AllPoints();
  if (all.coloured && all.rgba.size() != 4 * all.size()) return false;
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  std::fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment static scene, TSDF zero crossings\nelement vertex %zu\n", all.size());
  std::fprintf(f, "%s%send_header\n", kVertexProperties, all.coloured ? kColourProperties : "");
  bool ok = true;
  for (size_t i = 0; i < all.size() && ok; ++i) ok = write_vertex(f, all, i, all.coloured);
  return std::fclose(f) == 0 && ok;
}

}  // namespace VDO_SLAM
