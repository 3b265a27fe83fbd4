// ObjectMapper host class: the lifecycle of the per-object volumes over vdo_objects_* (label statistics, one batched label-selecting fusion per
// frame), vdo_dense_* (the volumes, their extraction and clearing) and vdo_raycast_* (views of a live model).
#include "ObjectMapper.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace VDO_SLAM {

static void die(const char* what) {   // (as DenseMapper.cc: a failure surfaces as an exception the flat hooks turn into a return code)
  throw std::runtime_error(std::string("VDO_SLAM::ObjectMapper: ") + what + ": " + vdo_last_error());
}

// C = A * B, every entry ((a0*b0 + a1*b1) + a2*b2) + a3*b3 (this file is built without contraction)
static void mul44d(const double* A, const double* B, double* C) {
  double out[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) out[4 * i + j] = ((A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j]) + A[4 * i + 3] * B[12 + j];
  std::memcpy(C, out, sizeof out);
}

std::string ObjectMapper::Check(const Settings& s) {
  if (s.maxObjects < 1 || s.maxObjects > 64) return "settings: Dense.Objects.MaxObjects outside 1..64";
  if (s.minPixels < 1) return "settings: Dense.Objects.MinPixels must be at least 1";
  if (s.minFrames < 1) return "settings: Dense.Objects.MinFrames must be at least 1";
  if (s.minWeight < 1 || s.minWeight > 255) return "settings: Dense.Objects.MinWeight outside 1..255";
  return "";
}

ObjectMapper::ObjectMapper(vdo_ctx* ctx, int width, int height, const Settings& settings) : ctx_(ctx ? ctx : HostContext()), s_(settings), w_(width), h_px_(height) {
  const std::string err = Check(s_);
  if (!err.empty()) throw std::runtime_error("VDO_SLAM::ObjectMapper: " + err);
  for (int a = 0; a < 3; ++a) s_.params.origin[a] = -(s_.params.n[a] / 2);
  const vdo_dense_params& p = s_.params;
  const vdo_objects_params op{{p.K[0], p.K[1], p.K[2], p.K[3]}, p.min_depth, p.max_depth, s_.maxLabels, s_.maxObjects};
  if (vdo_objects_create(ctx_, width, height, &op, &stage_) != VDO_OK) die("vdo_objects_create");
  stats_.assign((size_t)(s_.maxLabels + 1) * 8, 0);
  if (s_.mesh) {
    const vdo_mesh_params mp{{p.n[0], p.n[1], p.n[2]}, 1 << 18, 1 << 19};
    if (vdo_mesh_create(ctx_, &mp, &mesher_) != VDO_OK) { vdo_objects_destroy(stage_); die("vdo_mesh_create"); }
  }
}

ObjectMapper::~ObjectMapper() {
  for (Live& m : live_) pool_.push_back(m.slot);
  for (Slot& s : pool_) { vdo_raycast_destroy(s.view); vdo_dense_destroy(s.map); }      // the view borrows the map
  vdo_mesh_destroy(mesher_);
  vdo_objects_destroy(stage_);
}

void ObjectMapper::ExtractMesh(vdo_dense* map, DenseMapper::Points& v, std::vector<int32_t>& tri) {
  const vdo_dense_params& p = s_.params;
  const int32_t lo[3] = {p.origin[0], p.origin[1], p.origin[2]}, hi[3] = {p.origin[0] + p.n[0], p.origin[1] + p.n[1], p.origin[2] + p.n[2]};
  v = DenseMapper::Points(); tri.clear();
  DenseMapper::AppendMeshOf(mesher_, map, lo, hi, 0, s_.minWeight, meshGuess_, v, tri);
}

void ObjectMapper::Extract(vdo_dense* map, DenseMapper::Points& to) {
  const vdo_dense_params& p = s_.params;
  const int32_t lo[3] = {p.origin[0], p.origin[1], p.origin[2]}, hi[3] = {p.origin[0] + p.n[0], p.origin[1] + p.n[1], p.origin[2] + p.n[2]};
  int64_t n = 0;
  if (vdo_dense_extract(map, lo, hi, s_.minWeight, 0, nullptr, nullptr, nullptr, 0, &n) != VDO_OK) die("vdo_dense_extract");
  to.xyz.assign(3 * (size_t)n, 0.f); to.grad.assign(3 * (size_t)n, 0); to.weight.assign((size_t)n, 0);
  if (n == 0) return;
  if (vdo_dense_extract(map, lo, hi, s_.minWeight, n, to.xyz.data(), to.grad.data(), to.weight.data(), 0, &n) != VDO_OK) die("vdo_dense_extract");
}

template <class Stats, class Integrate>
void ObjectMapper::Flow(int f, const float Tcw[16], const std::vector<Motion>& motions, Stats stats, Integrate integrate) {
  double Tc[16];
  for (int i = 0; i < 16; ++i) Tc[i] = (double)Tcw[i];
  if (stats(stats_.data()) != VDO_OK) die("vdo_objects_stats");                                                   // 1
  for (size_t i = 0; i < live_.size();) {                                                                         // 2
    const int mod = live_[i].mod_label;
    if (std::any_of(motions.begin(), motions.end(), [mod](const Motion& m) { return m.mod_label == mod; })) { ++i; continue; }
    Live gone = std::move(live_[i]);
    live_.erase(live_.begin() + (long)i);
    if (gone.frames >= s_.minFrames) {
      Model m;
      m.mod_label = gone.mod_label; m.live = false; m.frames = gone.frames; m.trajectory = std::move(gone.traj);
      Extract(gone.slot.map, m.points);
      if (mesher_) ExtractMesh(gone.slot.map, m.mesh, m.tri);
      finished_.push_back(std::move(m));
    } else {
      ++dropped_;
    }
    if (vdo_dense_clear(gone.slot.map) != VDO_OK) die("vdo_dense_clear");
    pool_.push_back(gone.slot);
  }
  std::vector<int> seen_mod, seen_sem;
  for (const Motion& mo : motions) {                                                                              // 3
    if (std::find(seen_mod.begin(), seen_mod.end(), mo.mod_label) != seen_mod.end() || std::find(seen_sem.begin(), seen_sem.end(), mo.sem_label) != seen_sem.end()) continue;
    seen_mod.push_back(mo.mod_label); seen_sem.push_back(mo.sem_label);
    auto it = std::find_if(live_.begin(), live_.end(), [&](const Live& m) { return m.mod_label == mo.mod_label; });
    if (it != live_.end()) {
      mul44d(mo.H, it->Two.data(), it->Two.data());
      it->sem_label = mo.sem_label;
    } else if ((int)live_.size() < s_.maxObjects && Count(mo.sem_label) >= s_.minPixels) {
      Live m;
      m.mod_label = mo.mod_label; m.sem_label = mo.sem_label; m.frames = 0;
      const int64_t* row = stats_.data() + (size_t)mo.sem_label * 8;
      const double den = 1024.0 * (double)row[0], c[3] = {(double)row[5] / den, (double)row[6] / den, (double)row[7] / den};
      m.Two = Pose{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
      for (int a = 0; a < 3; ++a) {
        // Twc = [R^T | -R^T t]: row a of R^T is column a of R
        const double t = -((Tc[a] * Tc[3] + Tc[4 + a] * Tc[7]) + Tc[8 + a] * Tc[11]);
        m.Two[4 * a + 3] = ((Tc[a] * c[0] + Tc[4 + a] * c[1]) + Tc[8 + a] * c[2]) + t;
      }
      if (!pool_.empty()) { m.slot = pool_.back(); pool_.pop_back(); }
      else if (vdo_dense_create(ctx_, w_, h_px_, &s_.params, &m.slot.map) != VDO_OK) die("vdo_dense_create");
      live_.push_back(std::move(m));
    } else {
      ++skipped_;
    }
  }
  std::vector<vdo_dense*> maps; std::vector<int32_t> labels; std::vector<float> T; std::vector<Live*> batch;      // 4
  for (Live& m : live_) {
    if (Count(m.sem_label) < s_.minPixels) continue;
    double To[16];
    mul44d(Tc, m.Two.data(), To);
    maps.push_back(m.slot.map); labels.push_back(m.sem_label); batch.push_back(&m);
    for (int i = 0; i < 16; ++i) T.push_back((float)To[i]);
  }
  std::vector<int64_t> out(3 * std::max<size_t>(maps.size(), 1), 0);
  if (integrate((int)maps.size(), maps.data(), labels.data(), T.data(), out.data()) != VDO_OK) die("vdo_objects_integrate");
  for (Live* m : batch) ++m->frames;
  for (Live& m : live_) m.traj.push_back(std::make_pair(f, m.Two));
}

void ObjectMapper::FuseFrame(int f, const vdo_frame_images* frame, const float Tcw[16], const std::vector<Motion>& motions) {
  Flow(f, Tcw, motions, [&](int64_t* st) { return vdo_objects_stats_frame(stage_, frame, st); },
       [&](int n, vdo_dense* const* maps, const int32_t* labels, const float* T, int64_t* out) { return vdo_objects_integrate_frame(stage_, frame, n, maps, labels, T, out); });
}

void ObjectMapper::Fuse(int f, const cv::Mat& depth, const cv::Mat& mask, const float Tcw[16], const std::vector<Motion>& motions) {
  auto image = [&](const cv::Mat& m, int type) { return !m.empty() && m.rows == h_px_ && m.cols == w_ && m.depth() == type && m.channels() == 1 && m.step % 4 == 0; };
  if (!image(depth, cv::CV_32F)) throw std::runtime_error("VDO_SLAM::ObjectMapper: depth must be CV_32FC1 of the mapper's size");
  if (!image(mask, cv::CV_32S)) throw std::runtime_error("VDO_SLAM::ObjectMapper: mask must be CV_32SC1 of the mapper's size");
  const float* d = (const float*)depth.data; const int32_t* m = (const int32_t*)mask.data;
  const int64_t ds = (int64_t)(depth.step / 4), ms = (int64_t)(mask.step / 4);
  Flow(f, Tcw, motions, [&](int64_t* st) { return vdo_objects_stats(stage_, d, ds, m, ms, 0, st); },
       [&](int n, vdo_dense* const* maps, const int32_t* labels, const float* T, int64_t* out) { return vdo_objects_integrate(stage_, d, ds, m, ms, 0, n, maps, labels, T, out); });
}

bool ObjectMapper::Render(int mod_label, const float Tcw[16], cv::Mat& depth, cv::Mat& normals, int64_t counts[3]) {
  auto it = std::find_if(live_.begin(), live_.end(), [&](const Live& m) { return m.mod_label == mod_label; });
  if (it == live_.end()) return false;
  if (!it->slot.view) {
    DenseMapper::Settings vs;
    vs.params = s_.params; vs.minWeight = s_.minWeight;
    DenseMapper::ViewDefaults(vs);
    const std::string err = DenseMapper::CheckView(vs);
    if (!err.empty()) throw std::runtime_error("VDO_SLAM::ObjectMapper: " + err);
    const vdo_raycast_params rp{{s_.params.K[0], s_.params.K[1], s_.params.K[2], s_.params.K[3]}, vs.viewNear, vs.viewStep, vs.viewSteps, vs.viewMinWeight};
    if (vdo_raycast_create(it->slot.map, w_, h_px_, &rp, &it->slot.view) != VDO_OK) die("vdo_raycast_create");
  }
  double Tc[16], To[16];
  float T[16];
  for (int i = 0; i < 16; ++i) Tc[i] = (double)Tcw[i];
  mul44d(Tc, it->Two.data(), To);
  for (int i = 0; i < 16; ++i) T[i] = (float)To[i];
  grad_.resize((size_t)w_ * h_px_ * 3);
  depth.create(h_px_, w_, cv::CV_32FC1);
  normals.create(h_px_, w_, cv::CV_32FC3);
  int64_t out[3] = {0, 0, 0};
  if (vdo_raycast_render(it->slot.view, T, (float*)depth.data, grad_.data(), nullptr, 0, out) != VDO_OK) die("vdo_raycast_render");
  float* nrm = (float*)normals.data;
  for (size_t i = 0; i < (size_t)w_ * h_px_; ++i) {
    const double g[3] = {(double)grad_[3 * i], (double)grad_[3 * i + 1], (double)grad_[3 * i + 2]};
    const double len = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    for (int k = 0; k < 3; ++k) nrm[3 * i + k] = len > 0 ? (float)(g[k] / len) : 0.f;
  }
  if (counts) for (int k = 0; k < 3; ++k) counts[k] = out[k];
  return true;
}

std::vector<ObjectMapper::Model> ObjectMapper::Models() {
  std::vector<Model> all = finished_;
  for (Live& l : live_) {
    Model m;
    m.mod_label = l.mod_label; m.live = true; m.frames = l.frames; m.trajectory = l.traj;
    Extract(l.slot.map, m.points);
    if (mesher_) ExtractMesh(l.slot.map, m.mesh, m.tri);
    all.push_back(std::move(m));
  }
  return all;
}

bool ObjectMapper::SaveMeshes(const std::string& prefix) {
  if (!mesher_) return false;
  for (const Model& m : Models())
    if (!DenseMapper::WriteMeshPLY(prefix + "_" + std::to_string(m.mod_label) + "_mesh.ply", m.mesh, m.tri)) return false;
  return true;
}

bool ObjectMapper::SaveModels(const std::string& prefix) {
  const std::vector<Model> all = Models();
  bool ok = true;
  for (const Model& m : all) {
    FILE* f = std::fopen((prefix + "_" + std::to_string(m.mod_label) + ".ply").c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment object %d, object frame, TSDF zero crossings\nelement vertex %zu\n", m.mod_label, m.points.size());
    std::fprintf(f, "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty int weight\nend_header\n");
    for (size_t i = 0; i < m.points.size() && ok; ++i) {
      const double g[3] = {(double)m.points.grad[3 * i], (double)m.points.grad[3 * i + 1], (double)m.points.grad[3 * i + 2]};
      const double len = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
      char rec[28];                                                          // (x86-64 is little-endian: the records are written as they lie)
      float v[6] = {m.points.xyz[3 * i], m.points.xyz[3 * i + 1], m.points.xyz[3 * i + 2], 0.f, 0.f, 0.f};
      if (len > 0) for (int k = 0; k < 3; ++k) v[3 + k] = (float)(g[k] / len);
      std::memcpy(rec, v, 24); std::memcpy(rec + 24, &m.points.weight[i], 4);
      ok = std::fwrite(rec, 1, 28, f) == 28;
    }
    ok = std::fclose(f) == 0 && ok;
    if (!ok) return false;
  }
  FILE* f = std::fopen((prefix + "_poses.txt").c_str(), "w");
  if (!f) return false;
  for (const Model& m : all)
    for (const auto& row : m.trajectory) {
      std::fprintf(f, "%d %d", row.first, m.mod_label);
      for (int i = 0; i < 16; ++i) std::fprintf(f, " %.9f", row.second[i]);
      std::fprintf(f, "\n");
    }
  return std::fclose(f) == 0;
}

}  // namespace VDO_SLAM
