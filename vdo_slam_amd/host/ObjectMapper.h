// ObjectMapper - a dense model per tracked object: a TSDF volume (a plain vdo_dense of libvdo_hip) in a frame of the object's own, whose pose Two is
// chained from the tracker's world-frame motions, fused from the pixels that carry the object's mask label (vdo_objects_* of libvdo_hip) and kept as
// points when the object is gone.  The reference keeps no dense map; the device semantics are stated in include/vdo_slam_hip.h, the per-frame flow
// below is restated by vdo_slam_amd/objects.py (ObjectMaps) and in NumPy by tests/objects_ref.py (RefMaps).
#pragma once
#include <array>
#include <string>
#include <utility>
#include <vector>

#include "DenseMapper.h"
#include "host_context.h"
#include "minicv.h"

namespace VDO_SLAM {

class ObjectMapper {
 public:
  // The settings file's Dense.Objects.* keys (System.h).  params: every object's volume (n, voxel, K, trunc, depth range, weight cap, stage_points;
  // the origin is set to -floor(n / 2) per axis here, so that a model's first centroid sits in the middle).
  struct Settings { vdo_dense_params params{}; int maxObjects = 16, minPixels = 200, minFrames = 3, minWeight = 2, maxLabels = 1023; bool mesh = false; };
  // (mesh: settings key Dense.Mesh - a mesher of the object volumes' size is made, and every model also carries its surface as triangles)
  // The settings error of the fields above ("" when in order): MaxObjects outside 1..64, MinPixels or MinFrames below 1, MinWeight outside 1..255
  static std::string Check(const Settings& s);
  // One tracked object of a frame: the unique tracking id, the label its pixels carry in the frame's mask, the world-frame motion from the last frame
  // to this one (a float entry converts exactly)
  struct Motion { int mod_label = 0, sem_label = 0; double H[16] = {0}; };
  typedef std::array<double, 16> Pose;
  // A model as Models() reports it: points in the object frame (of a live model: what is in its volume now), the (frame, Two) rows
  struct Model { int mod_label = 0; bool live = false; int frames = 0; DenseMapper::Points points; std::vector<std::pair<int, Pose> > trajectory;
                 DenseMapper::Points mesh; std::vector<int32_t> tri; };      // with settings().mesh: the whole volume's mesh (vdo_mesh_extract), object frame

  // For width x height depth and mask images on `ctx` (HostContext() when null).  Throws std::runtime_error when the library refuses.
  ObjectMapper(vdo_ctx* ctx, int width, int height, const Settings& settings);
  ~ObjectMapper();
  ObjectMapper(const ObjectMapper&) = delete;
  ObjectMapper& operator=(const ObjectMapper&) = delete;
  // One frame f with Tcw (16 floats, world -> camera: the pose the static map was fused with) and the frame's motions in the tracker's order; all
  // pose algebra in double, every 4 x 4 product entry ((a0*b0 + a1*b1) + a2*b2) + a3*b3.
  //   1. the label statistics of the frame (vdo_objects_stats);
  //   2. every live model whose mod_label is not in the list is retired: its whole box is extracted (minWeight) and kept as a finished model if it
  //      was fused in at least minFrames frames, else dropped (counted); its handle is cleared and goes back to a pool;
  //   3. the list in order, a mod_label or sem_label seen earlier in it ignored: a live model's Two <- H * Two (and its label is this frame's);
  //      otherwise, with fewer than maxObjects live models and at least minPixels counting pixels, a model starts - world axes, the origin at
  //      Twc * (sx, sy, sz) / (1024 * count); otherwise the object is skipped (counted);
  //   4. ONE vdo_objects_integrate call over the live models whose label counts at least minPixels pixels, T_i = Tcw * Two rounded to float once per
  //      entry; a live model below minPixels keeps its chained pose and is not fused; (f, Two) is appended to every live model's trajectory.
  void FuseFrame(int f, const vdo_frame_images* frame, const float Tcw[16], const std::vector<Motion>& motions);
  void Fuse(int f, const cv::Mat& depth, const cv::Mat& mask, const float Tcw[16], const std::vector<Motion>& motions);     // CV_32FC1 metres, CV_32SC1
  // What the model of a LIVE object predicts a camera at Tcw would see: a vdo_raycast view on the object's map, made on first use with
  // DenseMapper::ViewDefaults of the object volumes, rendered at Tcw * Two.  Outputs as DenseMapper::Render (normals in the OBJECT frame).  False
  // when no live model carries mod_label.
  bool Render(int mod_label, const float Tcw[16], cv::Mat& depth, cv::Mat& normals, int64_t counts[3] = nullptr);
  // The finished models, then the live ones as they stand; nothing changes.
  std::vector<Model> Models();
  // <prefix>_<mod_label>.ply per model in the object frame (the binary layout of DenseMapper::SavePLY) and <prefix>_poses.txt: frame, mod_label and
  // the 16 entries of Two per row, fixed with 9 digits (the row style of System::SaveResults).  False when a file cannot be written.
  bool SaveModels(const std::string& prefix);
  // With settings().mesh: <prefix>_<mod_label>_mesh.ply per model in the object frame (the layout of DenseMapper::SaveMeshPLY) - a finished model as
  // it was meshed when it was retired, a live one as its volume stands.  False without settings().mesh or when a file cannot be written.
  bool SaveMeshes(const std::string& prefix);
  int dropped() const { return dropped_; }
  int skipped() const { return skipped_; }
  int live() const { return (int)live_.size(); }
  // (mod_label, Two) of every live model, in their order; nothing is extracted
  std::vector<std::pair<int, Pose> > LivePoses() const {
    std::vector<std::pair<int, Pose> > out;
    for (const Live& l : live_) out.emplace_back(l.mod_label, l.Two);
    return out;
  }
  const int64_t* last_stats() const { return stats_.data(); }     // [(maxLabels + 1)][8] of the last frame
  vdo_objects* handle() { return stage_; }
  const Settings& settings() const { return s_; }

 private:
  struct Slot { vdo_dense* map = nullptr; vdo_raycast* view = nullptr; };      // a volume and the view made on it (the view borrows the map)
  struct Live { int mod_label, sem_label, frames; Pose Two; std::vector<std::pair<int, Pose> > traj; Slot slot; };
  template <class Stats, class Integrate> void Flow(int f, const float Tcw[16], const std::vector<Motion>& motions, Stats stats, Integrate integrate);
  void Extract(vdo_dense* map, DenseMapper::Points& to);
  void ExtractMesh(vdo_dense* map, DenseMapper::Points& v, std::vector<int32_t>& tri);
  int64_t Count(int sem) const { return sem >= 1 && sem <= s_.maxLabels ? stats_[(size_t)sem * 8] : 0; }
  vdo_ctx* ctx_ = nullptr;
  vdo_objects* stage_ = nullptr;
  vdo_mesh* mesher_ = nullptr;                           // only with settings().mesh
  int64_t meshGuess_[2] = {1 << 14, 1 << 15};
  Settings s_;
  int w_, h_px_;
  std::vector<int64_t> stats_;
  std::vector<Live> live_;
  std::vector<Model> finished_;
  std::vector<Slot> pool_;
  std::vector<float> grad_;
  int dropped_ = 0, skipped_ = 0;
};

}  // namespace VDO_SLAM
