// DenseMapper - the dense map of the static scene: a TSDF voxel volume on the device (vdo_dense_* of libvdo_hip) that follows the camera, and the
// surface points of what has left it, on the host.  The reference keeps no dense map; the semantics of the volume are stated in
// include/vdo_slam_hip.h, the per-frame flow below is restated by vdo_slam_amd/dense.py (FollowingMap).
#pragma once
#include <string>
#include <vector>

#include "host_context.h"
#include "minicv.h"

namespace VDO_SLAM {

class DenseMapper {
 public:
  // The settings file's Dense.* keys (System.h): the volume and the fusion (params.origin is where the volume waits for the first frame), the camera
  // centre's target place in the volume as fractions of its size, the distance in voxels from that place at which the volume moves, and the smallest
  // weight of an extracted voxel
  struct Settings {
    vdo_dense_params params{}; double anchor[3] = {0.5, 0.5, 0.25}; int margin = 0; int minWeight = 2;
    // The view Render makes (settings keys Dense.View.*): the z-depth of a ray's first sample and between samples (metres), the samples per ray and the
    // smallest weight of a sampled voxel.  viewSteps == 0: not set yet - Render then takes ViewDefaults.
    float viewNear = 0.f, viewStep = 0.f; int viewSteps = 0, viewMinWeight = 0;
    // The alignment Align makes (settings keys Dense.Align.*): the Gauss-Newton rounds (0: System aligns no frame; Align itself then takes 10), the
    // gate on the distance between a point and its model point in metres (0: params.trunc), the sample stride, the smallest number of used samples
    // (0: a sixteenth of the sample grid, at least 6), and whether System fuses with the aligned pose.
    int alignIterations = 0; float alignMaxDist = 0.f; int alignSubsample = 1, alignMinPixels = 0; bool alignApply = false;
    // The photometric term beside it (settings keys Dense.Align.Photo*): the weight in metres per grey level (0: off - there is no default weight), the
    // gate on the grey residual in levels (255 turns it off) and the smallest number of used photometric samples (0: the aligner's).
    float alignPhoto = 0.f, alignPhotoMaxDiff = 255.f; int alignPhotoMinPixels = 0;
    // Settings key Dense.Mesh (0): a mesher is made, and before the volume moves the quads that will not be wholly inside what stays are kept (Mesh below)
    bool mesh = false;
    // Settings keys Dense.Colour (0), Dense.Colour.Band (params.trunc / 2), Dense.Colour.MaxWeight (params.max_weight), Dense.Colour.MinWeight (1): a
    // colourer is made beside the volume (vdo_colour_*), FuseColour fuses a frame's image, and every Points this class hands out carries rgba.
    // colourBand == 0 and colourMaxWeight == 0 stand for the defaults.
    bool colour = false; float colourBand = 0.f; int colourMaxWeight = 0, colourMinWeight = 1;
    // Settings keys Dense.Distance (0), Dense.Distance.Radius (2.0 metres), Dense.Distance.MinWeight (minWeight; 0 stands for it): a distance field
    // of the volume's size is made (vdo_distance_*) and Distance and Clearance serve it.  Nothing runs per frame.
    bool distance = false; float distanceRadius = 2.f; int distanceMinWeight = 0;
  };
  // The radius in voxels: ceil(distanceRadius / voxel) in double; 0 when that is not a number in 1..8191
  static int DistanceRadiusVoxels(const Settings& s);
  // The settings error of the distance fields ("" when in order): Radius not positive or not finite, or outside 1..8191 voxels; MinWeight outside
  // 1..255 (0 stands for minWeight)
  static std::string CheckDistance(const Settings& s);
  // The settings error of the colour fields ("" when in order): Band not positive, not finite or above params.trunc; MaxWeight, MinWeight outside 1..255
  static std::string CheckColour(const Settings& s);
  // The settings error of the alignment fields ("" when in order): Iterations outside 0..64, MaxDist negative or not finite (0 stands for the default; the settings reader itself refuses a zero key), Subsample
  // outside 1..8, MinPixels below 6 (0 stands for the default).
  static std::string CheckAlign(const Settings& s);
  // The smallest number of used samples Align asks for on width x height images
  static int AlignMinPixels(const Settings& s, int width, int height);
  // The settings error of the photometric fields ("" when in order): Photo negative or not finite, MaxDiff outside (0, 255], MinPixels below 6 (0
  // stands for the aligner's)
  static std::string CheckAlignPhoto(const Settings& s);
  // The smallest number of used photometric samples AlignPhoto asks for
  static int AlignPhotoMinPixels(const Settings& s, int width, int height);
  // The defaults of the view from the fields above: Near max(min_depth, voxel); Step trunc / 2 - half the thickness of the valid negative band behind a
  // surface, so that a pair of samples cannot step over that band from the fusing direction; MinWeight minWeight.
  static void ViewDefaults(Settings& s);
  // viewSteps = ceil((max_depth - Near) / Step) + 1 in double.  Returns the settings error ("" when in order): a non-finite value, Step <= 0, Near < 0,
  // Near >= max_depth, MinWeight outside 1..255, more than 65536 samples.
  static std::string CheckView(Settings& s);
  static Settings DefaultSettings(const float K[4], float voxel, float maxDepth) {
    Settings s;
    s.params = vdo_dense_params{{256, 128, 256}, voxel, {0, 0, 0}, {K[0], K[1], K[2], K[3]}, 4.f * voxel, 0.f, maxDepth, 64, 1 << 20};
    s.margin = 128 / 8;
    return s;
  }
  // The surface points kept on the host: xyz [n][3], the unnormalised integer gradient [n][3], the weight [n] and, with settings().colour, the colour
  // [n][4] (red, green, blue, alpha; alpha 0: no colour was fused there) - `coloured` says whether the points carry colours at all (also when there
  // are none); rgba stays empty and coloured false when colour is off
  struct Points { std::vector<float> xyz; std::vector<int32_t> grad, weight; std::vector<uint8_t> rgba; bool coloured = false; size_t size() const { return weight.size(); } };
  // An image FuseColour reads: uint8, 1 (grey), 3 or 4 channels per pixel, rows `step` bytes apart, R first unless bgr; a host or a device pointer
  struct Image { const uint8_t* data; int64_t step; int channels; bool bgr; bool device; };

  // A mapper for width x height depth and mask images on `ctx` (HostContext() when null).  Throws std::runtime_error when the library refuses.
  DenseMapper(vdo_ctx* ctx, int width, int height, const Settings& settings);
  ~DenseMapper();
  DenseMapper(const DenseMapper&) = delete;
  DenseMapper& operator=(const DenseMapper&) = delete;
  // One frame.  Before it is fused the camera centre's voxel c = floor(-R^T t / voxel) is computed in double; if the volume has not started, or c is
  // further than `margin` voxels from origin + floor(anchor * n) on any axis, what leaves the volume is extracted (the x slab, then the y slab of what
  // stays on x, then the z slab of what stays on x and y; the whole volume for a move of n or more) and appended to kept(), and the volume moves so
  // that c sits at its target place.  Then the frame's resident depth and mask (or the cv::Mats: CV_32FC1 metres, CV_32SC1 or empty) are fused with
  // Tcw (16 floats, world -> camera).  counts (optional): updated, masked and occluded voxels.
  void FuseFrame(const vdo_frame_images* frame, const float Tcw[16], int64_t counts[3] = nullptr);
  void Fuse(const cv::Mat& depth, const cv::Mat& mask, const float Tcw[16], int64_t counts[3] = nullptr);
  // The colour of the frame the last FuseFrame fused, with the same pose (vdo_colour_integrate_frame, label 0: the pixels the geometry left out are
  // left out here).  The image has the mapper's size.  counts (optional): voxels updated, skipped by the mask, skipped as outside the band.  Throws
  // std::runtime_error unless settings().colour and the last frame came through FuseFrame (Fuse keeps nothing of its cv::Mats).
  void FuseColour(const Image& image, const float Tcw[16], int64_t counts[3] = nullptr);
  // What the map predicts a camera at Tcw would see, in colour: Render's depth image, then the colour of its points (vdo_colour_render) as CV_8UC4
  // (red, green, blue, alpha; 0 without a surface or a colour).  Throws std::runtime_error unless settings().colour.
  void RenderColour(const float Tcw[16], cv::Mat& rgba);
  // kept() followed by what is in the volume now (neither is changed)
  Points AllPoints();
  // AllPoints() as a binary little-endian PLY: x, y, z, nx, ny, nz (float; the gradient normalised in double and narrowed, or 0) and weight (int);
  // with settings().colour also red, green, blue, alpha (uchar).  False when the file cannot be written.
  bool SavePLY(const std::string& path);
  // The surface as connected triangles (vdo_mesh_extract, surface nets): the pieces kept before the moves, then the whole current volume; tri holds
  // 3 indices per triangle into v, every piece rebased by the number of vertices before it.  Pieces share no vertices; no quad is lost or doubled
  // at a seam, whatever the direction of a move.  Throws std::runtime_error unless settings().mesh.
  void Mesh(Points& v, std::vector<int32_t>& tri);
  // Mesh() as a binary little-endian PLY: the vertices as SavePLY writes its points, then `face` as uchar int lists of 3.  False when the file
  // cannot be written.
  bool SaveMeshPLY(const std::string& path);
  // The file SaveMeshPLY writes, for any mesh (ObjectMapper::SaveMeshes writes its models with it); the four uchar colour properties iff v.coloured -
  // decided once for the header and every record; false, nothing written, if v.rgba does not then hold four bytes per vertex
  static bool WriteMeshPLY(const std::string& path, const Points& v, const std::vector<int32_t>& tri);
  // The mesh of `map` for the box and mode (vdo_mesh_extract) appended to v and tri, the new indices rebased by the vertices already in v.  ONE
  // extraction when the outputs fit `guess` (vertices, triangles: what the last call of this caller needed, kept up to date here), else a second
  // one at the counts the first reported.
  static void AppendMeshOf(vdo_mesh* mesher, vdo_dense* map, const int32_t lo[3], const int32_t hi[3], int outside, int min_weight, int64_t guess[2], Points& v,
                           std::vector<int32_t>& tri);
  // What the map predicts a camera at Tcw (16 floats, world -> camera) would see (vdo_raycast_render): depth CV_32FC1 (metres, 0 without a surface),
  // normals CV_32FC3 (world frame, towards free space: the gradient normalised in double and narrowed, or 0, as SavePLY writes them) and, optionally,
  // weight CV_32SC1.  The view is made on first use at the mapper's image size and K with the settings' view fields; nothing of the map changes.
  // counts (optional): rays that hit, rays that missed, rays with no valid sample.
  void Render(const float Tcw[16], cv::Mat& depth, cv::Mat& normals, cv::Mat* weight = nullptr, int64_t counts[3] = nullptr);
  // How far a pose is from the geometry in the map: the view is rendered at Tcw_init straight into the aligner's model (vdo_align_set_model_from_view)
  // and the frame - the cv::Mats as Fuse takes them, or a frame's resident depth and mask - is aligned against it (vdo_align_solve: point-to-plane
  // ICP, the model fixed, eps 1e-5).  Tcw_out: the refined pose, Tcw_init bit for bit unless report->status is 0 (1: too few samples met the map -
  // an empty map, for instance; 2: the geometry does not constrain all six motions).  The view and the aligner are made on first use; nothing of
  // the map changes.
  void Align(const cv::Mat& depth, const cv::Mat& mask, const float Tcw_init[16], float Tcw_out[16], vdo_align_report* report = nullptr);
  void AlignFrame(const vdo_frame_images* frame, const float Tcw_init[16], float Tcw_out[16], vdo_align_report* report = nullptr);
  // Align with the photometric term (vdo_photo_solve: include/vdo_slam_hip.h, "Photometric aligner"; settings().alignPhoto > 0, else it throws): the
  // frame's image becomes the photometric handle's grey image, and the frame is aligned jointly - the aligner against the map's view rendered at
  // Tcw_init, the intensity term against the MODEL FRAME KeepPhotoModel last kept - with the weight settings().alignPhoto.  Without a model frame
  // (the first frame), and whenever the joint solve ends with status 1, the frame is aligned by the geometry alone, exactly as Align does it, and
  // the report says so: used_photo and both rms_photo are 0.  The handle is made on first use.
  void AlignPhoto(const cv::Mat& depth, const cv::Mat& mask, const Image& image, const float Tcw_init[16], float Tcw_out[16], vdo_photo_report* report = nullptr);
  void AlignPhotoFrame(const vdo_frame_images* frame, const Image& image, const float Tcw_init[16], float Tcw_out[16], vdo_photo_report* report = nullptr);
  // The frame whose image the last AlignPhoto* set becomes the model frame with the pose it was fused with (vdo_photo_keep_as_model_frame: masked
  // pixels - moving objects - carry no depth and are left out).
  void KeepPhotoModel(const vdo_frame_images* frame, const float Tcw[16]);
  // The distance field of the box [lo, hi) (global voxels, clipped to the volume; both null: the whole current volume) with the settings' radius and
  // weight (vdo_distance_compute); it becomes the snapshot Clearance samples until the map changes.  counts (optional): sites, voxels within the
  // radius, voxels of the clipped box.  Throws std::runtime_error unless settings().distance.
  void Distance(const int32_t lo[3], const int32_t hi[3], int64_t counts[3] = nullptr);
  // The field words (include/vdo_slam_hip.h, "Distance field") of n world points xyz [n][3].  The whole current volume's field is computed first if
  // the map was fused or moved since the last whole-volume field (a generation counter that Fuse, FuseFrame and a move bump), or if the snapshot is
  // a box of Distance's; two calls with nothing in between compute once.  Throws std::runtime_error unless settings().distance.
  void Clearance(const float* xyz, int64_t n, uint32_t* words);
  int distanceComputes() const { return distComputes_; } // the fields computed so far
  const Points& kept() const { return kept_; }
  int recenters() const { return recenters_; }
  void origin(int32_t out[3]) const;
  vdo_dense* handle() { return h_; }
  int width() const { return w_; }
  int height() const { return h_px_; }
  const Settings& settings() const { return s_; }

 private:
  void Follow(const float Tcw[16]);
  void Append(const int32_t lo[3], const int32_t hi[3], Points& to);
  void AppendMesh(const int32_t lo[3], const int32_t hi[3], int outside, Points& v, std::vector<int32_t>& tri);
  void Colour(Points& p, size_t from);                   // with a colourer: p.rgba of the points from `from` on, sampled from the volume as it is now
  void EnsureView();
  void EnsureAligner(const float Tcw_init[16]);          // and renders the view at Tcw_init into its model
  void EnsurePhoto(const Image& image);                  // and packs the image into its grey image
  // the joint solve (frame, or depth and mask when frame is null), or the aligner's alone: see AlignPhoto
  void SolvePhoto(const vdo_frame_images* frame, const cv::Mat* depth, const cv::Mat* mask, const float Tcw_init[16], float Tcw_out[16], vdo_photo_report* report);
  vdo_ctx* ctx_ = nullptr;
  vdo_dense* h_ = nullptr;
  vdo_raycast* view_ = nullptr;                          // made by the first Render or Align; destroyed before the map
  vdo_align* align_ = nullptr;                           // made by the first Align; destroyed before the view
  vdo_photo* photo_ = nullptr;                           // made by the first AlignPhoto; destroyed before the view
  bool photoModel_ = false;                              // KeepPhotoModel has kept a frame
  vdo_mesh* mesher_ = nullptr;                           // only with settings().mesh
  vdo_colour* colour_ = nullptr;                         // only with settings().colour; borrows the map: destroyed before it
  vdo_distance* dist_ = nullptr;                         // only with settings().distance; destroyed before the map
  uint64_t generation_ = 1, distGeneration_ = 0;         // bumped by every fusion and move; the generation the whole-volume field was computed at (0: none)
  int distComputes_ = 0;
  const vdo_frame_images* lastFrame_ = nullptr;          // what the last FuseFrame fused; null after Fuse
  std::vector<float> grad_;                              // [h][w][3]: the gradient image of the last Render
  Settings s_;
  int w_, h_px_;
  bool started_ = false;
  int recenters_ = 0;
  Points kept_;
  Points keptMeshV_;                                     // the mesh pieces kept before the moves
  std::vector<int32_t> keptMeshT_;
  int64_t meshGuess_[2] = {1 << 16, 1 << 17};            // the capacities the next mesh extraction tries first
};

}  // namespace VDO_SLAM
