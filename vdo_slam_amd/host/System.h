// System / Tracking — the reference's entry API (include/System.h:42-53, include/Tracking.h) as thin shells around
// FramePipeline: settings file, colour conversion, the in-place depth conversion the caller sees, ground-truth rows as the
// gate of the object tracker, Map bookkeeping, the batch optimisations and SaveResults' five text files (src/System.cc:75-100).  Visualisation (imTraj)
// and metric printing are out of scope; the hot path is entirely behind FramePipeline.
#pragma once
#include <array>
#include <chrono>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "FlowMatcher.h"
#include "Frame.h"
#include "FramePipeline.h"
#include "DenseMapper.h"
#include "ObjectMapper.h"
#include "InstanceLabeler.h"
#include "StereoRectifier.h"
#include "Map.h"
#include "MotionSegmenter.h"
#include "StereoMatcher.h"
#include "minicv.h"

namespace VDO_SLAM {

class System;

class Tracking {
 public:
  Tracking(System* pSys, Map* pMap, const std::string& strSettingPath, const int sensor);
  ~Tracking();
  // Tracking::GrabImageRGBD (src/Tracking.cc:164-314): imD is converted in place (raw disparity*factor -> metres), maskSEM
  // receives the labels UpdateMask recovered; returns mTcw.clone() (4x4 CV_32F)
  cv::Mat GrabImageRGBD(const cv::Mat& imRGB, cv::Mat& imD, const cv::Mat& imFlow, const cv::Mat& maskSEM, const cv::Mat& mTcw_gt,
                        const std::vector<std::vector<float> >& vObjPose_gt, const double& timestamp, cv::Mat& imTraj, const int& nImage);
  // The driver's frame step from files (example/vdo_slam.cc:104-131: imread -> convertTo(CV_32F) -> readOpticalFlow -> LoadMask) + the
  // call above: the host reads the four files and inflates the two PNGs (DatasetIO's InflatePNG); the mask parse, the PNG un-filter +
  // colour conversion and the .flo copy run on the device (vdo_ingest_frame) into the images Step takes.  The converted depth map and
  // the repaired mask stay on the device: SyncFrameState() brings them back (mDepthMap, mSegMap).  Empty Mat + stderr on a file that
  // cannot be read or decoded.
  cv::Mat GrabFilesRGBD(const std::string& rgbPath, const std::string& depthPath, const std::string& flowPath, const std::string& maskPath, const cv::Mat& mTcw_gt,
                        const std::vector<std::vector<float> >& vObjPose_gt, const double& timestamp, const int& nImage);
  // A rectified pair instead of a depth map (System::STEREO): both images to grey, the disparity x 256 x DepthMapFactor / 256 computed on the
  // device (StereoMatcher, settings keys Stereo.*) into a device depth_raw image, the flow and the mask brought up beside it, then the same
  // device-input Step as GrabFilesRGBD - the disparity never passes through the host.  K1 always converts it (whatever ChooseData says: a
  // disparity is not metric); only a power-of-two DepthMapFactor keeps that composition exact.  Inputs as GrabImageRGBD's.
  cv::Mat GrabImageStereo(const cv::Mat& imLeft, const cv::Mat& imRight, const cv::Mat& imFlow, const cv::Mat& maskSEM, const cv::Mat& mTcw_gt,
                          const std::vector<std::vector<float> >& vObjPose_gt, const double& timestamp, cv::Mat& imTraj, const int& nImage);
  // As GrabImageStereo, but the flow image is made here as well: the dense flow from the grey left image to the grey NEXT left image (the flow
  // image of frame t is the flow from t to t + 1), computed on the device (FlowMatcher, settings keys Flow.*) into the device flow image the step
  // takes - no host round trip.  The caller is one frame ahead of the tracker: it needs image t + 1 to track frame t.
  cv::Mat GrabImageStereoPair(const cv::Mat& imLeft, const cv::Mat& imRight, const cv::Mat& imLeftNext, const cv::Mat& maskSEM, const cv::Mat& mTcw_gt,
                              const std::vector<std::vector<float> >& vObjPose_gt, const double& timestamp, cv::Mat& imTraj, const int& nImage);
  // As GrabImageStereoPair, but the instance mask is made here as well, from a class image (CV_8UC1, 0 = background; a semantic map without
  // instances): on the device, the disparity, then the speckle filter if Stereo.SpeckleSize > 0, then the connected components of the class image
  // cut at disparity jumps (InstanceLabeler, settings keys Labels.*) written into the device mask image the step takes, then the flow.  The mask
  // never exists on the host; its labels carry no identity from frame to frame (the tracker associates objects through the flow).
  cv::Mat GrabImageStereoPairSemantic(const cv::Mat& imLeft, const cv::Mat& imRight, const cv::Mat& imLeftNext, const cv::Mat& classes, const cv::Mat& mTcw_gt,
                                      const std::vector<std::vector<float> >& vObjPose_gt, const double& timestamp, cv::Mat& imTraj, const int& nImage);
  // As GrabImageStereoPairSemantic, but the class image is made here as well: "which pixels move against the scene", from the next stereo pair.  On
  // the device, in this order: the disparity of the next pair (into the segmenter's own image), the disparity of the current pair (gate and
  // speckle filter as above; the matcher's staging image then holds the current left image for the step), the flow with its validity image, the
  // camera motion from grid samples (vdo_motionseg_egomotion, settings keys Motion.Ego*), the class image (MotionSegmenter, settings keys Motion.*)
  // straight into the labeller's device class image, the instance mask, the step.  With too few ego-motion inliers the class image is all zero
  // for that frame - it is tracked as static-only - and a line goes to stderr.  With Rectify.* keys the four pictures are the four jobs of one
  // vdo_rectify_compute.  The segmenter is made on the first call.
  cv::Mat GrabImageStereoVideo(const cv::Mat& imLeft, const cv::Mat& imRight, const cv::Mat& imLeftNext, const cv::Mat& imRightNext, const cv::Mat& mTcw_gt,
                               const std::vector<std::vector<float> >& vObjPose_gt, const double& timestamp, cv::Mat& imTraj, const int& nImage);
  // The dense map (settings keys Dense.*, System::SaveDenseMap below): null without Dense.VoxelSize.  Every Grab* entry fuses its frame in FinishFrame,
  // after the pose is known: the frame's resident depth and mask with that pose, on a context of its own.
  DenseMapper* dense() { return dense_.get(); }
  const int64_t* dense_counts() const { return dense_counts_; }      // updated, masked and occluded voxels of the last frame
  const int64_t* dense_colour_counts() const { return colour_counts_; }      // Dense.Colour: voxels coloured, skipped by the mask, outside the band in the last frame
  // With Dense.Align.Iterations > 0: the alignment of the last frame against the map, made at the tracker's pose before the frame was fused
  // (null otherwise, and before the first frame), and the pose the frame was fused with
  const vdo_align_report* dense_alignment() const { return dense_align_valid_ ? &dense_align_ : nullptr; }
  long long dense_alignments() const { return dense_align_count_; }      // frames aligned so far
  // With Dense.Align.Photo as well: the joint report of the same alignment (null otherwise).  dense_alignment() then carries its geometric half.
  const vdo_photo_report* dense_photo_alignment() const { return dense_photo_valid_ ? &dense_photo_ : nullptr; }
  bool rgb_order() const { return mbRGB; }               // Camera.RGB: the order of a colour image handed in
  const float* dense_fused_pose() const { return dense_fused_; }
  // The object mapper (settings keys Dense.Objects.*, System::SaveObjectMaps below): null without Dense.VoxelSize and Dense.Objects.VoxelSize.
  // FinishFrame runs its frame right after the static map's, on the same context, with the pose that map was fused with and the step's motions.
  ObjectMapper* objects() { return objects_.get(); }
  MotionSegmenter* motion() { return motion_.get(); }    // null before the first GrabImageStereoVideo
  // What the last GrabImageStereoVideo found: ego-motion inliers, moving pixels after the vote (0 when the ego-motion failed), labels
  const int* video_counts() const { return video_counts_; }
  // Raw images (settings keys Rectify.*, STEREO only; System::TrackStereo below): with the keys present, imLeft / imRight / imLeftNext of the three
  // entries above are the RAW images of Rectify.Width x Rectify.Height; one vdo_rectify_compute undistorts, rectifies and makes them grey straight
  // into the matchers' device images, and the disparity is cleared wherever the left map is invalid.  rectifier() is null without the keys.
  StereoRectifier* rectifier() { return rectifier_.get(); }
  // The rectified grey left image of the last Grab*Stereo* call (CV_8UC1 of Camera.width x Camera.height), e.g. to run a segmentation on it; empty
  // without a rectifier (the caller's own image is the rectified one then).
  cv::Mat DownloadRectifiedLeft();
  FramePipeline* pipeline() { return pipe_.get(); }
  InstanceLabeler* labeler() { return labels_.get(); }   // null unless the sensor is System::STEREO
  FlowMatcher* flow() { return flow_.get(); }            // null unless the sensor is System::STEREO
  StereoMatcher* stereo() { return stereo_.get(); }      // null unless the sensor is System::STEREO

  // ---- public state of the reference class (include/Tracking.h:116-198).  Scalar configuration / progress members are kept up to date by
  // every call.  The per-frame containers live in HBM / in FramePipeline's flat arrays; SyncFrameState() materialises them in the reference's
  // form on request (as System::map() does for the Map): mCurrentFrame - mTcw, the renewed static set (mvStatKeysTmp, mvStatDepthTmp,
  // mvStat3DPointTmp, mvCorres, mvFlowNext, N_s_tmp), the renewed object set (mvObjKeys, mvObjDepth, mvObj3DPoint, mvObjCorres, mvObjFlowNext,
  // vSemObjLabel, vObjLabel) and the per-object vectors (nSemPosition, nModLabel, bObjStat, vObjMod) as Track() leaves them
  // (src/Tracking.cc:2780-2812, 2984-2991, 836-933) -, the semi-dense samples mvTmpObj*, max_id, and the converted depth map / repaired mask
  // (mDepthMap, mSegMap).  mImGray / mFlowMap are the caller's own buffers; TemperalMatch* and repro_e are locals of Track() here.
  void SyncFrameState();
  Frame mCurrentFrame;
  cv::Mat mDepthMap, mSegMap;
  std::vector<cv::KeyPoint> mvTmpObjKeys, mvTmpObjCorres;
  std::vector<float> mvTmpObjDepth;
  std::vector<int> mvTmpSemObjLabel;
  std::vector<cv::Point2f> mvTmpObjFlowNext;
  int max_id = 1;
  enum eTrackingState { NO_IMAGES_YET = 0, NOT_INITIALIZED = 1, OK = 2 };
  eTrackingState mState = NO_IMAGES_YET, mLastProcessedState = NO_IMAGES_YET;
  enum eDataState { OMD = 1, KITTI = 2, VirtualKITTI = 3 };
  eDataState mTestData = KITTI;        // ChooseData
  int mSensor = 2;                     // System::RGBD
  int f_id = 0, StopFrame = 0;
  bool bLocalBatch = true, bGlobalBatch = true, bJoint = true, bFrame2Frame = false, bFirstFrame = true;
  int nWINDOW_SIZE = 0, nOVERLAP_SIZE = 0, nMaxTrackPointBG = 0, nMaxTrackPointOBJ = 0, nUseSampleFea = 0;
  float fSFMgThres = 0, fSFDsThres = 0;
  std::vector<float> all_timing;       // per frame: ms of this TrackRGBD call (the reference keeps five clock() buckets per frame)
  cv::Mat mK, mDistCoef;
  float mbf = 0, mThDepth = 0, mThDepthObj = 0, mDepthMapFactor = 1;

 private:
  Map* mpMap;
  std::map<std::string, double> cfg_;
  bool mbRGB = true;
  vdo_ctx* ctx_[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};     // front-end / camera LM / object LMs / helper thread / ORB thread
  std::unique_ptr<FramePipeline> pipe_;
  std::vector<uint8_t> gray_, gray_right_, gray_next_;
  std::unique_ptr<StereoMatcher> stereo_;
  std::unique_ptr<FlowMatcher> flow_;
  std::unique_ptr<InstanceLabeler> labels_;
  std::unique_ptr<StereoRectifier> rectifier_;           // Rectify.* keys present: the stereo entries take raw images
  int rect_border_ = 0, rect_classes_ = 0;               // Rectify.Border, Rectify.Classes
  std::unique_ptr<DenseMapper> dense_;                   // Dense.VoxelSize present: the dense map of the static scene
  vdo_ctx* ctx_dense_ = nullptr;                         // its context (made only with the mapper)
  std::unique_ptr<ObjectMapper> objects_;                // Dense.Objects.VoxelSize present as well: a volume per tracked object, on ctx_dense_
  int64_t dense_counts_[3] = {0, 0, 0};
  DenseMapper::Image colour_src_{};                      // Dense.Colour: the image of the frame in hand, set by every Grab* entry before FinishFrame
  int64_t colour_counts_[3] = {0, 0, 0};                 // voxels coloured, skipped by the mask, skipped as outside the band in the last frame
  vdo_align_report dense_align_{};                       // Dense.Align.Iterations > 0: the last frame against the map
  bool dense_align_valid_ = false;
  vdo_photo_report dense_photo_{};                       // Dense.Align.Photo > 0: the joint report of the last frame
  bool dense_photo_valid_ = false;
  long long dense_align_count_ = 0;
  float dense_fused_[16] = {0};                          // the pose the last frame was fused with
  std::unique_ptr<MotionSegmenter> motion_;              // made by the first GrabImageStereoVideo from motion_p_
  vdo_motionseg_params motion_p_{};                      // Motion.* keys (read and checked with the STEREO sensor only)
  MotionSegmenter::EgoParams ego_;                       // Motion.Ego* keys
  std::vector<uint8_t> gray_next_right_, zero_classes_;
  int video_counts_[3] = {0, 0, 0};
  int speckle_size_ = 0, speckle_range_ = 256;           // Stereo.SpeckleSize (0: no filter), Stereo.SpeckleRange, the latter in the depth image's units
  cv::Mat GrabStereoFrame(const char* who, const cv::Mat& imLeft, const cv::Mat& imRight, const cv::Mat* imFlow, const cv::Mat* imLeftNext, const cv::Mat* maskSEM,
                          const cv::Mat* classes, const cv::Mat& mTcw_gt, const std::vector<std::vector<float> >& vObjPose_gt, const int& nImage);
  cv::Mat GrabRawStereoFrame(const char* who, const cv::Mat& imLeft, const cv::Mat& imRight, const cv::Mat* imFlow, const cv::Mat* imLeftNext, const cv::Mat* maskSEM,
                             const cv::Mat* classes, const cv::Mat& mTcw_gt, const std::vector<std::vector<float> >& vObjPose_gt, std::chrono::steady_clock::time_point t_call);
  bool have_frame_ = false;
  vdo_ingest* ingest_ = nullptr;       // GrabFilesRGBD: device decode of the frame's files, made on first use
  cv::Mat FinishFrame(const cv::Mat& mTcw_gt, std::chrono::steady_clock::time_point t_call);
  cv::Mat mOriginInv;                  // ground-truth pose of the first frame (src/Tracking.cc:319-323)
};

class System {
 public:
  enum eSensor { MONOCULAR = 0, STEREO = 1, RGBD = 2 };
  System(const std::string& strSettingsFile, const eSensor sensor);
  ~System();
  cv::Mat TrackRGBD(const cv::Mat& im, cv::Mat& depthmap, const cv::Mat& flowmap, const cv::Mat& masksem, const cv::Mat& mTcw_gt,
                    const std::vector<std::vector<float> >& vObjPose_gt, const double& timestamp, cv::Mat& imTraj, const int& nImage);
  // TrackRGBD on the frame's files (Tracking::GrabFilesRGBD): rgbPath an 8-bit grey / RGB / RGBA PNG, depthPath an 8/16-bit grey disparity
  // PNG, flowPath a .flo file, maskPath the instance-mask text - what the reference's driver reads for one frame.
  cv::Mat TrackRGBDFromFiles(const std::string& rgbPath, const std::string& depthPath, const std::string& flowPath, const std::string& maskPath, const cv::Mat& mTcw_gt,
                             const std::vector<std::vector<float> >& vObjPose_gt, const double& timestamp, const int& nImage);
  // The reference's result files (src/System.cc:66-198), `filename` being the path PREFIX as there: initial_stereo_new.txt,
  // refined_stereo_new.txt, cam_pose_gt_stereo.txt (frame id + the 16 entries of T_wc, fixed, 9 digits) and the object motions per
  // transition in the same row format.  The reference writes the object motions in the BODY frame of the ground-truth object pose
  // (obj_mot_stereo_new.txt / _rf_new.txt / obj_mot_gt.txt / obj_centre.txt: ground-truth object-pose parsing, out of scope);
  // here they are written in the WORLD frame under names of their own: obj_mot_world_new.txt / obj_mot_world_rf_new.txt.
  // A STEREO system (settings keys Stereo.MaxDisparity 128, Stereo.P1 10, Stereo.P2 120, Stereo.Paths 8, Stereo.Uniqueness 5, Stereo.LRMaxDiff 1,
  // Stereo.SubPixel 1, all optional): Tracking::GrabImageStereo.  Exits like TrackRGBD when the sensor is not STEREO.
  cv::Mat TrackStereo(const cv::Mat& imLeft, const cv::Mat& imRight, const cv::Mat& flowmap, const cv::Mat& masksem, const cv::Mat& mTcw_gt,
                      const std::vector<std::vector<float> >& vObjPose_gt, const double& timestamp, cv::Mat& imTraj, const int& nImage);
  // Raw, unrectified images (all three stereo entries): the settings keys Rectify.Left.K: [fx, fy, cx, cy], Rectify.Left.D: [k1, k2, p1, p2, k3] (4 values:
  // k3 = 0), Rectify.Left.R: [9 values, row-major] and the same three for Rectify.Right.*, with the optional scalars Rectify.Width / Rectify.Height (the raw
  // size; default Camera.width / Camera.height), Rectify.Border (0) and Rectify.Classes (0; 1: the class image of TrackStereoPairSemantic is raw too and
  // is remapped nearest-neighbour through the left map).  Camera.* then describes the RECTIFIED camera, Camera.bf the rectified baseline; flow, mask and
  // class images are taken as given in the rectified geometry.  A partial set, a wrong list length or the keys with an RGBD sensor are settings errors.
  // TrackStereo with the flow made on the device from imLeft and imLeftNext (Tracking::GrabImageStereoPair; settings keys Flow.Levels 6, Flow.Radius 2,
  // Flow.Window 2, Flow.Median 1, Flow.FBMaxDiff 1, Flow.SubPixel 1, all optional).  Exits like TrackStereo when the sensor is not STEREO.
  cv::Mat TrackStereoPair(const cv::Mat& imLeft, const cv::Mat& imRight, const cv::Mat& imLeftNext, const cv::Mat& masksem, const cv::Mat& mTcw_gt,
                          const std::vector<std::vector<float> >& vObjPose_gt, const double& timestamp, cv::Mat& imTraj, const int& nImage);
  // TrackStereoPair with the instance mask made on the device from a class image (Tracking::GrabImageStereoPairSemantic; settings keys
  // Labels.Connectivity 8, Labels.MaxDispDiff 512 (in 1/256 px: multiplied by DepthMapFactor / 256 into the units of the depth image),
  // Labels.MinArea 200, Labels.MaxLabels 1023, Stereo.SpeckleSize 0 (off), Stereo.SpeckleRange 256 (as MaxDispDiff), all optional).  Exits like
  // TrackStereo when the sensor is not STEREO.
  cv::Mat TrackStereoPairSemantic(const cv::Mat& imLeft, const cv::Mat& imRight, const cv::Mat& imLeftNext, const cv::Mat& classes, const cv::Mat& mTcw_gt,
                                  const std::vector<std::vector<float> >& vObjPose_gt, const double& timestamp, cv::Mat& imTraj, const int& nImage);
  // Raw stereo video in, trajectories out: TrackStereoPairSemantic with the class image made on the device from the next pair - the pixels that move
  // against the scene (Tracking::GrabImageStereoVideo).  Settings keys, all optional: Motion.SigmaFlow 0.5, Motion.SigmaDisp 0.5 (px), Motion.Chi2 9,
  // Motion.VoteRadius 2, Motion.VoteNum 1, Motion.VoteDen 2, Motion.MinKnown 6, Motion.MinDisparity Camera.bf / ThDepthBG (px), Motion.Class 1,
  // Motion.EgoStep 16, Motion.EgoThreshold 1.0, Motion.EgoIterations 500, Motion.EgoConfidence 0.98, Motion.EgoMinInliers 50.  A value outside its
  // range is a settings error with the STEREO sensor.  The caller is one frame ahead of the tracker, as with TrackStereoPair.  Exits like TrackStereo when
  // the sensor is not STEREO.
  cv::Mat TrackStereoVideo(const cv::Mat& imLeft, const cv::Mat& imRight, const cv::Mat& imLeftNext, const cv::Mat& imRightNext, const cv::Mat& mTcw_gt,
                           const std::vector<std::vector<float> >& vObjPose_gt, const double& timestamp, cv::Mat& imTraj, const int& nImage);
  // The dense map of the static scene.  Settings keys, all optional; the mapper exists only if Dense.VoxelSize (the voxel edge in metres) is present,
  // and without it nothing changes: Dense.Size [nx, ny, nz] ([256, 128, 256]), Dense.Truncation (4 x voxel), Dense.MinDepth (0), Dense.MaxDepth
  // (ThDepthBG), Dense.MaxWeight (64), Dense.MinWeight (2: the smallest weight of an extracted voxel), Dense.Anchor [ax, ay, az] in (0, 1), the camera
  // centre's target place in the volume ([0.5, 0.5, 0.25]), Dense.RecenterMargin in voxels (min(n) / 8).  A value outside its range is a settings error
  // with every sensor.  Every Track* entry fuses its frame once the pose is known (DenseMapper::FuseFrame): the volume follows the camera, and what
  // leaves it is kept as points on the host.  SaveDenseMap writes those points and the surface in the volume as a binary little-endian PLY (x, y, z,
  // nx, ny, nz, weight); false without a mapper or when the file cannot be written.  Limits: the map is fused with the tracker's per-frame poses - or,
  // with Dense.Align.Apply, with those poses refined against the map itself, which the tracker never sees - and is not re-fused after a bundle adjustment; an edge between a leaving and a staying voxel can be lost when the volume moves towards a negative axis;
  // objects are left out of this map (their own models: SaveObjectMaps below); with semantic masks on the RGBD path parked instances are left out too.
  bool SaveDenseMap(const std::string& path);
  // Settings key Dense.Mesh (0 or 1, default 0; read only with Dense.VoxelSize; another value is a settings error with every sensor).  With 1 the
  // static map is also kept as connected triangles (vdo_mesh_extract, surface nets): before the volume moves, the quads that will not lie wholly
  // inside what stays are kept on the host, so no quad is lost or doubled at a seam - the loss on moves towards a negative axis named above has no
  // counterpart in the mesh.  SaveDenseMesh writes the kept pieces and the whole current volume as a binary little-endian PLY: the vertices as
  // SaveDenseMap writes its points, then `face` as uchar int lists of 3; pieces share no vertices.  False without a mapper, without Dense.Mesh or when
  // the file cannot be written.  Without the key no mesher is made and no frame does anything it did not do before.
  bool SaveDenseMesh(const std::string& path);
  // What the dense map predicts a camera at Tcw (4 x 4 CV_32F, world -> camera) would see (DenseMapper::Render, vdo_raycast_render): depth CV_32FC1 in
  // metres, 0 where no surface is met, and normals CV_32FC3 in the world frame, towards free space, 0 where the surface has an unseen neighbour - at the
  // camera's image size and K.  Settings keys, all optional and read only with Dense.VoxelSize: Dense.View.Near (max(Dense.MinDepth, Dense.VoxelSize)),
  // the z-depth of a ray's first sample; Dense.View.Step (Dense.Truncation / 2), the z-depth between samples; Dense.View.MinWeight (Dense.MinWeight);
  // a ray has ceil((Dense.MaxDepth - Near) / Step) + 1 samples, at most 65536.  A non-finite value, Step <= 0, Near < 0, Near >= Dense.MaxDepth or too
  // many samples is a settings error.  False without a mapper; nothing of the map or of the tracker changes.
  bool RenderDenseView(const cv::Mat& Tcw, cv::Mat& depth, cv::Mat& normals);
  // A coloured dense map.  Settings keys, all optional and read only with Dense.VoxelSize: Dense.Colour (0 or 1, default 0; another value is a settings
  // error with every sensor); Dense.Colour.Band (Dense.Truncation / 2; positive, at most Dense.Truncation), the distance in metres of z-depth from the
  // measured surface within which a voxel takes the pixel's colour; Dense.Colour.MaxWeight (Dense.MaxWeight; 1..255), the cap of the running mean's
  // weight; Dense.Colour.MinWeight (1; 1..255), the smallest colour weight of a voxel that counts when a colour is read.  With Dense.Colour: 1 every
  // Track* entry fuses its image after the frame's geometry, with the same pose: TrackRGBD the image it was handed (Camera.RGB says which channel
  // comes first), the stereo entries the left grey image, the files entry the grey image decoded on the device.  SaveDenseMap and SaveDenseMesh then
  // write red, green, blue, alpha (uchar) after weight; alpha is the share of the trilinear weight that had colour, 0 where none was fused.  What
  // leaves the volume is coloured before it leaves.  The object models stay uncoloured.  Without the key every file keeps today's bytes.
  // RenderDenseColour: RenderDenseView's depth image at Tcw, then the colour of its points as CV_8UC4 (red, green, blue, alpha).  False without a
  // mapper or without Dense.Colour.
  bool RenderDenseColour(const cv::Mat& Tcw, cv::Mat& rgba);
  // How much room a point has to the static scene (DenseMapper::Clearance, vdo_distance_*): the exact Euclidean distance to the nearest voxel at a zero
  // crossing of the map.  Settings keys, all optional and read only with Dense.VoxelSize: Dense.Distance (0 or 1, default 0; another value is a
  // settings error with every sensor); Dense.Distance.Radius (2.0 metres; positive and finite, ceil(Radius / Dense.VoxelSize) in 1..8191 voxels), the
  // distance beyond which a point is simply far; Dense.Distance.MinWeight (Dense.MinWeight; 1..255), the smallest weight of a voxel that counts.
  // Nothing runs per frame: the field of the whole current volume is computed when a query finds the map fused or moved since the last one.
  // DenseClearance: points n x 3 CV_32F in the world frame; metres CV_32FC1 n x 1, the distance (+inf beyond the radius, NaN for a point outside the
  // volume); state CV_8UC1 n x 1, 0 unknown, 1 free, 2 inside a surface, 255 outside the volume.  False without a mapper or without Dense.Distance.
  bool DenseClearance(const cv::Mat& points, cv::Mat& metres, cv::Mat& state);
  // For every live model of the object mapper: (mod_label, the clearance in metres at the world position of the model's origin - the translation of
  // its current Two), in the models' order.  False without Dense.Distance or without an object mapper.
  bool ObjectClearances(std::vector<std::pair<int, float> >& out);
  // How far a pose is from the geometry in the map (DenseMapper::Align, vdo_align_solve): imD (CV_32FC1 metres) and mask (CV_32SC1 or empty) of the
  // camera's image size are aligned by point-to-plane ICP against the map's view at Tcw (4 x 4 CV_32F, world -> camera); Tcw_out receives the refined
  // pose (Tcw itself unless LastDenseAlignment's status is 0).  False without a mapper; nothing of the map or of the tracker changes.  Settings keys,
  // all optional and read only with Dense.VoxelSize: Dense.Align.Iterations (0: off; 1..64: every Track* entry aligns its frame against the map at the
  // tracker's pose before it fuses, and keeps the report), Dense.Align.MaxDist (Dense.Truncation), Dense.Align.Subsample (1; 1..8),
  // Dense.Align.MinPixels (a sixteenth of the sample grid; at least 6), Dense.Align.Apply (0; 1: the frame is fused with the aligned pose when the
  // alignment's status is 0, with the tracker's pose otherwise - on the first frame, for instance, when the map is empty).  The TRACKER's trajectory
  // is the same bytes in every case.  A value outside its range is a settings error.
  bool AlignDenseView(const cv::Mat& Tcw, const cv::Mat& imD, const cv::Mat& mask, cv::Mat& Tcw_out);
  // The report of the last alignment - of AlignDenseView, or of the last frame with Dense.Align.Iterations > 0, whichever came later.  False when
  // there has been none.
  bool LastDenseAlignment(vdo_align_report& report) const;
  // AlignDenseView with the photometric term (DenseMapper::AlignPhoto, vdo_photo_solve): image (CV_8U, 1, 3 or 4 channels, in the order of Camera.RGB)
  // is the frame's image; the intensity term compares it with the last frame the tracker kept as its model frame.  False without a mapper or without
  // Dense.Align.Photo.  Settings keys, read only with Dense.VoxelSize and Dense.Align.Iterations > 0: Dense.Align.Photo (0 or absent: off; a positive
  // value: the weight of a grey level in metres - every Track* entry then aligns its frame jointly and keeps the fused frame as the next model frame;
  // there is no default weight), Dense.Align.Photo.MaxDiff (255; (0, 255]), Dense.Align.Photo.MinPixels (Dense.Align.MinPixels).  The first frame,
  // and a frame whose joint solve ends with status 1, is aligned by the geometry alone.  Dense.Align.Apply keeps its meaning.
  bool AlignDenseViewPhoto(const cv::Mat& Tcw, const cv::Mat& imD, const cv::Mat& mask, const cv::Mat& image, cv::Mat& Tcw_out);
  // The joint report of the last alignment with the photometric term - of AlignDenseViewPhoto or of the last frame, whichever came later.
  bool LastDensePhotoAlignment(vdo_photo_report& report) const;
  // A dense model per tracked object (ObjectMapper).  Settings keys, read only with Dense.VoxelSize; the object mapper exists only if
  // Dense.Objects.VoxelSize (the voxel edge in metres) is present as well, and without it nothing changes: Dense.Objects.Size [nx, ny, nz] ([96, 64, 96]),
  // Dense.Objects.Truncation (4 x voxel), Dense.Objects.MaxDepth (ThDepthOBJ; above Dense.MinDepth, which is the objects' too), Dense.Objects.MaxObjects
  // (16; 1..64 live models), Dense.Objects.MinPixels (200: the pixels a label needs to start a model or to be fused), Dense.Objects.MinFrames (3: a
  // retired model fused in fewer frames is dropped), Dense.Objects.MinWeight (Dense.MinWeight); the weight cap is Dense.MaxWeight.  A value outside its
  // range is a settings error.  Every Track* entry runs the object stage right after the static map's frame, with the pose that map was fused with
  // and the step's object motions (mod_label: the tracking id; sem_label: the label the object's pixels carry in the frame's repaired mask; H: the
  // world-frame motion from the last frame).  Limits: a model is fused with the tracker's per-frame motions and not re-fused after a bundle
  // adjustment; free space is not carved from other labels' pixels; an object that comes back under a new tracking id starts a new model; in the
  // shell's throughput mode (the object stage of a frame ends inside the next call) the motions at hand are the last frame's, and the object stage is skipped.
  // SaveObjectMaps: <prefix>_<mod_label>.ply per finished and live model in the OBJECT frame and <prefix>_poses.txt (frame, mod_label, the 16
  // entries of Two); false without an object mapper or when a file cannot be written.
  bool SaveObjectMaps(const std::string& prefix);
  // With Dense.Mesh: 1 the object mapper also meshes every model (whole volume; a model that is retired is meshed then, next to its points).
  // SaveObjectMeshes writes <prefix>_<mod_label>_mesh.ply per finished and live model in the OBJECT frame, in the layout of SaveDenseMesh.  False
  // without an object mapper, without Dense.Mesh or when a file cannot be written.
  bool SaveObjectMeshes(const std::string& prefix);
  // What the model of the live object mod_label predicts a camera at Tcw (4 x 4 CV_32F, world -> camera) would see: depth CV_32FC1, normals CV_32FC3 in
  // the object frame.  False without an object mapper or a live model of that id.
  bool RenderObjectView(int mod_label, const cv::Mat& Tcw, cv::Mat& depth, cv::Mat& normals);
  // The finished models, then the live ones: per model mod_label, live (0 / 1), frames fused, points.  Returns their number, -1 without an object
  // mapper; counts2 (may be null): objects dropped (MinFrames) and skipped (MaxObjects, MinPixels) so far.
  int ObjectModelInfo(std::vector<std::array<long long, 4> >& rows, long long counts2[2] = nullptr);
  void SaveResults(const std::string& filename);
  Map* map();                          // brought up to date from the pipeline's GraphStore on access
  Tracking* tracker() { return mpTracker; }

 private:
  eSensor mSensor;
  Map* mpMap;
  Tracking* mpTracker;
  vdo_align_report view_align_{};      // of the last AlignDenseView
  bool view_align_valid_ = false;
  long long view_align_at_ = 0;        // the frames the tracker had aligned when AlignDenseView ran: a later frame's report is the newer one
  vdo_photo_report view_photo_{};      // of the last AlignDenseViewPhoto
  bool view_photo_valid_ = false;
  long long view_photo_at_ = 0;
};

}  // namespace VDO_SLAM
