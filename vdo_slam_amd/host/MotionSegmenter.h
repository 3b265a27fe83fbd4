// MotionSegmenter - the class image of the pixels that move against the scene, from two disparity images, the flow between them and the camera
// motion, and the camera motion from the same images, on the device (vdo_motionseg_* of libvdo_hip) behind a cv::Mat surface.  The reference takes
// the class of every pixel from an offline segmentation network; what "moving" means here is stated in include/vdo_slam_hip.h.
#pragma once
#include "host_context.h"
#include "minicv.h"

namespace VDO_SLAM {

class MotionSegmenter {
 public:
  // The settings file's Motion.* defaults around a camera: K = (fx, fy, cx, cy), bf, the disparity images' unit (DepthMapFactor) and
  // Motion.MinDisparity in pixels (the settings default is Camera.bf / ThDepthBG)
  static vdo_motionseg_params DefaultParams(const float K[4], float bf, float dispUnit, float minDisparity) {
    return vdo_motionseg_params{{K[0], K[1], K[2], K[3]}, bf, dispUnit, 0.5f, 0.5f, 9.f, minDisparity, 2, 1, 2, 6, 1};
  }
  // The ego-motion's settings (Motion.Ego*) and their defaults
  struct EgoParams { int step = 16; double threshold = 1.0; int iterations = 500; double confidence = 0.98; int minInliers = 50; };
  // A segmenter for width x height images on `ctx` (HostContext() when null).  Throws std::runtime_error when the library refuses.
  MotionSegmenter(vdo_ctx* ctx, int width, int height, const vdo_motionseg_params& params);
  ~MotionSegmenter();
  MotionSegmenter(const MotionSegmenter&) = delete;
  MotionSegmenter& operator=(const MotionSegmenter&) = delete;
  // disparity0 / disparity1: CV_32FC1, flow: CV_32FC2, flowValid: CV_8UC1 or empty, width x height, any row step; T: 4 x 4 CV_32F, camera t + 1
  // from camera t.  Returns the class image as CV_8UC1; counts (optional) receives the moving, static and unknown pixel counts.
  cv::Mat Compute(const cv::Mat& disparity0, const cv::Mat& disparity1, const cv::Mat& flow, const cv::Mat& flowValid, const cv::Mat& T, int counts[3] = nullptr);
  // The camera motion from t to t + 1 as a 4 x 4 CV_32F (the identity with fewer than ego.minInliers inliers); counts (optional) receives
  // n_samples, n_inliers, iterations_run.
  cv::Mat EgoMotion(const cv::Mat& disparity0, const cv::Mat& flow, const cv::Mat& flowValid, const EgoParams& ego, int counts[3] = nullptr);
  vdo_motionseg* handle() { return h_; }
  int width() const { return w_; }
  int height() const { return h_px_; }

 private:
  void CheckSources(const cv::Mat& disparity0, const cv::Mat& flow, const cv::Mat& flowValid) const;
  vdo_motionseg* h_ = nullptr;
  int w_, h_px_;
};

}  // namespace VDO_SLAM
