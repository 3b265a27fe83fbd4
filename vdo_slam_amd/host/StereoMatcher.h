// StereoMatcher - census + semi-global matching on the device (vdo_stereo_* of libvdo_hip) behind a cv::Mat surface.  The reference
// consumes disparity maps x 256 (src/Tracking.cc:180-204) and leaves making them to an offline matcher; what a disparity is here, is
// stated in include/vdo_slam_hip.h.
#pragma once
#include "host_context.h"
#include "minicv.h"

namespace VDO_SLAM {

class StereoMatcher {
 public:
  // The settings file's Stereo.* defaults
  static vdo_stereo_params DefaultParams() { return vdo_stereo_params{128, 10, 120, 8, 5, 1, 1}; }
  // A matcher for width x height images on `ctx` (HostContext() when null).  Throws std::runtime_error when the library refuses.
  StereoMatcher(vdo_ctx* ctx, int width, int height, const vdo_stereo_params& params);
  ~StereoMatcher();
  StereoMatcher(const StereoMatcher&) = delete;
  StereoMatcher& operator=(const StereoMatcher&) = delete;
  // left / right: CV_8UC1, width x height, any row step.  Returns disparity x 256 as CV_32F (0 = invalid); nValid (optional) the
  // number of valid pixels.
  cv::Mat Compute(const cv::Mat& left, const cv::Mat& right, int* nValid = nullptr);
  vdo_stereo* handle() { return h_; }
  int width() const { return w_; }
  int height() const { return h_px_; }

 private:
  vdo_stereo* h_ = nullptr;
  int w_, h_px_;
};

}  // namespace VDO_SLAM
