// FlowMatcher - dense optical flow by a coarse-to-fine census search on the device (vdo_optflow_* of libvdo_hip) behind a cv::Mat surface.  The
// reference consumes one flow image per frame (the flow from that frame to the next) and leaves making it to an offline network; what a flow is
// here, is stated in include/vdo_slam_hip.h.
#pragma once
#include "host_context.h"
#include "minicv.h"

namespace VDO_SLAM {

class FlowMatcher {
 public:
  // The settings file's Flow.* defaults: levels, radius, window, median, fb_max_diff, subpixel
  static vdo_optflow_params DefaultParams() { return vdo_optflow_params{6, 2, 2, 1, 1, 1}; }
  // A matcher for width x height images on `ctx` (HostContext() when null).  Throws std::runtime_error when the library refuses.
  FlowMatcher(vdo_ctx* ctx, int width, int height, const vdo_optflow_params& params);
  ~FlowMatcher();
  FlowMatcher(const FlowMatcher&) = delete;
  FlowMatcher& operator=(const FlowMatcher&) = delete;
  // im0 / im1: CV_8UC1, width x height, any row step.  Returns the flow from im0 to im1 as CV_32FC2 (u, v; written for every pixel); valid
  // (optional) becomes CV_8UC1 with 1 where the forward-backward check passed, nValid (optional) their number.
  cv::Mat Compute(const cv::Mat& im0, const cv::Mat& im1, cv::Mat* valid = nullptr, int* nValid = nullptr);
  vdo_optflow* handle() { return h_; }
  int width() const { return w_; }
  int height() const { return h_px_; }

 private:
  vdo_optflow* h_ = nullptr;
  int w_, h_px_;
};

}  // namespace VDO_SLAM
