// InstanceLabeler - connected components of a class image to the instance mask the tracker takes, and a disparity speckle filter, on the device
// (vdo_labels_* of libvdo_hip) behind a cv::Mat surface.  The reference consumes one instance mask per frame and leaves making it to an offline
// segmentation network; what a label is here, is stated in include/vdo_slam_hip.h.
#pragma once
#include "host_context.h"
#include "minicv.h"

namespace VDO_SLAM {

class InstanceLabeler {
 public:
  // The settings file's Labels.* defaults: connectivity, max_disp_diff, min_area, max_labels
  static vdo_labels_params DefaultParams() { return vdo_labels_params{8, 512, 200, 1023}; }
  // A labeller for width x height images on `ctx` (HostContext() when null).  Throws std::runtime_error when the library refuses.
  InstanceLabeler(vdo_ctx* ctx, int width, int height, const vdo_labels_params& params);
  ~InstanceLabeler();
  InstanceLabeler(const InstanceLabeler&) = delete;
  InstanceLabeler& operator=(const InstanceLabeler&) = delete;
  // classes: CV_8UC1, disparity: CV_32FC1 or empty (only with max_disp_diff -1), width x height, any row step.  Returns the mask as CV_32SC1
  // (0 = background, 1..n); counts (optional) receives n_labels, n_components, area_threshold.
  cv::Mat Compute(const cv::Mat& classes, const cv::Mat& disparity, int counts[3] = nullptr);
  // In place on a continuous CV_32FC1 image: components of at most maxSize pixels become 0.  Returns the number of pixels zeroed.
  int FilterSpeckles(cv::Mat& disparity, int maxDiff, int maxSize);
  vdo_labels* handle() { return h_; }
  int width() const { return w_; }
  int height() const { return h_px_; }

 private:
  vdo_labels* h_ = nullptr;
  int w_, h_px_;
};

}  // namespace VDO_SLAM
