// InstanceLabeler host class: checks the cv::Mat and calls the device labeller (vdo_labels_compute / vdo_labels_filter_speckles).
#include "InstanceLabeler.h"

#include <stdexcept>
#include <string>

namespace VDO_SLAM {

static void die(const char* what) {   // (as StereoMatcher.cc: a failure surfaces as an exception the flat hooks turn into a return code)
  throw std::runtime_error(std::string("VDO_SLAM::InstanceLabeler: ") + what + ": " + vdo_last_error());
}

InstanceLabeler::InstanceLabeler(vdo_ctx* ctx, int width, int height, const vdo_labels_params& params) : w_(width), h_px_(height) {
  if (vdo_labels_create(ctx ? ctx : HostContext(), width, height, &params, &h_) != VDO_OK) die("vdo_labels_create");
}

InstanceLabeler::~InstanceLabeler() { vdo_labels_destroy(h_); }

cv::Mat InstanceLabeler::Compute(const cv::Mat& classes, const cv::Mat& disparity, int counts[3]) {
  if (classes.empty() || classes.rows != h_px_ || classes.cols != w_ || classes.depth() != cv::CV_8U || classes.channels() != 1)
    throw std::runtime_error("VDO_SLAM::InstanceLabeler: classes must be CV_8UC1 of the labeller's size");
  if (!disparity.empty() && (disparity.rows != h_px_ || disparity.cols != w_ || disparity.depth() != cv::CV_32F || disparity.channels() != 1 || disparity.step % sizeof(float)))
    throw std::runtime_error("VDO_SLAM::InstanceLabeler: disparity must be empty or CV_32FC1 of the labeller's size");
  cv::Mat mask(h_px_, w_, cv::CV_32SC1);
  int32_t out[3] = {0, 0, 0};
  if (vdo_labels_compute(h_, classes.data, (int64_t)classes.step, disparity.empty() ? nullptr : (const float*)disparity.data,
                         disparity.empty() ? 0 : (int64_t)(disparity.step / sizeof(float)), 0, (int32_t*)mask.data, 0, out) != VDO_OK)
    die("vdo_labels_compute");
  if (counts) for (int k = 0; k < 3; ++k) counts[k] = out[k];
  return mask;
}

int InstanceLabeler::FilterSpeckles(cv::Mat& disparity, int maxDiff, int maxSize) {
  if (disparity.empty() || disparity.rows != h_px_ || disparity.cols != w_ || disparity.depth() != cv::CV_32F || disparity.channels() != 1 ||
      disparity.step != (size_t)w_ * sizeof(float))
    throw std::runtime_error("VDO_SLAM::InstanceLabeler: disparity must be a continuous CV_32FC1 image of the labeller's size");
  int32_t n = 0;
  if (vdo_labels_filter_speckles(h_, (float*)disparity.data, 0, maxDiff, maxSize, &n) != VDO_OK) die("vdo_labels_filter_speckles");
  return n;
}

}  // namespace VDO_SLAM
