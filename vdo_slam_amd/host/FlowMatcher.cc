// FlowMatcher host class: checks the two cv::Mat and calls the device matcher (vdo_optflow_compute).
#include "FlowMatcher.h"

#include <stdexcept>
#include <string>

namespace VDO_SLAM {

static void die(const char* what) {   // (as StereoMatcher.cc: a failure surfaces as an exception the flat hooks turn into a return code)
  throw std::runtime_error(std::string("VDO_SLAM::FlowMatcher: ") + what + ": " + vdo_last_error());
}

FlowMatcher::FlowMatcher(vdo_ctx* ctx, int width, int height, const vdo_optflow_params& params) : w_(width), h_px_(height) {
  if (vdo_optflow_create(ctx ? ctx : HostContext(), width, height, &params, &h_) != VDO_OK) die("vdo_optflow_create");
}

FlowMatcher::~FlowMatcher() { vdo_optflow_destroy(h_); }

cv::Mat FlowMatcher::Compute(const cv::Mat& im0, const cv::Mat& im1, cv::Mat* valid, int* nValid) {
  for (const cv::Mat* m : {&im0, &im1})
    if (m->empty() || m->rows != h_px_ || m->cols != w_ || m->depth() != cv::CV_8U || m->channels() != 1)
      throw std::runtime_error("VDO_SLAM::FlowMatcher: images must be CV_8UC1 of the matcher's size");
  cv::Mat flow(h_px_, w_, cv::CV_32FC2);
  if (valid) *valid = cv::Mat(h_px_, w_, cv::CV_8UC1);
  int32_t n = 0;
  if (vdo_optflow_compute(h_, im0.data, (int64_t)im0.step, im1.data, (int64_t)im1.step, 0, (float*)flow.data, valid ? valid->data : nullptr, 0, &n) != VDO_OK)
    die("vdo_optflow_compute");
  if (nValid) *nValid = n;
  return flow;
}

}  // namespace VDO_SLAM
