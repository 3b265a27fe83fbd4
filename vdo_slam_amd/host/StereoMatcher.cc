// StereoMatcher host class: checks the two cv::Mat and calls the device matcher (vdo_stereo_compute).
#include "StereoMatcher.h"

#include <stdexcept>
#include <string>

namespace VDO_SLAM {

static void die(const char* what) {   // (as ORBmatcher.cc: a failure surfaces as an exception the flat hooks turn into a return code)
  throw std::runtime_error(std::string("VDO_SLAM::StereoMatcher: ") + what + ": " + vdo_last_error());
}

StereoMatcher::StereoMatcher(vdo_ctx* ctx, int width, int height, const vdo_stereo_params& params) : w_(width), h_px_(height) {
  if (vdo_stereo_create(ctx ? ctx : HostContext(), width, height, &params, &h_) != VDO_OK) die("vdo_stereo_create");
}

StereoMatcher::~StereoMatcher() { vdo_stereo_destroy(h_); }

cv::Mat StereoMatcher::Compute(const cv::Mat& left, const cv::Mat& right, int* nValid) {
  for (const cv::Mat* m : {&left, &right})
    if (m->empty() || m->rows != h_px_ || m->cols != w_ || m->depth() != cv::CV_8U || m->channels() != 1)
      throw std::runtime_error("VDO_SLAM::StereoMatcher: images must be CV_8UC1 of the matcher's size");
  cv::Mat disp(h_px_, w_, cv::CV_32F);
  int32_t n = 0;
  if (vdo_stereo_compute(h_, left.data, (int64_t)left.step, right.data, (int64_t)right.step, 0, (float*)disp.data, 0, &n) != VDO_OK) die("vdo_stereo_compute");
  if (nValid) *nValid = n;
  return disp;
}

}  // namespace VDO_SLAM
