// MotionSegmenter host class: checks the cv::Mats and calls the device segmenter (vdo_motionseg_compute / vdo_motionseg_egomotion).
#include "MotionSegmenter.h"

#include <cstring>
#include <stdexcept>
#include <string>

namespace VDO_SLAM {

static void die(const char* what) {   // (as InstanceLabeler.cc: a failure surfaces as an exception the flat hooks turn into a return code)
  throw std::runtime_error(std::string("VDO_SLAM::MotionSegmenter: ") + what + ": " + vdo_last_error());
}

MotionSegmenter::MotionSegmenter(vdo_ctx* ctx, int width, int height, const vdo_motionseg_params& params) : w_(width), h_px_(height) {
  if (vdo_motionseg_create(ctx ? ctx : HostContext(), width, height, &params, &h_) != VDO_OK) die("vdo_motionseg_create");
}

MotionSegmenter::~MotionSegmenter() { vdo_motionseg_destroy(h_); }

void MotionSegmenter::CheckSources(const cv::Mat& disparity0, const cv::Mat& flow, const cv::Mat& flowValid) const {
  auto image = [&](const cv::Mat& m, int depth, int channels, size_t unit) {
    return !m.empty() && m.rows == h_px_ && m.cols == w_ && m.depth() == depth && m.channels() == channels && m.step % unit == 0;
  };
  if (!image(disparity0, cv::CV_32F, 1, sizeof(float))) throw std::runtime_error("VDO_SLAM::MotionSegmenter: a disparity must be CV_32FC1 of the segmenter's size");
  if (!image(flow, cv::CV_32F, 2, sizeof(float))) throw std::runtime_error("VDO_SLAM::MotionSegmenter: flow must be CV_32FC2 of the segmenter's size");
  if (!flowValid.empty() && !image(flowValid, cv::CV_8U, 1, 1)) throw std::runtime_error("VDO_SLAM::MotionSegmenter: flowValid must be empty or CV_8UC1 of the segmenter's size");
}

cv::Mat MotionSegmenter::Compute(const cv::Mat& disparity0, const cv::Mat& disparity1, const cv::Mat& flow, const cv::Mat& flowValid, const cv::Mat& T, int counts[3]) {
  CheckSources(disparity0, flow, flowValid);
  CheckSources(disparity1, flow, flowValid);
  if (T.empty() || T.rows != 4 || T.cols != 4 || T.depth() != cv::CV_32F || T.channels() != 1 || T.step != 4 * sizeof(float))
    throw std::runtime_error("VDO_SLAM::MotionSegmenter: T must be a continuous 4 x 4 CV_32F");
  cv::Mat cls(h_px_, w_, cv::CV_8UC1);
  int32_t out[3] = {0, 0, 0};
  if (vdo_motionseg_compute(h_, (const float*)disparity0.data, (int64_t)(disparity0.step / sizeof(float)), (const float*)disparity1.data,
                            (int64_t)(disparity1.step / sizeof(float)), (const float*)flow.data, (int64_t)(flow.step / sizeof(float)), flowValid.empty() ? nullptr : flowValid.data,
                            flowValid.empty() ? 0 : (int64_t)flowValid.step, 0, (const float*)T.data, cls.data, 0, out) != VDO_OK)
    die("vdo_motionseg_compute");
  if (counts) for (int k = 0; k < 3; ++k) counts[k] = out[k];
  return cls;
}

cv::Mat MotionSegmenter::EgoMotion(const cv::Mat& disparity0, const cv::Mat& flow, const cv::Mat& flowValid, const EgoParams& ego, int counts[3]) {
  CheckSources(disparity0, flow, flowValid);
  cv::Mat T(4, 4, cv::CV_32F);
  int32_t out[3] = {0, 0, 0};
  if (vdo_motionseg_egomotion(h_, (const float*)disparity0.data, (int64_t)(disparity0.step / sizeof(float)), (const float*)flow.data, (int64_t)(flow.step / sizeof(float)),
                              flowValid.empty() ? nullptr : flowValid.data, flowValid.empty() ? 0 : (int64_t)flowValid.step, 0, ego.step, ego.iterations, ego.threshold,
                              ego.confidence, ego.minInliers, (float*)T.data, out) != VDO_OK)
    die("vdo_motionseg_egomotion");
  if (counts) for (int k = 0; k < 3; ++k) counts[k] = out[k];
  return T;
}

}  // namespace VDO_SLAM
