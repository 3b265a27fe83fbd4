// StereoRectifier host class: checks the cv::Mats and calls the device rectifier (vdo_rectify_compute / vdo_rectify_gate).
#include "StereoRectifier.h"

#include <stdexcept>
#include <string>

namespace VDO_SLAM {

static void die(const char* what) {   // (as StereoMatcher.cc: a failure surfaces as an exception the flat hooks turn into a return code)
  throw std::runtime_error(std::string("VDO_SLAM::StereoRectifier: ") + what + ": " + vdo_last_error());
}

StereoRectifier::StereoRectifier(vdo_ctx* ctx, const vdo_rectify_params& params) : w_(params.width), h_px_(params.height), n_cams_(params.n_cams) {
  if (vdo_rectify_create(ctx ? ctx : HostContext(), &params, &h_) != VDO_OK) die("vdo_rectify_create");
  for (int c = 0; c < n_cams_ && c < 2; ++c) { sw_[c] = params.cam[c].src_width; sh_[c] = params.cam[c].src_height; }
}

StereoRectifier::~StereoRectifier() { vdo_rectify_destroy(h_); }

std::vector<cv::Mat> StereoRectifier::Rectify(const std::vector<cv::Mat>& raw, const std::vector<int>& cams, bool rgbOrder, const std::vector<int>& nearest, int border) {
  if (raw.empty() || raw.size() > 4) throw std::runtime_error("VDO_SLAM::StereoRectifier: 1 to 4 images per call");
  if ((!cams.empty() && cams.size() != raw.size()) || (!nearest.empty() && nearest.size() != raw.size()))
    throw std::runtime_error("VDO_SLAM::StereoRectifier: cams and nearest must be empty or as long as the image list");
  std::vector<cv::Mat> out(raw.size());
  vdo_rectify_job jobs[4];
  for (size_t k = 0; k < raw.size(); ++k) {
    const cv::Mat& m = raw[k];
    const int cam = cams.empty() ? 0 : cams[k];
    if (cam < 0 || cam >= n_cams_) throw std::runtime_error("VDO_SLAM::StereoRectifier: camera index out of range");
    if (m.empty() || m.rows != sh_[cam] || m.cols != sw_[cam] || m.depth() != cv::CV_8U || m.channels() == 2 || m.channels() > 4)
      throw std::runtime_error("VDO_SLAM::StereoRectifier: an image must be CV_8UC1 / C3 / C4 of its camera's source size");
    out[k].create(h_px_, w_, cv::CV_8UC1);
    jobs[k] = vdo_rectify_job{m.data, (int64_t)m.step, m.channels(), rgbOrder ? 1 : 0, cam, nearest.empty() ? 0 : nearest[k], out[k].data, (int64_t)out[k].step};
  }
  if (vdo_rectify_compute(h_, jobs, (int)raw.size(), 0, 0, border) != VDO_OK) die("vdo_rectify_compute");
  return out;
}

int StereoRectifier::Gate(cv::Mat& image, int cam) {
  if (image.empty() || image.rows != h_px_ || image.cols != w_ || image.depth() != cv::CV_32F || image.channels() != 1 || image.step % sizeof(float))
    throw std::runtime_error("VDO_SLAM::StereoRectifier: the image must be CV_32FC1 of the rectifier's destination size");
  int32_t n = 0;
  if (vdo_rectify_gate(h_, cam, (float*)image.data, (int64_t)(image.step / sizeof(float)), 0, &n) != VDO_OK) die("vdo_rectify_gate");
  return n;
}

}  // namespace VDO_SLAM
