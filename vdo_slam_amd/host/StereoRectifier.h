// StereoRectifier - lens undistortion and rectification of the raw images of one or two cameras on the device (vdo_rectify_* of libvdo_hip) behind
// a cv::Mat surface.  The reference's stereo example does this with cv::initUndistortRectifyMap + cv::remap before its System sees an image; what
// the map and the interpolation are here, is stated in include/vdo_slam_hip.h.
#pragma once
#include <vector>

#include "host_context.h"
#include "minicv.h"

namespace VDO_SLAM {

class StereoRectifier {
 public:
  // A rectifier for params.n_cams cameras on `ctx` (HostContext() when null).  Throws std::runtime_error when the library refuses.
  StereoRectifier(vdo_ctx* ctx, const vdo_rectify_params& params);
  ~StereoRectifier();
  StereoRectifier(const StereoRectifier&) = delete;
  StereoRectifier& operator=(const StereoRectifier&) = delete;
  // raw: 1 to 4 images, CV_8UC1 / C3 / C4 of their camera's source size, any row step; cams: the camera of each (empty: all camera 0); nearest: per
  // image, one channel only (empty: none).  One device call for all of them.  Returns the rectified grey images, CV_8UC1 of the destination size.
  std::vector<cv::Mat> Rectify(const std::vector<cv::Mat>& raw, const std::vector<int>& cams, bool rgbOrder, const std::vector<int>& nearest = std::vector<int>(),
                               int border = 0);
  // In place on a CV_32FC1 image of the destination size (any row step): 0 wherever cam's map is invalid.  Returns the number of values changed.
  int Gate(cv::Mat& image, int cam);
  vdo_rectify* handle() { return h_; }
  int width() const { return w_; }
  int height() const { return h_px_; }
  int srcWidth(int cam) const { return sw_[cam]; }
  int srcHeight(int cam) const { return sh_[cam]; }

 private:
  vdo_rectify* h_ = nullptr;
  int w_, h_px_, n_cams_, sw_[2] = {0, 0}, sh_[2] = {0, 0};
};

}  // namespace VDO_SLAM
