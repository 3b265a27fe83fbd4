// ORBmatcher - ORB-SLAM2's familiar surface (TH_LOW / TH_HIGH, DescriptorDistance, nnratio) over the device matcher of
// libvdo_hip (vdo_orb_match*).  The reference keeps the skeleton such a class plugs into (mDescriptors, mvKeysUn) but ships
// no matcher; what a match is, is stated in include/vdo_slam_hip.h.
#pragma once
#include <vector>

#include "ORBextractor.h"
#include "host_context.h"
#include "minicv.h"

namespace VDO_SLAM {

class ORBmatcher {
 public:
  static const int TH_LOW = 50;
  static const int TH_HIGH = 100;
  // nnratio: best < nnratio * second (off outside (0, 1)); crossCheck: keep mutual bests only
  ORBmatcher(float nnratio = 0.6f, bool crossCheck = true);
  // Hamming distance of two 32-byte descriptor rows (host popcount)
  static int DescriptorDistance(const cv::Mat& a, const cv::Mat& b);
  // Brute-force match of descQ (CV_8U, n x 32, row i belongs to keysQ[i]) against descT.  window: half-width of the search square
  // around the query's position in pixels (< 0: anywhere); maxOctaveDiff: largest |octave difference| (< 0: any); maxDistance: 0..256.
  // matchesQT[i] = index into keysT, or -1; dist (optional) [i] = best distance, -1 without a candidate.  Returns the number of matches.
  int Match(const std::vector<cv::KeyPoint>& keysQ, const cv::Mat& descQ, const std::vector<cv::KeyPoint>& keysT, const cv::Mat& descT, float window,
            int maxOctaveDiff, int maxDistance, std::vector<int>& matchesQT, std::vector<int>* dist = nullptr);
  // The same between the keypoints the two extractors returned last, descriptors and keypoints staying on the device
  int Match(ORBextractor& extQ, ORBextractor& extT, float window, int maxOctaveDiff, int maxDistance, std::vector<int>& matchesQT,
            std::vector<int>* dist = nullptr);

 protected:
  float mfNNratio;
  bool mbCrossCheck;
};

}  // namespace VDO_SLAM
