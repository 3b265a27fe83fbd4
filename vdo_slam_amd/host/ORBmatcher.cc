// ORBmatcher host class: marshals keypoints / descriptors into vdo_match_set and calls the device matcher (vdo_orb_match*).
#include "ORBmatcher.h"

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>

namespace VDO_SLAM {

static void die(const char* what) {   // (as ORBextractor.cc: a failure surfaces as an exception the flat hooks turn into a return code)
  throw std::runtime_error(std::string("VDO_SLAM::ORBmatcher: ") + what + ": " + vdo_last_error());
}

ORBmatcher::ORBmatcher(float nnratio, bool crossCheck) : mfNNratio(nnratio), mbCrossCheck(crossCheck) {}

int ORBmatcher::DescriptorDistance(const cv::Mat& a, const cv::Mat& b) {
  int dist = 0;
  for (int i = 0; i < 4; ++i) {
    uint64_t x, y;
    std::memcpy(&x, a.data + 8 * i, 8); std::memcpy(&y, b.data + 8 * i, 8);
    dist += __builtin_popcountll(x ^ y);
  }
  return dist;
}

namespace {
struct FlatSet {
  std::vector<uint8_t> desc; std::vector<float> x, y; std::vector<int32_t> oct;
  vdo_match_set set{};
  FlatSet(const std::vector<cv::KeyPoint>& keys, const cv::Mat& d) {
    const int n = (int)keys.size();
    if (n && (d.rows != n || d.cols != 32 || d.depth() != cv::CV_8U || d.channels() != 1)) throw std::runtime_error("VDO_SLAM::ORBmatcher: descriptors must be CV_8U, keys x 32");
    desc.resize(32 * (size_t)n + 32); x.resize(n + 1); y.resize(n + 1); oct.resize(n + 1);
    for (int i = 0; i < n; ++i) {
      std::memcpy(desc.data() + 32 * (size_t)i, d.data + (size_t)i * d.step, 32);
      x[i] = keys[i].pt.x; y[i] = keys[i].pt.y; oct[i] = keys[i].octave;
    }
    set.n = n; set.desc = desc.data(); set.x = x.data(); set.y = y.data(); set.octave = oct.data(); set.is_device = 0;
  }
};
}  // namespace

int ORBmatcher::Match(const std::vector<cv::KeyPoint>& keysQ, const cv::Mat& descQ, const std::vector<cv::KeyPoint>& keysT, const cv::Mat& descT, float window,
                      int maxOctaveDiff, int maxDistance, std::vector<int>& matchesQT, std::vector<int>* dist) {
  FlatSet Q(keysQ, descQ), T(keysT, descT);
  const vdo_match_params p{maxDistance, mfNNratio, window, maxOctaveDiff, mbCrossCheck ? 1 : 0, 0};
  const int n = Q.set.n;
  std::vector<int32_t> idx(n + 1), best(n + 1), second(n + 1);
  int32_t m = 0;
  if (vdo_orb_match(HostContext(), &Q.set, &T.set, &p, idx.data(), best.data(), second.data(), &m) != VDO_OK) die("vdo_orb_match");
  matchesQT.assign(idx.begin(), idx.begin() + n);
  if (dist) dist->assign(best.begin(), best.begin() + n);
  return m;
}

int ORBmatcher::Match(ORBextractor& extQ, ORBextractor& extT, float window, int maxOctaveDiff, int maxDistance, std::vector<int>& matchesQT, std::vector<int>* dist) {
  matchesQT.clear();
  if (dist) dist->clear();
  if (!extQ.handle() || !extT.handle()) return 0;            // nothing extracted yet
  int n = 0;
  if (vdo_orb_last_keypoints(extQ.handle(), &n) != VDO_OK) die("vdo_orb_last_keypoints");
  const vdo_match_params p{maxDistance, mfNNratio, window, maxOctaveDiff, mbCrossCheck ? 1 : 0, 0};
  std::vector<int32_t> idx(n + 1), best(n + 1), second(n + 1);
  int32_t m = 0;
  if (vdo_orb_match_extractors(extQ.handle(), extT.handle(), &p, idx.data(), best.data(), second.data(), &m, n) != VDO_OK) die("vdo_orb_match_extractors");
  matchesQT.assign(idx.begin(), idx.begin() + n);
  if (dist) dist->assign(best.begin(), best.begin() + n);
  return m;
}

}  // namespace VDO_SLAM
