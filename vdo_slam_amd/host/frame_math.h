// The small float arithmetic of the per-frame sequence, written once: plain C++, no GPU, no vdo_* types (tests/test_frame_math.py compiles it alone).
// Every loop is in float, left to right, the way cv::gemm's 2..4-wide fast path works (the untransposed small products of the reference - Tcw * H, R * x + t);
// the build keeps -ffp-contract=off, so none of it fuses into a multiply-add.
#pragma once
#include <cmath>
#include <cstdint>

namespace VDO_SLAM::frame_math {

constexpr float kI4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// Converter::toInvMatrix (src/Converter.cc:151-166): t_inv = -R.t() * t is a cv::gemm with a TRANSPOSED operand (GEMM_1_T), which OpenCV 3.4 runs
// through its generic GEMMSingleMul<float, double>: the dot product accumulated in double, k ascending, times alpha = -1, ONE rounding to float.
inline void inv_rigid(const float* T, float* o) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o[4 * i + j] = T[4 * j + i];
    double s = 0.0;
    for (int k = 0; k < 3; ++k) s += (double)T[4 * k + i] * (double)T[4 * k + 3];
    o[4 * i + 3] = (float)(s * -1.0);
  }
  o[12] = o[13] = o[14] = 0; o[15] = 1;
}

// C = A * B, row-major 4x4 (C aliases neither)
inline void mul44(const float* A, const float* B, float* C) {
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { float a = 0.f; for (int k = 0; k < 4; ++k) a += A[4 * i + k] * B[4 * k + j]; C[4 * i + j] = a; }
}

// The inliers of a motion model MM (GetInitModelCam / GetInitModelObj, src/Tracking.cc:1690-1712, 1767-1800): point q of the list (ids[q], or q itself
// without a list) projects within 0.4 px of its observation (cx, cy).  flags[q] = 1 / 0 by list position; returns the count.
inline int count_mm_inliers(const float* MM, const float* K4, int n, const int32_t* ids, const float* xyz, const float* cx, const float* cy, uint8_t* flags) {
  int mm = 0;
  for (int q = 0; q < n; ++q) {
    const int id = ids ? ids[q] : q;
    const float x = xyz[3 * id], y = xyz[3 * id + 1], z = xyz[3 * id + 2];
    const float xc = MM[0] * x + MM[1] * y + MM[2] * z + MM[3], yc = MM[4] * x + MM[5] * y + MM[6] * z + MM[7], invz = 1.0f / (MM[8] * x + MM[9] * y + MM[10] * z + MM[11]);
    const float u_ = cx[id] - (K4[0] * xc * invz + K4[2]), v_ = cy[id] - (K4[1] * yc * invz + K4[3]);
    flags[q] = std::sqrt(u_ * u_ + v_ * v_) < 0.4f ? 1 : 0;
    mm += flags[q];
  }
  return mm;
}

// float key + DOUBLE refined flow, rounded once on the assignment (`pt.x = pLastFrame->mvStatKeys[..].pt.x + flow_new(0)`, src/Optimizer.cc:2529-2530, 2949-2950)
inline float key_plus_flow(float key, double flow) { return (float)((double)key + flow); }

}  // namespace VDO_SLAM::frame_math
