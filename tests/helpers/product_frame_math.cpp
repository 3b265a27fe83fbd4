// Test helper: the PRODUCT's per-frame float arithmetic (vdo_slam_amd/host/frame_math.h, plain C++) behind C entry points, so that
// tests/test_frame_math.py can compare it bit for bit with a numpy float32 restatement on the CPU, without a GPU.
#include "../../vdo_slam_amd/host/frame_math.h"

namespace fm = VDO_SLAM::frame_math;

extern "C" {
void product_fm_identity(float* out16) { for (int i = 0; i < 16; ++i) out16[i] = fm::kI4[i]; }
void product_fm_inv_rigid(const float* T, float* out16) { fm::inv_rigid(T, out16); }
void product_fm_mul44(const float* A, const float* B, float* C) { fm::mul44(A, B, C); }
int product_fm_count_mm_inliers(const float* MM, const float* K4, int n, const int32_t* ids, const float* xyz, const float* cx, const float* cy, uint8_t* flags) {
  return fm::count_mm_inliers(MM, K4, n, ids, xyz, cx, cy, flags);
}
void product_fm_key_plus_flow(int n, const float* key, const double* flow, float* out) { for (int i = 0; i < n; ++i) out[i] = fm::key_plus_flow(key[i], flow[i]); }
}
