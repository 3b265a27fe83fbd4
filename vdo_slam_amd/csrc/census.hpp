// The 9 x 7 census transform shared by the stereo matcher (stereo.hip) and the dense optical-flow matcher (optflow.hip): step 1 of the stereo
// section of include/vdo_slam_hip.h.  62 bits in a uint64, bit k = the k-th window offset in raster order (dy = -3 .. 3 outer, dx = -4 .. 4 inner,
// the centre skipped) is darker than the centre; borders clamped.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vdo {

constexpr int kCensusTX = 32, kCensusTY = 8;            // pixels per census workgroup (256 threads)

// One 32 x 8 tile at (x0, y0) of a W x H image with rows `stride` bytes apart, from an LDS tile with a 4 / 3 pixel halo (40 x 14 bytes); out is the
// packed [H][W] census image.  Called by all 256 threads of the workgroup (it holds a barrier).
__device__ __forceinline__ void census_tile(const uint8_t* __restrict__ img, int64_t stride, int W, int H, int x0, int y0, uint64_t* __restrict__ out) {
  __shared__ uint8_t tile[kCensusTY + 6][kCensusTX + 8];
  for (int i = threadIdx.x; i < (kCensusTY + 6) * (kCensusTX + 8); i += 256) {
    const int r = i / (kCensusTX + 8), c = i % (kCensusTX + 8);
    const int gx = min(max(x0 + c - 4, 0), W - 1), gy = min(max(y0 + r - 3, 0), H - 1);
    tile[r][c] = img[(int64_t)gy * stride + gx];
  }
  __syncthreads();
  const int tx = threadIdx.x % kCensusTX, ty = threadIdx.x / kCensusTX;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= W || y >= H) return;
  const uint8_t centre = tile[ty + 3][tx + 4];
  uint64_t bits = 0;
  int k = 0;
#pragma unroll
  for (int dy = 0; dy < 7; ++dy)
#pragma unroll
    for (int dx = 0; dx < 9; ++dx) {
      if (dy == 3 && dx == 4) continue;
      bits |= (uint64_t)(tile[ty + dy][tx + dx] < centre) << k;
      ++k;
    }
  out[(size_t)y * W + x] = bits;
}

}  // namespace vdo
