// Times one stereo match (vdo_stereo_compute, csrc/stereo.hip) on a seeded textured pair with a ramp of disparities: hipEvents on the context's
// stream around the call, warm-up, median over the runs; 8 paths with every filter and 4 paths without filters, device-resident images and a
// device output.  Also prints the traffic the aggregation's layout implies, for the bytes/s of its kernel time (rocprofv3 --kernel-trace --stats).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/stereo_timing.hip -Iinclude -Lvdo_slam_amd -lvdo_hip -Wl,-rpath,'$ORIGIN/../vdo_slam_amd' -o tools/stereo_timing
//   tools/stereo_timing [width=1242] [height=375] [max_disparity=128] [runs=30]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "vdo_slam_hip.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
  const int W = argc > 1 ? std::atoi(argv[1]) : 1242, H = argc > 2 ? std::atoi(argv[2]) : 375, D = argc > 3 ? std::atoi(argv[3]) : 128;
  const int runs = argc > 4 ? std::atoi(argv[4]) : 30, warm = 5;
  if (W < 1 || H < 1 || runs < 1) { std::fprintf(stderr, "usage: stereo_timing [width] [height] [max_disparity] [runs]\n"); return 2; }
  // left: smoothed noise; right: left shifted by a disparity that grows down the image from D/8 to D/2 (noise where nothing lands)
  std::mt19937 rng(7);
  std::vector<uint8_t> left((size_t)W * H), right((size_t)W * H);
  for (auto& b : right) b = (uint8_t)(rng() & 255);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const unsigned v = rng() & 255;
      left[(size_t)y * W + x] = (uint8_t)((v + (x ? left[(size_t)y * W + x - 1] : v) + (y ? left[(size_t)(y - 1) * W + x] : v)) / 3);
    }
  for (int y = 0; y < H; ++y) {
    const int d = D / 8 + (int)((long long)y * (D / 2 - D / 8) / H);
    for (int x = d; x < W; ++x) right[(size_t)y * W + x - d] = left[(size_t)y * W + x];
  }
  hipStream_t stream;
  CK(hipStreamCreate(&stream));
  vdo_ctx* ctx = nullptr;
  if (vdo_ctx_create(0, stream, &ctx) != VDO_OK) { std::fprintf(stderr, "vdo_ctx_create: %s\n", vdo_last_error()); return 1; }
  uint8_t *d_left, *d_right; float* d_out;
  CK(hipMalloc((void**)&d_left, left.size())); CK(hipMalloc((void**)&d_right, right.size())); CK(hipMalloc((void**)&d_out, left.size() * sizeof(float)));
  CK(hipMemcpy(d_left, left.data(), left.size(), hipMemcpyHostToDevice)); CK(hipMemcpy(d_right, right.data(), right.size(), hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  struct Case { const char* name; vdo_stereo_params p; };
  const Case cases[] = {{"8 paths, uniqueness 5, LR 1, sub-pixel", {D, 10, 120, 8, 5, 1, 1}}, {"4 paths, no filters", {D, 10, 120, 4, 0, -1, 0}}};
  for (const Case& c : cases) {
    vdo_stereo* h = nullptr;
    if (vdo_stereo_create(ctx, W, H, &c.p, &h) != VDO_OK) { std::fprintf(stderr, "vdo_stereo_create: %s\n", vdo_last_error()); return 1; }
    std::vector<float> ev; std::vector<double> wall;
    int32_t n_valid = 0;
    for (int r = 0; r < warm + runs; ++r) {
      CK(hipEventRecord(e0, stream));
      const auto t0 = std::chrono::steady_clock::now();
      if (vdo_stereo_compute(h, d_left, W, d_right, W, 1, d_out, 1, &n_valid) != VDO_OK) { std::fprintf(stderr, "vdo_stereo_compute: %s\n", vdo_last_error()); return 1; }
      const auto t1 = std::chrono::steady_clock::now();
      CK(hipEventRecord(e1, stream)); CK(hipEventSynchronize(e1));
      float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= warm) { ev.push_back(ms); wall.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); }
    }
    std::sort(ev.begin(), ev.end()); std::sort(wall.begin(), wall.end());
    // what the aggregation moves: per direction the cost volume read once (1 byte per entry) and one 32-bit atomic add per pair of entries (a
    // read-modify-write of 2 bytes per entry at the L2: 2 read + 2 written)
    const double vol = (double)W * H * D, agg_bytes = c.p.paths * vol * (1.0 + 2.0 + 2.0);
    std::printf("%d x %d x %d  %-40s valid %7d  stream (hipEvents) median %.3f ms  min %.3f  max %.3f | host call median %.3f ms  (%d runs after %d) | aggregation traffic %.1f MB\n",
                W, H, D, c.name, n_valid, ev[ev.size() / 2], ev.front(), ev.back(), wall[wall.size() / 2], runs, warm, agg_bytes / 1e6);
    vdo_stereo_destroy(h);
  }
  vdo_ctx_destroy(ctx);
  return 0;
}
