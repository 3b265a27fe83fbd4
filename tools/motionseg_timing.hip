// Times the motion segmenter (vdo_motionseg_compute and vdo_motionseg_egomotion, csrc/motionseg.hip) on device-resident images: hipEvents on the
// context's stream around the call, warm-up, median over the runs.  The scene: a road-like disparity ramp seen by a camera that drives forward, the
// flow and the next disparity that motion gives (computed here in double), three rectangles that move on their own, 2 % of the pixels without
// disparity and a validity image with 5 % zeros.
// Per-kernel times come from the same program under rocprofv3 --kernel-trace --stats, in a run of its own.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/motionseg_timing.hip -Iinclude -Lvdo_slam_amd -lvdo_hip -Wl,-rpath,'$ORIGIN/../vdo_slam_amd' -o tools/motionseg_timing
//   tools/motionseg_timing [width=1242] [height=375] [runs=30]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "vdo_slam_hip.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
  const int W = argc > 1 ? std::atoi(argv[1]) : 1242, H = argc > 2 ? std::atoi(argv[2]) : 375;
  const int runs = argc > 3 ? std::atoi(argv[3]) : 30, warm = 5;
  if (W < 1 || H < 1 || runs < 1) { std::fprintf(stderr, "usage: motionseg_timing [width] [height] [runs]\n"); return 2; }
  const size_t n = (size_t)W * H;
  const double fx = 721.5377 * W / 1242.0, fy = 721.5377 * H / 375.0, cx = 0.49 * W, cy = 0.46 * H, bf = 387.5744 * W / 1242.0, unit = 256.0, tz = -0.8;
  std::mt19937 rng(7);
  std::vector<float> disp0(n), disp1(n, 0.f), flow(2 * n);
  std::vector<uint8_t> valid(n);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t i = (size_t)y * W + x;
      double d = 3.0 + 60.0 * y / H;                                  // px
      double mx = 0, mz = 0;                                          // the pixel's own motion [m]
      for (int k = 0; k < 3; ++k) {
        const int x0 = (1 + 2 * k) * W / 7, y0 = H / 3 + k * H / 12;
        if (x >= x0 && x < x0 + W / 10 && y >= y0 && y < y0 + H / 5) { d = 20.0 + 8.0 * k; mx = 0.05 * (k - 1); mz = 0.4 + 0.1 * k; }
      }
      const double Z = bf / d, X = (x - cx) * Z / fx, Y = (y - cy) * Z / fy, Zn = Z + tz + mz, Xn = X + mx;
      flow[2 * i] = (float)(fx * Xn / Zn + cx - x); flow[2 * i + 1] = (float)(fy * Y / Zn + cy - y);
      disp0[i] = rng() % 100u < 2u ? 0.f : (float)(d * unit);
      valid[i] = rng() % 100u < 5u ? 0 : 1;
      const long xt = std::lround(x + flow[2 * i]), yt = std::lround(y + flow[2 * i + 1]);
      if (xt >= 0 && xt < W && yt >= 0 && yt < H) disp1[(size_t)yt * W + xt] = (float)(bf / Zn * unit);
    }
  hipStream_t stream;
  CK(hipStreamCreate(&stream));
  vdo_ctx* ctx = nullptr;
  if (vdo_ctx_create(0, stream, &ctx) != VDO_OK) { std::fprintf(stderr, "vdo_ctx_create: %s\n", vdo_last_error()); return 1; }
  const vdo_motionseg_params p{{(float)fx, (float)fy, (float)cx, (float)cy}, (float)bf, (float)unit, 0.5f, 0.5f, 9.f, (float)(bf / 40.0), 2, 1, 2, 6, 1};
  vdo_motionseg* h = nullptr;
  if (vdo_motionseg_create(ctx, W, H, &p, &h) != VDO_OK) { std::fprintf(stderr, "vdo_motionseg_create: %s\n", vdo_last_error()); return 1; }
  float *d_disp0, *d_disp1, *d_flow; uint8_t *d_valid, *d_cls;
  CK(hipMalloc((void**)&d_disp0, n * sizeof(float))); CK(hipMalloc((void**)&d_disp1, n * sizeof(float))); CK(hipMalloc((void**)&d_flow, 2 * n * sizeof(float)));
  CK(hipMalloc((void**)&d_valid, n)); CK(hipMalloc((void**)&d_cls, n));
  CK(hipMemcpy(d_disp0, disp0.data(), n * sizeof(float), hipMemcpyHostToDevice)); CK(hipMemcpy(d_disp1, disp1.data(), n * sizeof(float), hipMemcpyHostToDevice));
  CK(hipMemcpy(d_flow, flow.data(), 2 * n * sizeof(float), hipMemcpyHostToDevice)); CK(hipMemcpy(d_valid, valid.data(), n, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  float T[16];
  int32_t ego[3] = {0, 0, 0}, out[3] = {0, 0, 0};
  for (int which = 0; which < 2; ++which) {                            // the ego-motion first: the compute takes its T
    std::vector<float> ev; std::vector<double> wall, own;
    for (int r = 0; r < warm + runs; ++r) {
      CK(hipEventRecord(e0, stream));
      const auto t0 = std::chrono::steady_clock::now();
      const int rc = which == 0 ? vdo_motionseg_egomotion(h, d_disp0, W, d_flow, 2 * (int64_t)W, d_valid, W, 1, 16, 500, 1.0, 0.98, 50, T, ego)
                                : vdo_motionseg_compute(h, d_disp0, W, d_disp1, W, d_flow, 2 * (int64_t)W, d_valid, W, 1, T, d_cls, 1, out);
      if (rc != VDO_OK) { std::fprintf(stderr, "motionseg: %s\n", vdo_last_error()); return 1; }
      const auto t1 = std::chrono::steady_clock::now();
      CK(hipEventRecord(e1, stream)); CK(hipEventSynchronize(e1));
      float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
      double m2[2]; vdo_motionseg_last_timing(h, m2);
      if (r >= warm) { ev.push_back(ms); wall.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); own.push_back(m2[1]); }
    }
    std::sort(ev.begin(), ev.end()); std::sort(wall.begin(), wall.end()); std::sort(own.begin(), own.end());
    if (which == 0) std::printf("%d x %d  vdo_motionseg_egomotion step 16   samples %6d  inliers %6d  iterations %3d  tz %.4f (true %.4f) ", W, H, ego[0], ego[1], ego[2], T[11], tz);
    else std::printf("%d x %d  vdo_motionseg_compute             moving %7d  static %7d  unknown %7d              ", W, H, out[0], out[1], out[2]);
    std::printf(" stream (hipEvents) median %.3f ms  min %.3f  max %.3f | host call median %.3f ms | kernels alone (handle's events) median %.3f ms  (%d runs after %d)\n",
                ev[ev.size() / 2], ev.front(), ev.back(), wall[wall.size() / 2], own[own.size() / 2], runs, warm);
  }
  vdo_motionseg_destroy(h);
  vdo_ctx_destroy(ctx);
  return 0;
}
