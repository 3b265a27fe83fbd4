// Times one dense optical-flow match (vdo_optflow_compute, csrc/optflow.hip) on a seeded textured pair whose second image is the first moved by a
// displacement that grows across the image, with a box moving on its own: hipEvents on the context's stream around the call, warm-up, median over
// the runs; the default parameters with the backward pass (forward-backward check) and without it, device-resident images and device outputs.
// Per-kernel times come from the same program under rocprofv3 --kernel-trace --stats, in a run of its own.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/optflow_timing.hip -Iinclude -Lvdo_slam_amd -lvdo_hip -Wl,-rpath,'$ORIGIN/../vdo_slam_amd' -o tools/optflow_timing
//   tools/optflow_timing [width=1242] [height=375] [runs=30]
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
  const int W = argc > 1 ? std::atoi(argv[1]) : 1242, H = argc > 2 ? std::atoi(argv[2]) : 375;
  const int runs = argc > 3 ? std::atoi(argv[3]) : 30, warm = 5;
  if (W < 1 || H < 1 || runs < 1) { std::fprintf(stderr, "usage: optflow_timing [width] [height] [runs]\n"); return 2; }
  // im0: smoothed noise; im1: noise under im0 moved by (2 + 10 x / W, -3) - and by (-6, 4) inside a box
  std::mt19937 rng(7);
  std::vector<uint8_t> im0((size_t)W * H), im1((size_t)W * H);
  for (auto& b : im1) b = (uint8_t)(rng() & 255);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const unsigned v = rng() & 255;
      im0[(size_t)y * W + x] = (uint8_t)((v + (x ? im0[(size_t)y * W + x - 1] : v) + (y ? im0[(size_t)(y - 1) * W + x] : v)) / 3);
    }
  for (int pass = 0; pass < 2; ++pass)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const bool box = x >= W / 3 && x < W / 2 && y >= H / 4 && y < H / 2;
        if (box != (pass == 1)) continue;                         // the box is drawn last: it occludes
        const int xt = x + (box ? -6 : 2 + 10 * x / W), yt = y + (box ? 4 : -3);
        if (xt >= 0 && xt < W && yt >= 0 && yt < H) im1[(size_t)yt * W + xt] = im0[(size_t)y * W + x];
      }
  hipStream_t stream;
  CK(hipStreamCreate(&stream));
  vdo_ctx* ctx = nullptr;
  if (vdo_ctx_create(0, stream, &ctx) != VDO_OK) { std::fprintf(stderr, "vdo_ctx_create: %s\n", vdo_last_error()); return 1; }
  uint8_t *d0, *d1, *d_valid; float* d_flow;
  CK(hipMalloc((void**)&d0, im0.size())); CK(hipMalloc((void**)&d1, im1.size()));
  CK(hipMalloc((void**)&d_flow, im0.size() * 2 * sizeof(float))); CK(hipMalloc((void**)&d_valid, im0.size()));
  CK(hipMemcpy(d0, im0.data(), im0.size(), hipMemcpyHostToDevice)); CK(hipMemcpy(d1, im1.data(), im1.size(), hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  struct Case { const char* name; vdo_optflow_params p; };
  const Case cases[] = {{"defaults (6 levels, r 2, w 2, median, FB 1, sub-pixel)", {6, 2, 2, 1, 1, 1}}, {"no backward pass (FB -1)", {6, 2, 2, 1, -1, 1}}};
  for (const Case& c : cases) {
    vdo_optflow* h = nullptr;
    if (vdo_optflow_create(ctx, W, H, &c.p, &h) != VDO_OK) { std::fprintf(stderr, "vdo_optflow_create: %s\n", vdo_last_error()); return 1; }
    std::vector<float> ev; std::vector<double> wall;
    int32_t n_valid = 0;
    for (int r = 0; r < warm + runs; ++r) {
      CK(hipEventRecord(e0, stream));
      const auto t0 = std::chrono::steady_clock::now();
      if (vdo_optflow_compute(h, d0, W, d1, W, 1, d_flow, d_valid, 1, &n_valid) != VDO_OK) { std::fprintf(stderr, "vdo_optflow_compute: %s\n", vdo_last_error()); return 1; }
      const auto t1 = std::chrono::steady_clock::now();
      CK(hipEventRecord(e1, stream)); CK(hipEventSynchronize(e1));
      float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= warm) { ev.push_back(ms); wall.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); }
    }
    std::sort(ev.begin(), ev.end()); std::sort(wall.begin(), wall.end());
    // what the search computes: per pixel of every level and direction (2r+1)^2 (2w+1)^2 XOR + popcounts of 64-bit words
    double pix = 0; int w = W, hh = H;
    for (int l = 0; l < c.p.levels; ++l) { pix += (double)w * hh; w = (w + 1) / 2; hh = (hh + 1) / 2; }
    const int nc = (2 * c.p.radius + 1) * (2 * c.p.radius + 1), nw = (2 * c.p.window + 1) * (2 * c.p.window + 1);
    const double pops = pix * (c.p.fb_max_diff >= 0 ? 2 : 1) * nc * nw;
    std::printf("%d x %d  %-56s valid %7d  stream (hipEvents) median %.3f ms  min %.3f  max %.3f | host call median %.3f ms  (%d runs after %d) | %.1f M 64-bit popcounts\n",
                W, H, c.name, n_valid, ev[ev.size() / 2], ev.front(), ev.back(), wall[wall.size() / 2], runs, warm, pops / 1e6);
    vdo_optflow_destroy(h);
  }
  vdo_ctx_destroy(ctx);
  return 0;
}
