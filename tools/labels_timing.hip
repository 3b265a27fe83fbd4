// Times the instance labeller (vdo_labels_compute, csrc/labels.hip) and its speckle filter on device-resident images: hipEvents on the context's
// stream around the call, warm-up, median over the runs.  Two class images: a scene of a dozen rectangles of three classes over a disparity
// ramp (what a semantic map of a street looks like to the labeller, the gate on), and noise of density 0.59 - the site-percolation threshold of the
// square lattice, where the components are as ragged and as many-tiled as they get - at both connectivities.
// Per-kernel times come from the same program under rocprofv3 --kernel-trace --stats, in a run of its own.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/labels_timing.hip -Iinclude -Lvdo_slam_amd -lvdo_hip -Wl,-rpath,'$ORIGIN/../vdo_slam_amd' -o tools/labels_timing
//   tools/labels_timing [width=1242] [height=375] [runs=30]
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
  if (W < 1 || H < 1 || runs < 1) { std::fprintf(stderr, "usage: labels_timing [width] [height] [runs]\n"); return 2; }
  const size_t n = (size_t)W * H;
  std::mt19937 rng(7);
  // scene: a ramp of disparities (in 1/256 px) that grows downwards like a road, twelve rectangles of classes 1..3 at their own constant disparity; two
  // pairs of them touch, one pair at disparities the gate joins and one it cuts
  std::vector<uint8_t> scene(n, 0), noise(n);
  std::vector<float> disp(n);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) disp[(size_t)y * W + x] = 256.f * (4.f + 60.f * y / H);
  for (int k = 0; k < 12; ++k) {
    const int w = W / 16 + (int)(rng() % (unsigned)(W / 12 + 1)), h = H / 8 + (int)(rng() % (unsigned)(H / 4 + 1));
    const int x0 = (k % 6) * (W / 6) + (k == 3 || k == 9 ? -(W / 40) : W / 60), y0 = (k / 6) * (H / 2) + H / 16;
    const float d = 256.f * (10.f + 4.f * k) + (k == 3 ? 300.f : 0.f);
    for (int y = std::max(0, y0); y < std::min(H, y0 + h); ++y)
      for (int x = std::max(0, x0); x < std::min(W, x0 + w); ++x) { scene[(size_t)y * W + x] = (uint8_t)(1 + k % 3); disp[(size_t)y * W + x] = d; }
  }
  for (auto& b : noise) b = (rng() % 100000u) < 59000u ? 1 : 0;
  std::vector<float> speckled = disp;                               // the ramp with 2 % of the pixels off by 40 px, single or in small clumps
  for (size_t i = 0; i + 1 < n; ++i) if (rng() % 100u < 2u) { speckled[i] += 256.f * 40.f; if (rng() & 1u) speckled[i + 1] = speckled[i]; }
  hipStream_t stream;
  CK(hipStreamCreate(&stream));
  vdo_ctx* ctx = nullptr;
  if (vdo_ctx_create(0, stream, &ctx) != VDO_OK) { std::fprintf(stderr, "vdo_ctx_create: %s\n", vdo_last_error()); return 1; }
  uint8_t* d_cls; float *d_disp, *d_work; int32_t* d_mask;
  CK(hipMalloc((void**)&d_cls, n)); CK(hipMalloc((void**)&d_disp, n * sizeof(float))); CK(hipMalloc((void**)&d_work, n * sizeof(float))); CK(hipMalloc((void**)&d_mask, n * sizeof(int32_t)));
  CK(hipMemcpy(d_disp, disp.data(), n * sizeof(float), hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  struct Case { const char* name; const std::vector<uint8_t>* cls; vdo_labels_params p; bool speckle; };
  const Case cases[] = {{"rectangles over a ramp, defaults (8, gate 512, min 200)", &scene, {8, 512, 200, 1023}, false},
                        {"noise 0.59, connectivity 4, no gate, min_area 1", &noise, {4, -1, 1, 1023}, false},
                        {"noise 0.59, connectivity 8, no gate, min_area 1", &noise, {8, -1, 1, 1023}, false},
                        {"speckle filter, ramp + 2 % outliers (256, 100)", nullptr, {8, -1, 1, 1023}, true}};
  for (const Case& c : cases) {
    vdo_labels* h = nullptr;
    if (vdo_labels_create(ctx, W, H, &c.p, &h) != VDO_OK) { std::fprintf(stderr, "vdo_labels_create: %s\n", vdo_last_error()); return 1; }
    if (c.cls) CK(hipMemcpy(d_cls, c.cls->data(), n, hipMemcpyHostToDevice));
    std::vector<float> ev; std::vector<double> wall;
    int32_t out[3] = {0, 0, 0}, n_removed = 0;
    for (int r = 0; r < warm + runs; ++r) {
      if (c.speckle) CK(hipMemcpy(d_work, speckled.data(), n * sizeof(float), hipMemcpyHostToDevice));       // the filter works in place
      CK(hipEventRecord(e0, stream));
      const auto t0 = std::chrono::steady_clock::now();
      const int rc = c.speckle ? vdo_labels_filter_speckles(h, d_work, 1, 256, 100, &n_removed) : vdo_labels_compute(h, d_cls, W, d_disp, W, 1, d_mask, 1, out);
      if (rc != VDO_OK) { std::fprintf(stderr, "labels: %s\n", vdo_last_error()); return 1; }
      const auto t1 = std::chrono::steady_clock::now();
      CK(hipEventRecord(e1, stream)); CK(hipEventSynchronize(e1));
      float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= warm) { ev.push_back(ms); wall.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); }
    }
    std::sort(ev.begin(), ev.end()); std::sort(wall.begin(), wall.end());
    if (c.speckle) std::printf("%d x %d  %-58s removed %7d                               ", W, H, c.name, n_removed);
    else std::printf("%d x %d  %-58s labels %5d  components %6d  threshold %5d ", W, H, c.name, out[0], out[1], out[2]);
    std::printf(" stream (hipEvents) median %.3f ms  min %.3f  max %.3f | host call median %.3f ms  (%d runs after %d)\n", ev[ev.size() / 2], ev.front(), ev.back(),
                wall[wall.size() / 2], runs, warm);
    vdo_labels_destroy(h);
  }
  vdo_ctx_destroy(ctx);
  return 0;
}
