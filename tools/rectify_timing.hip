// Times the stereo rectifier (vdo_rectify_compute / vdo_rectify_gate, csrc/rectify.hip) on device-resident sources and destinations: hipEvents on the
// context's stream around the call, warm-up, median over the runs.  The camera is a KITTI-sized one with a barrel distortion and a small rotation,
// the rectified view a little wider than the raw one (an invalid frame exists, so the gate has something to clear).  Cases: three grey jobs (left,
// right, next-left), three RGB jobs, three RGB jobs plus one nearest job (the class image), the gate.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/rectify_timing.hip -Iinclude -Lvdo_slam_amd -lvdo_hip -Wl,-rpath,'$ORIGIN/../vdo_slam_amd' -o tools/rectify_timing
//   tools/rectify_timing [width=1242] [height=375] [runs=30]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
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
  if (W < 1 || H < 1 || runs < 1) { std::fprintf(stderr, "usage: rectify_timing [width] [height] [runs]\n"); return 2; }
  const size_t n = (size_t)W * H;
  vdo_rectify_params p{};
  p.n_cams = 2; p.width = W; p.height = H;
  const double f = 0.58 * W;
  p.P[0] = 0.97 * f; p.P[1] = 0.97 * f; p.P[2] = 0.5 * (W - 1); p.P[3] = 0.5 * (H - 1);
  for (int c = 0; c < 2; ++c) {
    vdo_rectify_camera& q = p.cam[c];
    q.K[0] = f; q.K[1] = f; q.K[2] = 0.5 * (W - 1) + 2.5; q.K[3] = 0.5 * (H - 1) - 1.5;
    q.D[0] = -0.28; q.D[1] = 0.07; q.D[2] = 2e-4; q.D[3] = 2e-5; q.D[4] = 0;
    const double a = c ? -0.004 : 0.006;                            // a small rotation about y
    const double R[9] = {std::cos(a), 0, std::sin(a), 0, 1, 0, -std::sin(a), 0, std::cos(a)};
    for (int k = 0; k < 9; ++k) q.R[k] = R[k];
    q.src_width = W; q.src_height = H;
  }
  hipStream_t stream;
  CK(hipStreamCreate(&stream));
  vdo_ctx* ctx = nullptr;
  if (vdo_ctx_create(0, stream, &ctx) != VDO_OK) { std::fprintf(stderr, "vdo_ctx_create: %s\n", vdo_last_error()); return 1; }
  vdo_rectify* h = nullptr;
  if (vdo_rectify_create(ctx, &p, &h) != VDO_OK) { std::fprintf(stderr, "vdo_rectify_create: %s\n", vdo_last_error()); return 1; }
  int32_t n_valid[2] = {0, 0};
  vdo_rectify_get_valid(h, 0, nullptr, &n_valid[0]); vdo_rectify_get_valid(h, 1, nullptr, &n_valid[1]);
  std::mt19937 rng(7);
  std::vector<uint8_t> host(n * 3);
  uint8_t *d_src[4], *d_dst[4]; float* d_disp;
  for (int k = 0; k < 4; ++k) {
    for (auto& b : host) b = (uint8_t)(rng() & 255u);
    CK(hipMalloc((void**)&d_src[k], n * 3)); CK(hipMalloc((void**)&d_dst[k], n));
    CK(hipMemcpy(d_src[k], host.data(), n * 3, hipMemcpyHostToDevice));
  }
  CK(hipMalloc((void**)&d_disp, n * sizeof(float)));
  std::vector<float> disp(n, 256.f * 20.f);
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  struct Case { const char* name; int n_jobs, channels; bool gate; };
  const Case cases[] = {{"3 grey jobs (left, right, next-left)", 3, 1, false}, {"3 RGB jobs", 3, 3, false}, {"3 RGB jobs + 1 nearest job", 4, 3, false}, {"gate", 0, 0, true}};
  std::printf("%d x %d, valid pixels %d (left) %d (right) of %zu\n", W, H, n_valid[0], n_valid[1], n);
  for (const Case& c : cases) {
    vdo_rectify_job jobs[4];
    for (int k = 0; k < c.n_jobs; ++k) {
      const bool nearest = k == 3;
      const int ch = nearest ? 1 : c.channels;
      jobs[k] = vdo_rectify_job{d_src[k], (int64_t)W * ch, ch, 1, k == 1 ? 1 : 0, nearest ? 1 : 0, d_dst[k], W};
    }
    std::vector<float> ev; std::vector<double> wall;
    int32_t n_cleared = 0;
    for (int r = 0; r < warm + runs; ++r) {
      if (c.gate) CK(hipMemcpy(d_disp, disp.data(), n * sizeof(float), hipMemcpyHostToDevice));       // the gate works in place
      CK(hipEventRecord(e0, stream));
      const auto t0 = std::chrono::steady_clock::now();
      const int rc = c.gate ? vdo_rectify_gate(h, 0, d_disp, W, 1, &n_cleared) : vdo_rectify_compute(h, jobs, c.n_jobs, 1, 1, 0);
      if (rc != VDO_OK) { std::fprintf(stderr, "rectify: %s\n", vdo_last_error()); return 1; }
      const auto t1 = std::chrono::steady_clock::now();
      CK(hipEventRecord(e1, stream)); CK(hipEventSynchronize(e1));
      float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= warm) { ev.push_back(ms); wall.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); }
    }
    std::sort(ev.begin(), ev.end()); std::sort(wall.begin(), wall.end());
    double ms2[2] = {0, 0};
    vdo_rectify_last_timing(h, ms2);
    if (c.gate) std::printf("%-38s cleared %7d ", c.name, n_cleared); else std::printf("%-38s                 ", c.name);
    std::printf(" stream (hipEvents) median %.3f ms  min %.3f  max %.3f | host call median %.3f ms | kernel alone (last call) %.3f ms  (%d runs after %d)\n", ev[ev.size() / 2],
                ev.front(), ev.back(), wall[wall.size() / 2], ms2[1], runs, warm);
  }
  vdo_rectify_destroy(h);
  vdo_ctx_destroy(ctx);
  return 0;
}
