// Times one descriptor match (vdo_orb_match, csrc/orb_match.hip) on seeded sets: hipEvents on the context's stream around the call, warm-up,
// median over the runs; gated (window 16, octave difference 1, max distance 100, cross-check) and ungated, device-resident sets and host sets.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/orb_match_timing.hip -Iinclude -Lvdo_slam_amd -lvdo_hip -Wl,-rpath,'$ORIGIN/../vdo_slam_amd' -o tools/orb_match_timing
//   tools/orb_match_timing [rows=2500] [runs=30]
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
  const int n = argc > 1 ? std::atoi(argv[1]) : 2500, runs = argc > 2 ? std::atoi(argv[2]) : 30, warm = 5;
  if (n < 1 || runs < 1) { std::fprintf(stderr, "usage: orb_match_timing [rows] [runs]\n"); return 2; }
  std::mt19937 rng(7);
  // KITTI-like query set: positions over 1242 x 375, 8 octaves, random 256-bit rows
  struct Host { std::vector<uint8_t> desc; std::vector<float> x, y; std::vector<int32_t> oct; } h[2];
  for (Host& s : h) { s.desc.resize(32 * (size_t)n); s.x.resize(n); s.y.resize(n); s.oct.resize(n); }
  for (auto& b : h[0].desc) b = (uint8_t)(rng() & 255);
  for (int i = 0; i < n; ++i) { h[0].x[i] = (float)(rng() % 124200) / 100.f; h[0].y[i] = (float)(rng() % 37500) / 100.f; h[0].oct[i] = (int32_t)(rng() % 8); }
  // the train set: the query set seen again - shuffled, moved by up to 8 px, 24 random bit flips per row - so that the gated match finds its partners
  std::vector<int> perm(n);
  for (int i = 0; i < n; ++i) perm[i] = i;
  std::shuffle(perm.begin(), perm.end(), rng);
  for (int i = 0; i < n; ++i) {
    const int j = perm[i];
    std::copy(h[0].desc.begin() + 32 * (size_t)j, h[0].desc.begin() + 32 * (size_t)(j + 1), h[1].desc.begin() + 32 * (size_t)i);
    for (int k = 0; k < 24; ++k) { const unsigned bit = rng() & 255; h[1].desc[32 * (size_t)i + bit / 8] ^= (uint8_t)(1u << (bit & 7)); }
    h[1].x[i] = h[0].x[j] + (float)((int)(rng() % 1601) - 800) / 100.f; h[1].y[i] = h[0].y[j] + (float)((int)(rng() % 1601) - 800) / 100.f; h[1].oct[i] = h[0].oct[j];
  }
  hipStream_t stream;
  CK(hipStreamCreate(&stream));
  vdo_ctx* ctx = nullptr;
  if (vdo_ctx_create(0, stream, &ctx) != VDO_OK) { std::fprintf(stderr, "vdo_ctx_create: %s\n", vdo_last_error()); return 1; }
  vdo_match_set host[2], dev[2];
  for (int k = 0; k < 2; ++k) {
    host[k] = vdo_match_set{n, h[k].desc.data(), h[k].x.data(), h[k].y.data(), h[k].oct.data(), 0};
    uint8_t* d; float *x, *y; int32_t* o;
    CK(hipMalloc((void**)&d, 32 * (size_t)n)); CK(hipMalloc((void**)&x, 4 * (size_t)n)); CK(hipMalloc((void**)&y, 4 * (size_t)n)); CK(hipMalloc((void**)&o, 4 * (size_t)n));
    CK(hipMemcpy(d, h[k].desc.data(), 32 * (size_t)n, hipMemcpyHostToDevice)); CK(hipMemcpy(x, h[k].x.data(), 4 * (size_t)n, hipMemcpyHostToDevice));
    CK(hipMemcpy(y, h[k].y.data(), 4 * (size_t)n, hipMemcpyHostToDevice)); CK(hipMemcpy(o, h[k].oct.data(), 4 * (size_t)n, hipMemcpyHostToDevice));
    dev[k] = vdo_match_set{n, d, x, y, o, 1};
  }
  const vdo_match_params gated{100, 0.f, 16.f, 1, 1, 0}, plain{256, 0.f, -1.f, -1, 0, 0};
  std::vector<int32_t> idx(n), best(n), second(n);
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  struct Case { const char* name; const vdo_match_set* s; const vdo_match_params* p; };
  const Case cases[] = {{"gated + cross-check, device sets", dev, &gated}, {"ungated, device sets", dev, &plain},
                        {"gated + cross-check, host sets", host, &gated}, {"ungated, host sets", host, &plain}};
  for (const Case& c : cases) {
    std::vector<float> ev; std::vector<double> wall;
    int32_t m = 0;
    for (int r = 0; r < warm + runs; ++r) {
      CK(hipEventRecord(e0, stream));
      const auto t0 = std::chrono::steady_clock::now();
      if (vdo_orb_match(ctx, &c.s[0], &c.s[1], c.p, idx.data(), best.data(), second.data(), &m) != VDO_OK) { std::fprintf(stderr, "vdo_orb_match: %s\n", vdo_last_error()); return 1; }
      const auto t1 = std::chrono::steady_clock::now();
      CK(hipEventRecord(e1, stream)); CK(hipEventSynchronize(e1));
      float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= warm) { ev.push_back(ms); wall.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); }
    }
    std::sort(ev.begin(), ev.end()); std::sort(wall.begin(), wall.end());
    std::printf("%d x %d  %-34s matches %5d  stream (hipEvents) median %.3f ms  min %.3f  max %.3f | host call median %.3f ms  (%d runs after %d)\n", n, n, c.name, m,
                ev[ev.size() / 2], ev.front(), ev.back(), wall[wall.size() / 2], runs, warm);
  }
  vdo_ctx_destroy(ctx);
  return 0;
}
