// Times the dense mapper (vdo_dense_integrate, vdo_dense_recenter and vdo_dense_extract, csrc/dense.hip) on device-resident images: hipEvents on the
// context's stream around the call, warm-up, median over the runs - and, as the yardstick, a device-to-device copy of the same volume in the same
// program.  The scene: a road-like depth ramp with a wall across it seen by a camera inside the volume, 2 % of the pixels without depth and three
// masked rectangles.  Two volumes: 512 x 128 x 512 (128 MiB, larger than the Infinity Cache together with its copy) and 128 x 64 x 128 (4 MiB).
// Per-kernel times come from the same program under rocprofv3 --kernel-trace --stats, in a run of its own.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/dense_timing.hip -Iinclude -Lvdo_slam_amd -lvdo_hip -Wl,-rpath,'$ORIGIN/../vdo_slam_amd' -o tools/dense_timing
//   tools/dense_timing [width=1242] [height=375] [runs=30] [voxels_per_thread=4]
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

static double median(std::vector<double>& v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char** argv) {
  const int W = argc > 1 ? std::atoi(argv[1]) : 1242, H = argc > 2 ? std::atoi(argv[2]) : 375;
  const int runs = argc > 3 ? std::atoi(argv[3]) : 30, vpt = argc > 4 ? std::atoi(argv[4]) : 4, warm = 5;
  if (W < 1 || H < 1 || runs < 1) { std::fprintf(stderr, "usage: dense_timing [width] [height] [runs] [voxels_per_thread]\n"); return 2; }
  const size_t npix = (size_t)W * H;
  const double fx = 721.5377 * W / 1242.0, fy = 721.5377 * H / 375.0, cx = 0.49 * W, cy = 0.46 * H;
  std::mt19937 rng(7);
  std::vector<float> depth(npix);
  std::vector<int32_t> mask(npix, 0);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t i = (size_t)y * W + x;
      double d = y > cy + 2 ? std::min(25.0, 1.65 * fy / (y - cy)) : 25.0;      // the ground 1.65 m below the camera, a wall 25 m ahead
      for (int k = 0; k < 3; ++k) {
        const int x0 = (1 + 2 * k) * W / 7, y0 = H / 3 + k * H / 12;
        if (x >= x0 && x < x0 + W / 10 && y >= y0 && y < y0 + H / 5) { d = 8.0 + 4.0 * k; mask[i] = k + 1; }
      }
      depth[i] = rng() % 100u < 2u ? 0.f : (float)d;
    }
  hipStream_t stream;
  CK(hipStreamCreate(&stream));
  vdo_ctx* ctx = nullptr;
  if (vdo_ctx_create(0, stream, &ctx) != VDO_OK) { std::fprintf(stderr, "vdo_ctx_create: %s\n", vdo_last_error()); return 1; }
  float* d_depth; int32_t* d_mask;
  CK(hipMalloc((void**)&d_depth, npix * sizeof(float))); CK(hipMalloc((void**)&d_mask, npix * sizeof(int32_t)));
  CK(hipMemcpy(d_depth, depth.data(), npix * sizeof(float), hipMemcpyHostToDevice)); CK(hipMemcpy(d_mask, mask.data(), npix * sizeof(int32_t), hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int sizes[2][3] = {{512, 128, 512}, {128, 64, 128}};
  for (int v = 0; v < 2; ++v) {
    const int* n = sizes[v];
    const float voxel = v == 0 ? 0.1f : 0.4f;                                  // both volumes 51.2 x 12.8 x 51.2 m ... 51.2 x 25.6 x 51.2 m around the camera
    const size_t nvox = (size_t)n[0] * n[1] * n[2];
    // the camera at the anchor (0.5, 0.5, 0.25) of a volume whose origin is (-n/2, -n/2, -n/4)
    const vdo_dense_params p{{n[0], n[1], n[2]}, voxel, {-n[0] / 2, -n[1] / 2, -n[2] / 4}, {(float)fx, (float)fy, (float)cx, (float)cy}, 4.f * voxel, 0.f, 40.f, 64, 1 << 20};
    vdo_dense* h = nullptr;
    if (vdo_dense_create(ctx, W, H, &p, &h) != VDO_OK) { std::fprintf(stderr, "vdo_dense_create: %s\n", vdo_last_error()); return 1; }
    if (vdo_dense_set_voxels_per_thread(h, vpt) != VDO_OK) { std::fprintf(stderr, "%s\n", vdo_last_error()); return 1; }
    uint32_t *d_vol = nullptr, *d_copy = nullptr;
    vdo_dense_device_volume(h, &d_vol);
    CK(hipMalloc((void**)&d_copy, nvox * sizeof(uint32_t)));
    float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    T[3] = 0.013f; T[7] = -0.007f; T[11] = 0.021f;
    int64_t out[3] = {0, 0, 0}, count = 0;
    const int32_t lo[3] = {p.origin[0], p.origin[1], p.origin[2]}, hi[3] = {p.origin[0] + n[0], p.origin[1] + n[1], p.origin[2] + n[2]};
    std::printf("volume %d x %d x %d (%.0f MiB), voxel %.2f m, image %d x %d, %d voxels per thread\n", n[0], n[1], n[2], nvox * 4.0 / (1 << 20), voxel, W, H, vpt);
    double t_copy = 0;
    for (int which = 0; which < 5; ++which) {                                   // copy, integrate (first frames), integrate (steady state), recenter, extract
      std::vector<double> ev, own;
      int32_t o[3] = {p.origin[0], p.origin[1], p.origin[2]};
      for (int r = 0; r < warm + runs; ++r) {
        int rc = VDO_OK;
        if (which == 3) { o[2] += 1; }                                          // one z slab: nx * ny words
        CK(hipEventRecord(e0, stream));
        if (which == 0) CK(hipMemcpyAsync(d_copy, d_vol, nvox * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        else if (which == 1 || which == 2) rc = vdo_dense_integrate(h, d_depth, W, d_mask, W, 1, T, out);
        else if (which == 3) rc = vdo_dense_recenter(h, o);
        else rc = vdo_dense_extract(h, lo, hi, 2, 0, nullptr, nullptr, nullptr, 1, &count);
        if (rc != VDO_OK) { std::fprintf(stderr, "dense: %s\n", vdo_last_error()); return 1; }
        CK(hipEventRecord(e1, stream)); CK(hipEventSynchronize(e1));
        float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
        double m2[2] = {0, 0}; vdo_dense_last_timing(h, m2);
        if (r >= warm) { ev.push_back(ms); own.push_back(m2[1]); }
      }
      if (which == 3) { const int32_t back[3] = {p.origin[0], p.origin[1], p.origin[2]}; vdo_dense_recenter(h, back); for (int r = 0; r < 3; ++r) vdo_dense_integrate(h, d_depth, W, d_mask, W, 1, T, out); }
      const double lo_ms = *std::min_element(ev.begin(), ev.end()), hi_ms = *std::max_element(ev.begin(), ev.end()), med = median(ev), med_own = median(own);
      static const char* const names[5] = {"hipMemcpyAsync device to device of the volume", "vdo_dense_integrate, frames 6..35 (weights still growing)", "vdo_dense_integrate, frames 41..70",
                                           "vdo_dense_recenter by one z slab", "vdo_dense_extract, whole volume, count only"};
      std::printf("  %-58s stream (hipEvents) median %.3f ms  min %.3f  max %.3f", names[which], med, lo_ms, hi_ms);
      if (which == 0) { t_copy = med; std::printf("  | %.2f TB/s read + written", 2.0 * nvox * 4 / (med * 1e-3) / 1e12); }
      else std::printf("  | kernel alone (handle's events) median %.3f ms", med_own);
      if (which == 1 || which == 2)
        std::printf("  | updated %lld masked %lld occluded %lld of %zu voxels | %.2f x the copy | volume bytes: read 4 B per voxel, written 4 B per updated voxel (whole 64 B lines): "
                    "%.2f TB/s on the kernel's time", (long long)out[0], (long long)out[1], (long long)out[2], nvox, med_own / t_copy, (nvox * 4.0 + out[0] * 4.0) / (med_own * 1e-3) / 1e12);
      if (which == 4) std::printf("  | %lld points", (long long)count);
      std::printf("  (%d runs after %d)\n", runs, warm);
    }
    CK(hipFree(d_copy));
    vdo_dense_destroy(h);
  }
  vdo_ctx_destroy(ctx);
  return 0;
}
