// Times the raycaster (vdo_raycast_render, csrc/raycast.hip) on a device-resident volume with device outputs: hipEvents on the context's stream around
// the call, warm-up, median over the runs - with the empty-space skipping on and off, the occupancy-grid build alone (the handle's events), and, as
// yardsticks in the same program, vdo_dense_integrate into the same volume and a device-to-device copy of it.  The scene: the ground 1.65 m below the
// camera and a wall 25 m ahead, rendered as a depth image and fused 4 times into a 512 x 128 x 512 volume of 0.1 m voxels (128 MiB) around the camera;
// the view is the fusing camera's (1242 x 375), then one turned by 20 degrees.  Samples every truncation / 2 = 0.2 m from 0.1 m to 40 m: 201 per ray.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/raycast_timing.hip -Iinclude -Lvdo_slam_amd -lvdo_hip -Wl,-rpath,'$ORIGIN/../vdo_slam_amd' -o tools/raycast_timing
//   tools/raycast_timing [width=1242] [height=375] [runs=30]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vdo_slam_hip.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static double median(std::vector<double>& v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char** argv) {
  const int W = argc > 1 ? std::atoi(argv[1]) : 1242, H = argc > 2 ? std::atoi(argv[2]) : 375, runs = argc > 3 ? std::atoi(argv[3]) : 30, warm = 5;
  if (W < 1 || H < 1 || runs < 1) { std::fprintf(stderr, "usage: raycast_timing [width] [height] [runs]\n"); return 2; }
  const size_t npix = (size_t)W * H;
  const double fx = 721.5377 * W / 1242.0, fy = 721.5377 * H / 375.0, cx = 0.49 * W, cy = 0.46 * H;
  std::vector<float> depth(npix);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) depth[(size_t)y * W + x] = (float)(y > cy + 2 ? std::min(25.0, 1.65 * fy / (y - cy)) : 25.0);      // the ground, then the wall
  hipStream_t stream;
  CK(hipStreamCreate(&stream));
  vdo_ctx* ctx = nullptr;
  if (vdo_ctx_create(0, stream, &ctx) != VDO_OK) { std::fprintf(stderr, "vdo_ctx_create: %s\n", vdo_last_error()); return 1; }
  float *d_depth, *d_out_depth, *d_out_grad; int32_t* d_out_wgt;
  CK(hipMalloc((void**)&d_depth, npix * sizeof(float))); CK(hipMalloc((void**)&d_out_depth, npix * sizeof(float)));
  CK(hipMalloc((void**)&d_out_grad, npix * 3 * sizeof(float))); CK(hipMalloc((void**)&d_out_wgt, npix * sizeof(int32_t)));
  CK(hipMemcpy(d_depth, depth.data(), npix * sizeof(float), hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int n[3] = {512, 128, 512};
  const float voxel = 0.1f;
  const size_t nvox = (size_t)n[0] * n[1] * n[2];
  const vdo_dense_params p{{n[0], n[1], n[2]}, voxel, {-n[0] / 2, -n[1] / 2, -n[2] / 4}, {(float)fx, (float)fy, (float)cx, (float)cy}, 4.f * voxel, 0.f, 40.f, 64, 1 << 20};
  vdo_dense* map = nullptr;
  if (vdo_dense_create(ctx, W, H, &p, &map) != VDO_OK) { std::fprintf(stderr, "vdo_dense_create: %s\n", vdo_last_error()); return 1; }
  const float near = voxel, step = p.trunc / 2.f;
  const int n_steps = (int)std::ceil(((double)p.max_depth - near) / step) + 1;
  const vdo_raycast_params rp{{p.K[0], p.K[1], p.K[2], p.K[3]}, near, step, n_steps, 2};
  vdo_raycast* view = nullptr;
  if (vdo_raycast_create(map, W, H, &rp, &view) != VDO_OK) { std::fprintf(stderr, "vdo_raycast_create: %s\n", vdo_last_error()); return 1; }
  uint32_t *d_vol = nullptr, *d_copy = nullptr;
  vdo_dense_device_volume(map, &d_vol);
  CK(hipMalloc((void**)&d_copy, nvox * sizeof(uint32_t)));
  float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  T[3] = 0.013f; T[7] = -0.007f; T[11] = 0.021f;
  const double a = 20.0 * 3.14159265358979323846 / 180.0;
  float T2[16] = {(float)std::cos(a), 0, (float)std::sin(a), 0.3f, 0, 1, 0, 0, (float)-std::sin(a), 0, (float)std::cos(a), 0.1f, 0, 0, 0, 1};
  int64_t out[3] = {0, 0, 0};
  for (int r = 0; r < 4; ++r)
    if (vdo_dense_integrate(map, d_depth, W, nullptr, 0, 1, T, out) != VDO_OK) { std::fprintf(stderr, "vdo_dense_integrate: %s\n", vdo_last_error()); return 1; }
  std::printf("volume %d x %d x %d (%.0f MiB), voxel %.2f m, fused 4 times (%lld voxels updated per frame); view %d x %d, near %.2f m, step %.2f m, %d samples per ray, min_weight 2\n", n[0],
              n[1], n[2], nvox * 4.0 / (1 << 20), voxel, (long long)out[0], W, H, near, step, n_steps);
  static const char* const names[6] = {"hipMemcpyAsync device to device of the volume", "vdo_dense_integrate (the same frame again)", "vdo_raycast_render, fusing pose, skipping on",
                                       "vdo_raycast_render, fusing pose, skipping off", "vdo_raycast_render, turned 20 deg, skipping on", "vdo_raycast_render, turned 20 deg, skipping off"};
  for (int which = 0; which < 6; ++which) {
    std::vector<double> ev, own, grid;
    if (which >= 2) vdo_raycast_set_skip(view, which % 2 == 0);
    for (int r = 0; r < warm + runs; ++r) {
      int rc = VDO_OK;
      CK(hipEventRecord(e0, stream));
      if (which == 0) CK(hipMemcpyAsync(d_copy, d_vol, nvox * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
      else if (which == 1) rc = vdo_dense_integrate(map, d_depth, W, nullptr, 0, 1, T, out);
      else rc = vdo_raycast_render(view, which < 4 ? T : T2, d_out_depth, d_out_grad, d_out_wgt, 1, out);
      if (rc != VDO_OK) { std::fprintf(stderr, "%s: %s\n", names[which], vdo_last_error()); return 1; }
      CK(hipEventRecord(e1, stream)); CK(hipEventSynchronize(e1));
      float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
      double m2[2] = {0, 0}, g = 0;
      if (which == 1) vdo_dense_last_timing(map, m2);
      if (which >= 2) { vdo_raycast_last_timing(view, m2); vdo_raycast_grid_timing(view, &g); }
      if (r >= warm) { ev.push_back(ms); own.push_back(m2[1]); grid.push_back(g); }
    }
    const double lo_ms = *std::min_element(ev.begin(), ev.end()), hi_ms = *std::max_element(ev.begin(), ev.end()), med = median(ev), med_own = median(own), med_grid = median(grid);
    std::printf("  %-50s stream (hipEvents) median %.3f ms  min %.3f  max %.3f", names[which], med, lo_ms, hi_ms);
    if (which == 0) std::printf("  | %.2f TB/s read + written", 2.0 * nvox * 4 / (med * 1e-3) / 1e12);
    if (which == 1) std::printf("  | kernel alone (handle's events) median %.3f ms", med_own);
    if (which >= 2) {
      std::printf("  | device part (handle's events) median %.3f ms, of it the grid build %.3f ms  | hit %lld, missed %lld, no valid sample %lld of %zu rays", med_own, med_grid,
                  (long long)out[0], (long long)out[1], (long long)out[2], npix);
    }
    std::printf("  (%d runs after %d)\n", runs, warm);
  }
  CK(hipFree(d_copy));
  vdo_raycast_destroy(view);
  vdo_dense_destroy(map);
  vdo_ctx_destroy(ctx);
  return 0;
}
