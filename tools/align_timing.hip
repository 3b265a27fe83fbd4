// Times the aligner (vdo_align_linearise, vdo_align_solve, csrc/align.hip) on a device-resident frame against a view of a device-resident volume:
// hipEvents on the context's stream around the call, warm-up, median over the runs - one linearisation and one full solve, with subsample 1 and 2 -
// and, as the yardstick in the same program, the render of the same view (vdo_raycast_render through vdo_align_set_model_from_view).  The scene is
// that of tools/raycast_timing.hip - the ground 1.65 m below the camera and a wall 25 m ahead - with a wall 6 m to the right, so that all six motions
// are constrained, fused 4 times into a 512 x 128 x 512 volume of 0.1 m voxels around the camera; the frame is the fusing camera's depth image
// (1242 x 375), its pose estimate off by 3 cm and 0.5 degrees.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/align_timing.hip -Iinclude -Lvdo_slam_amd -lvdo_hip -Wl,-rpath,'$ORIGIN/../vdo_slam_amd' -o tools/align_timing
//   tools/align_timing [width=1242] [height=375] [runs=30]
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
  if (W < 1 || H < 1 || runs < 1) { std::fprintf(stderr, "usage: align_timing [width] [height] [runs]\n"); return 2; }
  const size_t npix = (size_t)W * H;
  const double fx = 721.5377 * W / 1242.0, fy = 721.5377 * H / 375.0, cx = 0.49 * W, cy = 0.46 * H;
  std::vector<float> depth(npix);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const double ahead = y > cy + 2 ? std::min(25.0, 1.65 * fy / (y - cy)) : 25.0;                   // the ground, then the wall ahead
      depth[(size_t)y * W + x] = (float)(x > cx + 2 ? std::min(ahead, 6.0 * fx / (x - cx)) : ahead);   // and a wall 6 m to the right: three directions
    }
  hipStream_t stream;
  CK(hipStreamCreate(&stream));
  vdo_ctx* ctx = nullptr;
  if (vdo_ctx_create(0, stream, &ctx) != VDO_OK) { std::fprintf(stderr, "vdo_ctx_create: %s\n", vdo_last_error()); return 1; }
  float* d_depth;
  CK(hipMalloc((void**)&d_depth, npix * sizeof(float)));
  CK(hipMemcpy(d_depth, depth.data(), npix * sizeof(float), hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int n[3] = {512, 128, 512};
  const float voxel = 0.1f;
  const vdo_dense_params p{{n[0], n[1], n[2]}, voxel, {-n[0] / 2, -n[1] / 2, -n[2] / 4}, {(float)fx, (float)fy, (float)cx, (float)cy}, 4.f * voxel, 0.f, 40.f, 64, 1 << 20};
  vdo_dense* map = nullptr;
  if (vdo_dense_create(ctx, W, H, &p, &map) != VDO_OK) { std::fprintf(stderr, "vdo_dense_create: %s\n", vdo_last_error()); return 1; }
  const float near = voxel, step = p.trunc / 2.f;
  const int n_steps = (int)std::ceil(((double)p.max_depth - near) / step) + 1;
  const vdo_raycast_params rp{{p.K[0], p.K[1], p.K[2], p.K[3]}, near, step, n_steps, 2};
  vdo_raycast* view = nullptr;
  if (vdo_raycast_create(map, W, H, &rp, &view) != VDO_OK) { std::fprintf(stderr, "vdo_raycast_create: %s\n", vdo_last_error()); return 1; }
  float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  T[3] = 0.013f; T[7] = -0.007f; T[11] = 0.021f;
  const double a = 0.5 * 3.14159265358979323846 / 180.0;
  float Ti[16] = {(float)std::cos(a), 0, (float)std::sin(a), T[3] + 0.02f, 0, 1, 0, T[7] - 0.01f, (float)-std::sin(a), 0, (float)std::cos(a), T[11] + 0.02f, 0, 0, 0, 1};
  int64_t out[3] = {0, 0, 0};
  for (int r = 0; r < 4; ++r)
    if (vdo_dense_integrate(map, d_depth, W, nullptr, 0, 1, T, out) != VDO_OK) { std::fprintf(stderr, "vdo_dense_integrate: %s\n", vdo_last_error()); return 1; }
  std::printf("volume %d x %d x %d, voxel %.2f m, fused 4 times; frame and view %d x %d, %d samples per ray; max_dist %.2f m, eps 1e-5, at most 10 iterations\n", n[0], n[1], n[2], voxel, W, H,
              n_steps, p.trunc);
  for (int sub = 1; sub <= 2; ++sub) {
    const int Ws = (W + sub - 1) / sub, Hs = (H + sub - 1) / sub;
    const vdo_align_params ap{{p.K[0], p.K[1], p.K[2], p.K[3]}, 0.f, 40.f, p.trunc, sub, Ws * Hs / 16, 10, 1e-5f, 0};
    vdo_align* al = nullptr;
    if (vdo_align_create(ctx, W, H, &ap, &al) != VDO_OK) { std::fprintf(stderr, "vdo_align_create: %s\n", vdo_last_error()); return 1; }
    static const char* const names[3] = {"vdo_align_set_model_from_view (the render)", "vdo_align_linearise", "vdo_align_solve"};
    for (int which = 0; which < 3; ++which) {
      std::vector<double> ev, own, wall;
      double sums[28];
      int64_t counts[5] = {0, 0, 0, 0, 0};
      float To[16];
      vdo_align_report rep{};
      for (int r = 0; r < warm + runs; ++r) {
        int rc = VDO_OK;
        CK(hipEventRecord(e0, stream));
        if (which == 0) rc = vdo_align_set_model_from_view(al, view, Ti, out);
        else if (which == 1) rc = vdo_align_linearise(al, d_depth, W, nullptr, 0, 1, Ti, sums, counts);
        else rc = vdo_align_solve(al, d_depth, W, nullptr, 0, 1, Ti, To, &rep, nullptr);
        if (rc != VDO_OK) { std::fprintf(stderr, "%s: %s\n", names[which], vdo_last_error()); return 1; }
        CK(hipEventRecord(e1, stream)); CK(hipEventSynchronize(e1));
        float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
        double m2[2] = {0, 0};
        if (which >= 1) vdo_align_last_timing(al, m2);
        if (r >= warm) { ev.push_back(ms); own.push_back(m2[1]); wall.push_back(m2[0]); }
      }
      const double lo_ms = *std::min_element(ev.begin(), ev.end()), hi_ms = *std::max_element(ev.begin(), ev.end()), med = median(ev), med_own = median(own), med_wall = median(wall);
      std::printf("  subsample %d  %-44s stream (hipEvents) median %.3f ms  min %.3f  max %.3f", sub, names[which], med, lo_ms, hi_ms);
      if (which == 0) std::printf("  | hit %lld, missed %lld, no valid sample %lld of %zu rays", (long long)out[0], (long long)out[1], (long long)out[2], npix);
      if (which == 1)
        std::printf("  | kernels alone (handle's events) median %.3f ms, wall %.3f ms  | used %lld, no depth %lld, masked %lld, no model %lld, far %lld of %d samples", med_own, med_wall,
                    (long long)counts[0], (long long)counts[1], (long long)counts[2], (long long)counts[3], (long long)counts[4], Ws * Hs);
      if (which == 2)
        std::printf("  | kernels alone median %.3f ms, wall %.3f ms  | %d iterations, status %d, used %lld, rms %.4f -> %.4f m", med_own, med_wall, rep.iterations, rep.status, (long long)rep.used,
                    rep.rms_first, rep.rms_last);
      std::printf("  (%d runs after %d)\n", runs, warm);
    }
    vdo_align_destroy(al);
  }
  vdo_raycast_destroy(view);
  vdo_dense_destroy(map);
  vdo_ctx_destroy(ctx);
  return 0;
}
