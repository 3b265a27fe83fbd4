// Times the object stage (vdo_objects_stats and vdo_objects_integrate, csrc/objects.hip) on device-resident images: hipEvents on the context's stream
// around the call, warm-up, median over the runs.  The scene: a road-like depth ramp with a wall across it and `objects` labelled boxes in front of
// it, 2 % of the pixels without depth; one 96 x 64 x 96 volume of 50 mm voxels per box, centred on the box's surface.  Measured: the stats pass alone;
// the batched fusion of all objects with culling on and off; the same objects as one call each (n = 1); and, as the scale, one vdo_dense_integrate of
// a 512 x 128 x 512 static volume on the same frame.  A call of vdo_objects_integrate includes its own stats pass and two stream synchronisations.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/objects_timing.hip -Iinclude -Lvdo_slam_amd -lvdo_hip -Wl,-rpath,'$ORIGIN/../vdo_slam_amd' -o tools/objects_timing
//   tools/objects_timing [width=1242] [height=375] [objects=8] [runs=30]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "vdo_slam_hip.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
#define VK(x) do { if ((x) != VDO_OK) { std::fprintf(stderr, "%s: %s\n", #x, vdo_last_error()); return 1; } } while (0)

static double median(std::vector<double>& v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char** argv) {
  const int W = argc > 1 ? std::atoi(argv[1]) : 1242, H = argc > 2 ? std::atoi(argv[2]) : 375;
  const int nobj = argc > 3 ? std::atoi(argv[3]) : 8, runs = argc > 4 ? std::atoi(argv[4]) : 30, warm = 5;
  if (W < 16 || H < 16 || nobj < 1 || nobj > 64 || runs < 1) { std::fprintf(stderr, "usage: objects_timing [width] [height] [objects 1..64] [runs]\n"); return 2; }
  const size_t npix = (size_t)W * H;
  const double fx = 721.5377 * W / 1242.0, fy = 721.5377 * H / 375.0, cx = 0.49 * W, cy = 0.46 * H;
  std::mt19937 rng(7);
  std::vector<float> depth(npix);
  std::vector<int32_t> mask(npix, 0);
  std::vector<double> box_d(nobj), box_x(nobj), box_y(nobj);
  const int bw = W / (nobj + 2), bh = H / 4;                                    // the boxes side by side: at 1242 x 375 with 8 objects 124 x 93 pixels each
  for (int k = 0; k < nobj; ++k) { box_d[k] = 8.0 + 1.5 * (k % 5); box_x[k] = (k + 1) * (double)W / (nobj + 1); box_y[k] = H * 0.5; }
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t i = (size_t)y * W + x;
      double d = y > cy + 2 ? std::min(25.0, 1.65 * fy / (y - cy)) : 25.0;      // the ground 1.65 m below the camera, a wall 25 m ahead
      for (int k = 0; k < nobj; ++k)
        if (std::abs(x - box_x[k]) * 2 < bw && std::abs(y - box_y[k]) * 2 < bh) { d = box_d[k] + 0.002 * (x - box_x[k]); mask[i] = k + 1; }
      depth[i] = rng() % 100u < 2u ? 0.f : (float)d;
    }
  hipStream_t stream;
  CK(hipStreamCreate(&stream));
  vdo_ctx* ctx = nullptr;
  VK(vdo_ctx_create(0, stream, &ctx));
  float* d_depth; int32_t* d_mask;
  CK(hipMalloc((void**)&d_depth, npix * sizeof(float))); CK(hipMalloc((void**)&d_mask, npix * sizeof(int32_t)));
  CK(hipMemcpy(d_depth, depth.data(), npix * sizeof(float), hipMemcpyHostToDevice)); CK(hipMemcpy(d_mask, mask.data(), npix * sizeof(int32_t), hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const float K[4] = {(float)fx, (float)fy, (float)cx, (float)cy};
  const vdo_objects_params op{{K[0], K[1], K[2], K[3]}, 0.f, 25.f, 1023, 64};
  vdo_objects* st = nullptr;
  VK(vdo_objects_create(ctx, W, H, &op, &st));
  const int n[3] = {96, 64, 96};
  const float voxel = 0.05f;
  std::vector<vdo_dense*> maps(nobj);
  std::vector<int32_t> labels(nobj);
  std::vector<float> T(16 * (size_t)nobj, 0.f);
  for (int k = 0; k < nobj; ++k) {
    const vdo_dense_params p{{n[0], n[1], n[2]}, voxel, {-n[0] / 2, -n[1] / 2, -n[2] / 2}, {K[0], K[1], K[2], K[3]}, 4.f * voxel, 0.f, 25.f, 64, 1 << 16};
    VK(vdo_dense_create(ctx, W, H, &p, &maps[k]));
    labels[k] = k + 1;
    float* Tk = T.data() + 16 * (size_t)k;                                      // object frame = camera axes, its origin at the centre of the box's face
    Tk[0] = Tk[5] = Tk[10] = Tk[15] = 1.f;
    Tk[3] = (float)((box_x[k] - cx) * box_d[k] / fx); Tk[7] = (float)((box_y[k] - cy) * box_d[k] / fy); Tk[11] = (float)box_d[k];
  }
  std::vector<int64_t> out(3 * (size_t)nobj, 0);
  std::printf("image %d x %d, %d objects of %d x %d x %d voxels of %.0f mm, boxes of %d x %d pixels\n", W, H, nobj, n[0], n[1], n[2], voxel * 1e3, bw, bh);
  auto report = [&](const char* name, std::vector<double>& ev, std::vector<double>& own) {
    const double lo = *std::min_element(ev.begin(), ev.end()), hi = *std::max_element(ev.begin(), ev.end());
    std::printf("  %-64s stream (hipEvents) median %.3f ms  min %.3f  max %.3f  | device work alone (handle's events) median %.3f ms  (%d runs after %d)\n", name, median(ev), lo, hi,
                median(own), runs, warm);
  };
  for (int which = 0; which < 4; ++which) {                                     // stats; batched, culling on; batched, culling off; one call per object
    std::vector<double> ev, own;
    if (which == 1 || which == 3) VK(vdo_objects_set_cull(st, 1));
    if (which == 2) VK(vdo_objects_set_cull(st, 0));
    for (int r = 0; r < warm + runs; ++r) {
      double own_ms = 0;
      CK(hipEventRecord(e0, stream));
      if (which == 0) {
        VK(vdo_objects_stats(st, d_depth, W, d_mask, W, 1, nullptr));
      } else if (which < 3) {
        VK(vdo_objects_integrate(st, d_depth, W, d_mask, W, 1, nobj, maps.data(), labels.data(), T.data(), out.data()));
      } else {
        for (int k = 0; k < nobj; ++k) {
          VK(vdo_objects_integrate(st, d_depth, W, d_mask, W, 1, 1, &maps[k], &labels[k], T.data() + 16 * (size_t)k, out.data() + 3 * (size_t)k));
          double m2[2] = {0, 0}; vdo_objects_last_timing(st, m2); own_ms += m2[1];
        }
      }
      CK(hipEventRecord(e1, stream)); CK(hipEventSynchronize(e1));
      float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
      if (which < 3) { double m2[2] = {0, 0}; vdo_objects_last_timing(st, m2); own_ms = m2[1]; }
      if (r >= warm) { ev.push_back(ms); own.push_back(own_ms); }
    }
    static const char* const names[4] = {"vdo_objects_stats", "vdo_objects_integrate, one call over all objects, culling on", "vdo_objects_integrate, one call over all objects, culling off",
                                         "vdo_objects_integrate, one call per object (n = 1), culling on"};
    report(names[which], ev, own);
    if (which == 1) {
      long long upd = 0, occ = 0, pix = 0;
      for (int k = 0; k < nobj; ++k) { upd += out[3 * k]; occ += out[3 * k + 1]; pix += out[3 * k + 2]; }
      std::printf("    updated %lld, occluded %lld of %lld voxels; %lld labelled pixels\n", upd, occ, (long long)nobj * n[0] * n[1] * n[2], pix);
    }
  }
  {
    const int sn[3] = {512, 128, 512};
    const vdo_dense_params p{{sn[0], sn[1], sn[2]}, 0.1f, {-sn[0] / 2, -sn[1] / 2, -sn[2] / 4}, {K[0], K[1], K[2], K[3]}, 0.4f, 0.f, 40.f, 64, 1 << 20};
    vdo_dense* h = nullptr;
    VK(vdo_dense_create(ctx, W, H, &p, &h));
    float Ts[16] = {1, 0, 0, 0.013f, 0, 1, 0, -0.007f, 0, 0, 1, 0.021f, 0, 0, 0, 1};
    int64_t o3[3];
    std::vector<double> ev, own;
    for (int r = 0; r < warm + runs; ++r) {
      CK(hipEventRecord(e0, stream));
      VK(vdo_dense_integrate(h, d_depth, W, d_mask, W, 1, Ts, o3));
      CK(hipEventRecord(e1, stream)); CK(hipEventSynchronize(e1));
      float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
      double m2[2] = {0, 0}; vdo_dense_last_timing(h, m2);
      if (r >= warm) { ev.push_back(ms); own.push_back(m2[1]); }
    }
    report("vdo_dense_integrate, 512 x 128 x 512 static volume (the scale)", ev, own);
    vdo_dense_destroy(h);
  }
  for (int k = 0; k < nobj; ++k) vdo_dense_destroy(maps[k]);
  vdo_objects_destroy(st);
  vdo_ctx_destroy(ctx);
  return 0;
}
