// The stereo rectifier's map planner: host only, fp64, no device and no context (like ba_plan.hpp).  The contract is written out in
// include/vdo_slam_hip.h (vdo_rectify_plan) and restated in NumPy by tests/rectify_ref.py.  Every operation below is one fp64 operation rounded on
// its own, in the order of the contract; the library is compiled without contraction, and a stand-alone host program may include this header.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/vdo_slam_hip.h"

namespace vdo {

constexpr int32_t kRectInvalid = INT32_MIN;               // both coordinates of an invalid map entry
constexpr int64_t kRectMaxPixels = int64_t(1) << 26;

// Bilinear validity of a stored (qx, qy) against a source of ws x hs: what the remap kernel re-derives (rectify.hip, rect_pixel).
inline bool rect_map_valid(int32_t qx, int32_t qy, int ws, int hs) {
  const int ix = qx >> 5, ax = qx & 31, iy = qy >> 5, ay = qy & 31;
  return ix >= 0 && iy >= 0 && ix + (ax > 0) <= ws - 1 && iy + (ay > 0) <= hs - 1;
}

// Checks params, and `cam` unless it is -1.  Returns nullptr when everything is in order, else a message naming the argument (in `msg`).
inline const char* rect_check_params(const vdo_rectify_params* p, int cam, char* msg, size_t cap) {
  if (!p) { std::snprintf(msg, cap, "params is null"); return msg; }
  if (p->n_cams < 1 || p->n_cams > 2) { std::snprintf(msg, cap, "n_cams %d outside 1..2", p->n_cams); return msg; }
  if (cam != -1 && (cam < 0 || cam >= p->n_cams)) { std::snprintf(msg, cap, "cam %d outside 0..%d", cam, p->n_cams - 1); return msg; }
  if (p->width < 1) { std::snprintf(msg, cap, "width %d < 1", p->width); return msg; }
  if (p->height < 1) { std::snprintf(msg, cap, "height %d < 1", p->height); return msg; }
  static const char* const pn[4] = {"fx'", "fy'", "cx'", "cy'"};
  for (int k = 0; k < 4; ++k) {
    if (!std::isfinite(p->P[k])) { std::snprintf(msg, cap, "P[%d] (%s) is not finite", k, pn[k]); return msg; }
    if (k < 2 && !(p->P[k] > 0)) { std::snprintf(msg, cap, "P[%d] (%s) = %g is not positive", k, pn[k], p->P[k]); return msg; }
  }
  static const char* const kn[4] = {"fx", "fy", "cx", "cy"};
  for (int c = 0; c < p->n_cams; ++c) {
    const vdo_rectify_camera& q = p->cam[c];
    if (q.src_width < 1) { std::snprintf(msg, cap, "cam[%d].src_width %d < 1", c, q.src_width); return msg; }
    if (q.src_height < 1) { std::snprintf(msg, cap, "cam[%d].src_height %d < 1", c, q.src_height); return msg; }
    for (int k = 0; k < 4; ++k) {
      if (!std::isfinite(q.K[k])) { std::snprintf(msg, cap, "cam[%d].K[%d] (%s) is not finite", c, k, kn[k]); return msg; }
      if (k < 2 && !(q.K[k] > 0)) { std::snprintf(msg, cap, "cam[%d].K[%d] (%s) = %g is not positive", c, k, kn[k], q.K[k]); return msg; }
    }
    for (int k = 0; k < 5; ++k) if (!std::isfinite(q.D[k])) { std::snprintf(msg, cap, "cam[%d].D[%d] is not finite", c, k); return msg; }
    for (int k = 0; k < 9; ++k) if (!std::isfinite(q.R[k])) { std::snprintf(msg, cap, "cam[%d].R[%d] is not finite", c, k); return msg; }
  }
  return nullptr;
}

// The map of camera `cam`: map [H][W][2] = (qx, qy), valid [H][W] (may be null), *n_valid (may be null).  The parameters have been checked.
inline void rect_plan_map(const vdo_rectify_params* p, int cam, int32_t* map, uint8_t* valid, int32_t* n_valid) {
  const vdo_rectify_camera& q = p->cam[cam];
  const double fx = q.K[0], fy = q.K[1], cx = q.K[2], cy = q.K[3];
  const double k1 = q.D[0], k2 = q.D[1], p1 = q.D[2], p2 = q.D[3], k3 = q.D[4];
  const double* R = q.R;
  const double fxp = p->P[0], fyp = p->P[1], cxp = p->P[2], cyp = p->P[3];
  const int W = p->width, H = p->height, ws = q.src_width, hs = q.src_height;
  const double lim = 1073741824.0;                        // 2^30
  int32_t count = 0;
  for (int v = 0; v < H; ++v) {
    const double y = ((double)v - cyp) / fyp;
    for (int u = 0; u < W; ++u) {
      const double x = ((double)u - cxp) / fxp;
      const double X = (R[0] * x + R[3] * y) + R[6], Y = (R[1] * x + R[4] * y) + R[7], Wc = (R[2] * x + R[5] * y) + R[8];
      int32_t qx = kRectInvalid, qy = kRectInvalid;
      bool ok = false;
      if (Wc > 0) {
        const double xn = X / Wc, yn = Y / Wc;
        const double x2 = xn * xn, y2 = yn * yn, r2 = x2 + y2, xy2 = 2 * (xn * yn);
        double t = r2 * k3; t = k2 + t; t = r2 * t; t = k1 + t; t = r2 * t;
        const double kr = 1 + t;
        const double xd = (xn * kr + p1 * xy2) + p2 * (r2 + 2 * x2);
        const double yd = (yn * kr + p1 * (r2 + 2 * y2)) + p2 * xy2;
        const double us = fx * xd + cx, vs = fy * yd + cy;
        const double rx = std::nearbyint(32 * us), ry = std::nearbyint(32 * vs);          // ties to even (the default rounding mode)
        if (std::isfinite(rx) && std::isfinite(ry) && std::fabs(rx) < lim && std::fabs(ry) < lim) {
          const int32_t a = (int32_t)rx, b = (int32_t)ry;
          if (rect_map_valid(a, b, ws, hs)) { qx = a; qy = b; ok = true; }
        }
      }
      const size_t i = (size_t)v * W + u;
      map[2 * i] = qx; map[2 * i + 1] = qy;
      if (valid) valid[i] = ok ? 1 : 0;
      count += ok;
    }
  }
  if (n_valid) *n_valid = count;
}

}  // namespace vdo
