// Stand-alone check of the device SE(3) / pose-pose edge functions (se3_dev.hpp, ba_posepose.hip) against the CPU oracle's functions (oracle/ref_math.hpp,
// ref_edges.hpp) on every branch: compact_quat, edge_se3_dev, edge_prior_dev and iso_oplus bit for bit (Jacobians at the oracle's own bar against the
// reference, 4e-15 * max(1, max|J|)), huber_dev against a long-double evaluation at the bar its own comment claims.  One launch per section.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/se3_dev_check.hip -o tools/se3_dev_check
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../vdo_slam_amd/csrc/ba_posepose.hip"
#include "../oracle/ref_edges.hpp"

namespace ora = vdo_oracle;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

// ---------------------------------------------------------------- device side: one thread per input
__global__ void k_compact_quat(const double* in, double* out, int n) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  double m[9];
  for (int i = 0; i < 9; ++i) m[i] = in[(size_t)c * 9 + i];
  const vdo::D3 q = vdo::compact_quat(m);
  out[(size_t)c * 3] = q.x; out[(size_t)c * 3 + 1] = q.y; out[(size_t)c * 3 + 2] = q.z;
}
__global__ void k_edge_se3(const double* in, double* out, int n) {          // in: Z | Xi | Xj, out: e (6) | Ji (36) | Jj (36) | e of the errors-only call (6)
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const vdo::IsoD Z = vdo::iso_load(in + (size_t)c * 36), Xi = vdo::iso_load(in + (size_t)c * 36 + 12), Xj = vdo::iso_load(in + (size_t)c * 36 + 24);
  double e[6], Ji[36], Jj[36], e2[6];
  vdo::edge_se3_dev(Z, Xi, Xj, e, Ji, Jj);
  vdo::edge_se3_dev(Z, Xi, Xj, e2, nullptr, nullptr);
  double* o = out + (size_t)c * 84;
  for (int i = 0; i < 6; ++i) { o[i] = e[i]; o[78 + i] = e2[i]; }
  for (int i = 0; i < 36; ++i) { o[6 + i] = Ji[i]; o[42 + i] = Jj[i]; }
}
__global__ void k_edge_prior(const double* in, double* out, int n) {        // in: Z | X, out: e (6) | J (36)
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  double e[6], J[36];
  vdo::edge_prior_dev(vdo::iso_load(in + (size_t)c * 24), vdo::iso_load(in + (size_t)c * 24 + 12), e, J);
  double* o = out + (size_t)c * 42;
  for (int i = 0; i < 6; ++i) o[i] = e[i];
  for (int i = 0; i < 36; ++i) o[6 + i] = J[i];
}
__global__ void k_oplus(const double* in, double* out, int n) {             // in: X (12) | d (6) | ortho, out: X' (12)
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  double d[6];
  for (int i = 0; i < 6; ++i) d[i] = in[(size_t)c * 19 + 12 + i];
  const vdo::IsoD o = vdo::iso_oplus(vdo::iso_load(in + (size_t)c * 19), d, in[(size_t)c * 19 + 18] != 0.0);
  vdo::iso_store(out + (size_t)c * 12, o);
}
__global__ void k_huber(const double* in, double* out, int n) {             // in: e | delta | dsqr, out: huber_dev rho0, rho1 | huber rho0, rho1
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const double e = in[(size_t)c * 3], delta = in[(size_t)c * 3 + 1], dsqr = in[(size_t)c * 3 + 2];
  double a0, a1, b0, b1;
  vdo::huber_dev(e, delta, dsqr, a0, a1);
  vdo::huber(e, delta, dsqr, b0, b1);
  out[(size_t)c * 4] = a0; out[(size_t)c * 4 + 1] = a1; out[(size_t)c * 4 + 2] = b0; out[(size_t)c * 4 + 3] = b1;
}

template <class Kern>
static std::vector<double> run_kernel(Kern kern, const std::vector<double>& in, int n, int out_stride) {
  std::vector<double> out((size_t)n * out_stride, -7.0);
  double *d_in, *d_out;
  HIP_OK(hipMalloc(&d_in, in.size() * 8)); HIP_OK(hipMalloc(&d_out, out.size() * 8));
  HIP_OK(hipMemcpy(d_in, in.data(), in.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_out, out.data(), out.size() * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kern, dim3((n + 63) / 64), dim3(64), 0, 0, d_in, d_out, n);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(out.data(), d_out, out.size() * 8, hipMemcpyDeviceToHost));
  HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_out));
  return out;
}

// ---------------------------------------------------------------- inputs
static unsigned long long g_st = 88172645463325252ull;
static double u01() { g_st ^= g_st << 13; g_st ^= g_st >> 7; g_st ^= g_st << 17; return (double)(g_st >> 11) / 9007199254740992.0; }
static double uni(double a, double b) { return a + (b - a) * u01(); }
static const double kPi = 3.14159265358979323846;

static ora::M3 rodrigues(const double n[3], double th) {
  const double c = std::cos(th), s = std::sin(th), v = 1 - c;
  return ora::M3{{c + v * n[0] * n[0], v * n[0] * n[1] - s * n[2], v * n[0] * n[2] + s * n[1],
                  v * n[1] * n[0] + s * n[2], c + v * n[1] * n[1], v * n[1] * n[2] - s * n[0],
                  v * n[2] * n[0] - s * n[1], v * n[2] * n[1] + s * n[0], c + v * n[2] * n[2]}};
}
static void unit(double v[3]) { const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); v[0] /= n; v[1] /= n; v[2] /= n; }
static void sphere(double v[3]) {
  double n2;
  do { for (int i = 0; i < 3; ++i) v[i] = uni(-1, 1); n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]; } while (n2 > 1 || n2 < 0.01);
  unit(v);
}
static const double kHalfTurns[6][9] = {{1, 0, 0, 0, -1, 0, 0, 0, -1}, {-1, 0, 0, 0, 1, 0, 0, 0, -1}, {-1, 0, 0, 0, -1, 0, 0, 0, 1},
                                        {0, 1, 0, 1, 0, 0, 0, 0, -1}, {0, 0, 1, 0, -1, 0, 1, 0, 0}, {-1, 0, 0, 0, 0, 1, 0, 1, 0}};
static const int kExact = 48;     // inputs 0 .. kExact-1 of every rotation section: the six exactly representable half-turns, in turn
// Rotation of input c.  c < kExact: an exact half-turn.  Otherwise by c % 16: 0-3 any angle in [0, pi - 1e-3] about any axis; 4-5 trace > 0; 6-11 trace < 0 with
// diagonal entry (k - 6) / 2 dominant and its axis component positive (even k) or negative (odd k: the raw qw is negative); 12-15 trace < 0 with the two largest
// diagonal entries 1e-6 apart, every pair and either order.
static ora::M3 class_rotation(int c) {
  if (c < kExact) { ora::M3 R; std::memcpy(R.m, kHalfTurns[c % 6], 72); return R; }
  const int k = c % 16;
  double n[3];
  const double lo = 2 * kPi / 3 + 0.01, hi = kPi - 1e-3;
  if (k < 4) { sphere(n); return rodrigues(n, uni(0, hi)); }
  if (k < 6) { sphere(n); return rodrigues(n, uni(0, 2 * kPi / 3 - 0.01)); }
  if (k < 12) {
    const int i = (k - 6) / 2;
    for (int q = 0; q < 3; ++q) n[q] = uni(-0.5, 0.5);
    n[i] = (k & 1) ? -1.0 : 1.0;
    unit(n);
    return rodrigues(n, uni(lo, hi));
  }
  const int sub = (c / 16) % 12, pair = sub / 4, i = pair, j = (pair + 1) % 3, l = (pair + 2) % 3;      // sub % 4: which of the two is larger, sign of the components
  const double th = uni(lo, hi), rest = uni(0, 0.2), d = ((sub & 1) ? -1e-6 : 1e-6) / (1 - std::cos(th));
  const double sg = (sub & 2) ? -1.0 : 1.0;
  n[i] = sg * std::sqrt((1 - rest + d) / 2); n[j] = (u01() < 0.5 ? -1 : 1) * std::sqrt((1 - rest - d) / 2); n[l] = (u01() < 0.5 ? -1 : 1) * std::sqrt(rest);
  return rodrigues(n, th);
}
static ora::Iso random_iso() {
  double n[3];
  sphere(n);
  ora::Iso T;
  T.R = rodrigues(n, uni(0, kPi));
  const double s = u01() < 0.5 ? 1.0 : 10.0;
  T.t = {uni(-s, s), uni(-s, s), uni(-s, s)};
  return T;
}

// Which branch a rotation takes in toCompactQuaternion (Eigen's choice) and in _q2m (g2o's choice, the Jacobian)
struct Branches {
  long tr_pos = 0, neg[3] = {0, 0, 0}, neg_flip[3] = {0, 0, 0}, qw_zero = 0, tie_rules_differ = 0, jac[3] = {0, 0, 0}, jac_flip = 0;
  void add(const ora::M3& m) {
    const double t = m(0, 0) + m(1, 1) + m(2, 2);
    if (t > 0.0) { ++tr_pos; return; }
    const ora::Quat q = ora::quat_from_matrix(m);
    int i = 0;
    if (m(1, 1) > m(0, 0)) i = 1;
    if (m(2, 2) > m(i, i)) i = 2;
    if (q.w < 0) ++neg_flip[i]; else ++neg[i];
    if (q.w == 0) ++qw_zero;
    const int dm = ((m(0, 0) > m(1, 1)) & (m(0, 0) > m(2, 2))) ? 0 : m(1, 1) > m(2, 2) ? 1 : 2;
    ++jac[dm];
    if (dm != i) ++tie_rules_differ;
    const int j = (dm + 1) % 3, k = (dm + 2) % 3;
    if (m(k, j) - m(j, k) <= 0) ++jac_flip;
  }
  void print() const {
    printf(" tr_pos=%ld x=%ld x_flip=%ld y=%ld y_flip=%ld z=%ld z_flip=%ld qw_zero=%ld tie_rules_differ=%ld jac_x=%ld jac_y=%ld jac_z=%ld jac_flip=%ld", tr_pos, neg[0], neg_flip[0],
           neg[1], neg_flip[1], neg[2], neg_flip[2], qw_zero, tie_rules_differ, jac[0], jac[1], jac[2], jac_flip);
  }
};

static bool same_bits(const double* a, const double* b, int n) { return std::memcmp(a, b, (size_t)n * 8) == 0; }
static double ulp_of(double x) { x = std::fabs(x); return std::nextafter(x, INFINITY) - x; }
static double ulp_dist(double a, double b) {            // distance in representable numbers (same sign, finite)
  int64_t ia, ib;
  std::memcpy(&ia, &a, 8); std::memcpy(&ib, &b, 8);
  return (double)(ia > ib ? ia - ib : ib - ia);
}

static const int N = 24576;

// ---------------------------------------------------------------- compact_quat
static int check_compact_quat() {
  std::vector<double> in((size_t)N * 9);
  Branches br;
  for (int c = 0; c < N; ++c) { const ora::M3 R = class_rotation(c); std::memcpy(&in[(size_t)c * 9], R.m, 72); br.add(R); }
  const std::vector<double> got = run_kernel(k_compact_quat, in, N, 3);
  int bad = 0;
  for (int c = 0; c < N; ++c) {
    ora::M3 R; std::memcpy(R.m, &in[(size_t)c * 9], 72);
    const ora::V3 q = ora::toCompactQuaternion(R);
    const double want[3] = {q.x, q.y, q.z};
    if (!same_bits(want, &got[(size_t)c * 3], 3)) { if (bad < 5) printf("compact_quat input %d: got %.17g %.17g %.17g want %.17g %.17g %.17g\n", c, got[c * 3], got[c * 3 + 1], got[c * 3 + 2], q.x, q.y, q.z); ++bad; }
  }
  printf("compact_quat: n=%d", N); br.print(); printf(" mismatches=%d %s\n", bad, bad ? "MISMATCH" : "ok");
  return bad;
}

// Jacobian against the oracle's: the bar is 4e-15 * max(1, max|J|); returns the deviation in units of DBL_EPSILON * max(1, max|J|)
static double jac_dev(const double* got, const double* want, bool& in_bar, bool& identical) {
  double mx = 1.0, d = 0.0;
  for (int i = 0; i < 36; ++i) mx = std::max(mx, std::fabs(want[i]));
  for (int i = 0; i < 36; ++i) { const double x = std::fabs(got[i] - want[i]); if (!(x <= d)) d = x; }
  if (!(d <= 4e-15 * mx)) in_bar = false;
  if (!same_bits(got, want, 36)) identical = false;
  return d / (DBL_EPSILON * mx);
}

// ---------------------------------------------------------------- EdgeSE3
static int check_edge_se3() {
  std::vector<double> in((size_t)N * 36);
  Branches br;
  for (int c = 0; c < N; ++c) {
    ora::Iso Z, Xi, Xj, T;
    T.R = class_rotation(c);
    const double s = (c & 1) ? 1.0 : 10.0;
    T.t = {uni(-s, s), uni(-s, s), uni(-s, s)};
    if (c < kExact) { Xi.t = {uni(-s, s), uni(-s, s), uni(-s, s)}; Xj = T; }          // Z = I, Xi = (I, t), Xj = (half-turn, t'): E is exact
    else { Z = random_iso(); Xi = random_iso(); Xj = ora::iso_mul(ora::iso_mul(Xi, Z), T); }
    ora::iso_to12(Z, &in[(size_t)c * 36]); ora::iso_to12(Xi, &in[(size_t)c * 36 + 12]); ora::iso_to12(Xj, &in[(size_t)c * 36 + 24]);
    br.add(ora::iso_mul(ora::iso_inv(Z), ora::iso_mul(ora::iso_inv(Xi), Xj)).R);
  }
  const std::vector<double> got = run_kernel(k_edge_se3, in, N, 84);
  int bad_e = 0, bad_j = 0;
  bool identical = true;
  double worst = 0;
  for (int c = 0; c < N; ++c) {
    const double* p = &in[(size_t)c * 36];
    double e[6], Ji[36], Jj[36];
    ora::edge_se3(ora::iso_from12(p), ora::iso_from12(p + 12), ora::iso_from12(p + 24), e, Ji, Jj);
    const double* g = &got[(size_t)c * 84];
    if (!same_bits(e, g, 6) || !same_bits(e, g + 78, 6)) { if (bad_e < 5) printf("edge_se3 input %d: residual %.17g %.17g %.17g | %.17g %.17g %.17g want %.17g %.17g %.17g | %.17g %.17g %.17g\n", c, g[0], g[1], g[2], g[3], g[4], g[5], e[0], e[1], e[2], e[3], e[4], e[5]); ++bad_e; }
    bool ok = true;
    worst = std::max(worst, std::max(jac_dev(g + 6, Ji, ok, identical), jac_dev(g + 42, Jj, ok, identical)));
    if (!ok) { if (bad_j < 5) printf("edge_se3 input %d: Jacobian outside 4e-15 * max(1, max|J|)\n", c); ++bad_j; }
  }
  printf("edge_se3: n=%d", N); br.print();
  printf(" residual_mismatches=%d jacobians_outside_bar=%d jac_worst_eps=%.3g jac_bit_identical=%s %s\n", bad_e, bad_j, worst, identical ? "yes" : "no", (bad_e || bad_j) ? "MISMATCH" : "ok");
  return bad_e + bad_j;
}

// ---------------------------------------------------------------- EdgeSE3Prior
static int check_edge_prior() {
  std::vector<double> in((size_t)N * 24);
  Branches br;
  for (int c = 0; c < N; ++c) {
    ora::Iso Z, X, T;
    T.R = class_rotation(c);
    const double s = (c & 1) ? 1.0 : 10.0;
    T.t = {uni(-s, s), uni(-s, s), uni(-s, s)};
    if (c < kExact) { Z.t = {uni(-s, s), uni(-s, s), uni(-s, s)}; X = T; }
    else { Z = random_iso(); X = ora::iso_mul(Z, T); }
    ora::iso_to12(Z, &in[(size_t)c * 24]); ora::iso_to12(X, &in[(size_t)c * 24 + 12]);
    br.add(ora::iso_mul(ora::iso_inv(Z), X).R);
  }
  const std::vector<double> got = run_kernel(k_edge_prior, in, N, 42);
  int bad_e = 0, bad_j = 0;
  bool identical = true;
  double worst = 0;
  for (int c = 0; c < N; ++c) {
    const double* p = &in[(size_t)c * 24];
    double e[6], J[36];
    ora::edge_prior(ora::iso_from12(p), ora::iso_from12(p + 12), e, J);
    const double* g = &got[(size_t)c * 42];
    if (!same_bits(e, g, 6)) { if (bad_e < 5) printf("edge_prior input %d: residual %.17g %.17g %.17g | %.17g %.17g %.17g want %.17g %.17g %.17g | %.17g %.17g %.17g\n", c, g[0], g[1], g[2], g[3], g[4], g[5], e[0], e[1], e[2], e[3], e[4], e[5]); ++bad_e; }
    bool ok = true;
    worst = std::max(worst, jac_dev(g + 6, J, ok, identical));
    if (!ok) { if (bad_j < 5) printf("edge_prior input %d: Jacobian outside 4e-15 * max(1, max|J|)\n", c); ++bad_j; }
  }
  printf("edge_prior: n=%d", N); br.print();
  printf(" residual_mismatches=%d jacobians_outside_bar=%d jac_worst_eps=%.3g jac_bit_identical=%s %s\n", bad_e, bad_j, worst, identical ? "yes" : "no", (bad_e || bad_j) ? "MISMATCH" : "ok");
  return bad_e + bad_j;
}

// ---------------------------------------------------------------- VertexSE3::oplusImpl
static int check_oplus() {
  std::vector<double> in((size_t)N * 19);
  long n_inside = 0, n_outside = 0, n_on = 0, n_zero = 0, n_ortho = 0, n_skewed = 0;
  for (int c = 0; c < N; ++c) {
    ora::Iso X = random_iso();
    const int k = c % 8;
    if ((c / 16) % 3 == 0) { for (int i = 0; i < 9; ++i) X.R.m[i] += uni(-1e-3, 1e-3); ++n_skewed; }      // R off orthogonality by 1e-3
    double d[6] = {uni(-2, 2), uni(-2, 2), uni(-2, 2), 0, 0, 0}, n[3];
    sphere(n);
    double r2 = 0;                                                                      // |q|^2: never within 1e-6 of 1 unless exactly 1
    if (k < 3) r2 = uni(0, 0.25);
    else if (k < 5) r2 = uni(0.9, 0.99);
    else if (k < 7) r2 = uni(1.01, 2.0);
    for (int i = 0; i < 3; ++i) d[3 + i] = std::sqrt(r2) * n[i];                        // (k == 7: |q| = 0)
    if (c < 12) { d[3] = d[4] = d[5] = 0; d[3 + c % 3] = (c % 6 < 3) ? 1.0 : -1.0; }    // |q|^2 == 1 exactly: w = 0, the square-root branch
    const double q2 = d[3] * d[3] + d[4] * d[4] + d[5] * d[5], w = 1 - q2;
    if (q2 != 1.0 && std::fabs(q2 - 1) < 1e-6) { printf("iso_oplus input %d: |q|^2 within 1e-6 of 1\n", c); return 1; }
    if (w < 0) ++n_outside; else if (w == 0) ++n_on; else if (q2 == 0) ++n_zero; else ++n_inside;
    const bool ortho = (c / 8) % 2 != 0;
    n_ortho += ortho;
    ora::iso_to12(X, &in[(size_t)c * 19]);
    for (int i = 0; i < 6; ++i) in[(size_t)c * 19 + 12 + i] = d[i];
    in[(size_t)c * 19 + 18] = ortho ? 1.0 : 0.0;
  }
  const std::vector<double> got = run_kernel(k_oplus, in, N, 12);
  int bad = 0;
  long r_kept = 0;
  for (int c = 0; c < N; ++c) {
    const double* p = &in[(size_t)c * 19];
    ora::Iso X = ora::iso_from12(p);
    int calls = p[18] != 0.0 ? 1000 : 0;
    ora::iso_oplus(X, p + 12, calls);
    double want[12];
    ora::iso_to12(X, want);
    if (!same_bits(want, &got[(size_t)c * 12], 12)) { if (bad < 5) printf("iso_oplus input %d (ortho %g): got R00 %.17g t %.17g want %.17g %.17g\n", c, p[18], got[(size_t)c * 12], got[(size_t)c * 12 + 9], want[0], want[9]); ++bad; }
    if (p[18] == 0.0 && same_bits(p, &got[(size_t)c * 12], 9)) ++r_kept;
  }
  printf("iso_oplus: n=%d inside=%ld outside=%ld on_sphere=%ld zero=%ld ortho=%ld skewed=%ld rotation_kept=%ld mismatches=%d %s\n", N, n_inside, n_outside, n_on, n_zero, n_ortho, n_skewed, r_kept,
         bad, bad ? "MISMATCH" : "ok");
  return bad;
}

// ---------------------------------------------------------------- RobustKernelHuber
static int check_huber() {
  std::vector<double> in;
  auto push = [&](double e, double delta) { in.push_back(e); in.push_back(delta); in.push_back((double)(float)(delta * delta)); };
  const double widths[6] = {1.1e-19, 1e-8, 1e-4, (double)std::sqrt(0.04f), 1.0, 1e3};
  for (const double delta : widths) {
    const double dsqr = (double)(float)(delta * delta);
    const double l0 = std::log(dsqr), l1 = std::log(1e300);
    for (int i = 0; i < 3600; ++i) { double e = std::exp(uni(l0, l1)); if (!(e > dsqr)) e = std::nextafter(dsqr, INFINITY); if (e > 1e300) e = 1e300; push(e, delta); }
    for (int i = 0; i < 400; ++i) push(std::max(std::nextafter(dsqr, INFINITY), dsqr * std::exp(uni(0, std::log(100.0)))), delta);
    for (int i = 0; i < 100; ++i) push(dsqr * u01(), delta);
    push(1e300, delta);
    push(std::nextafter(dsqr, INFINITY), delta);
    push(dsqr, delta);
    push(std::nextafter(dsqr, 0.0), delta);
    push(0.0, delta);
  }
  for (const double delta : {0.0, -1.0, -1e-4}) {
    for (int i = 0; i < 100; ++i) push(std::exp(uni(std::log(1e-30), std::log(1e30))), delta);
    push(0.0, delta);
  }
  const int n = (int)(in.size() / 3);
  const std::vector<double> got = run_kernel(k_huber, in, n, 4);
  int bad = 0;
  long n_in = 0, n_out = 0, n_off = 0, n_boundary = 0;
  double w0 = 0, w1 = 0, v0 = 0, v1 = 0;       // worst huber_dev error in ulps (rho0 against its larger term); worst distance huber_dev - huber()
  for (int c = 0; c < n; ++c) {
    const double e = in[(size_t)c * 3], delta = in[(size_t)c * 3 + 1], dsqr = in[(size_t)c * 3 + 2];
    const double* g = &got[(size_t)c * 4];
    if (delta <= 0 || e <= dsqr) {
      if (delta <= 0) ++n_off; else { ++n_in; if (e == dsqr) ++n_boundary; }
      if (!(g[0] == e && g[1] == 1.0 && g[2] == e && g[3] == 1.0)) { if (bad < 5) printf("huber input %d (e %.17g delta %g): inlier / no kernel gives rho %.17g %.17g, plain %.17g %.17g\n", c, e, delta, g[0], g[1], g[2], g[3]); ++bad; }
      continue;
    }
    ++n_out;
    const long double s = sqrtl((long double)e), big = 2 * s * (long double)delta, r0 = big - (long double)dsqr, r1 = (long double)delta / s;
    const double d0 = (double)(fabsl((long double)g[0] - r0) / (long double)ulp_of((double)big)), d1 = (double)(fabsl((long double)g[1] - r1) / (long double)ulp_of((double)r1));
    if (!(d0 <= 2.0 && d1 <= 2.0)) { if (bad < 5) printf("huber input %d (e %.17g delta %g): rho0 %.17g off by %.3g ulp of 2 sqrt(e) delta, rho1 %.17g off by %.3g ulp\n", c, e, delta, g[0], d0, g[1], d1); ++bad; }
    w0 = std::max(w0, d0); w1 = std::max(w1, d1);
    // the plain routine (VDO_SLOW_HUBER, the host): the same bar, and how far the fused sequence is from it
    const double p0 = (double)(fabsl((long double)g[2] - r0) / (long double)ulp_of((double)big)), p1 = (double)(fabsl((long double)g[3] - r1) / (long double)ulp_of((double)r1));
    if (!(p0 <= 2.0 && p1 <= 2.0)) { if (bad < 5) printf("huber input %d (e %.17g delta %g): plain huber() rho0 off by %.3g ulp, rho1 by %.3g ulp\n", c, e, delta, p0, p1); ++bad; }
    v0 = std::max(v0, std::fabs(g[0] - g[2]) / ulp_of((double)big)); v1 = std::max(v1, ulp_dist(g[1], g[3]));
  }
  printf("huber: n=%d inliers=%ld boundary=%ld outliers=%ld no_kernel=%ld rho0_worst_ulp=%.3f rho1_worst_ulp=%.3f vs_plain_rho0_ulp=%.3f vs_plain_rho1_ulp=%.0f mismatches=%d %s\n", n, n_in, n_boundary, n_out, n_off,
         w0, w1, v0, v1, bad, bad ? "MISMATCH" : "ok");
  return bad;
}

int main() {
  int bad = check_compact_quat();
  bad += check_edge_se3();
  bad += check_edge_prior();
  bad += check_oplus();
  bad += check_huber();
  return bad ? 1 : 0;
}
