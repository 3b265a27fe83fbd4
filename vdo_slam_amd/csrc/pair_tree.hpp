// The upper levels of the fixed adjacent-pair tree behind the sums of the aligner (align.hip) and the photometric aligner (photo.hip): 32 doubles per
// node - 28 terms and four counts as 0.0 / 1.0 -, v[k] = v[2k] + v[2k+1] level by level, so that no bit depends on the launch shape or the schedule.
// Each file keeps its own __global__ kernel around pt_tree, under its own name, and its own text of the first six levels (the wave's transposing
// xor-butterfly at the end of its row kernel): called through a function the butterfly moves k_al_rows' register count (profiles/photo_resources.txt).
//
//   pt_tree        eight levels over 256 consecutive nodes per workgroup of 256 threads: thread (sub, term) pairs 32 nodes of one term in registers
//                  (five levels), the eight subs meet in LDS (three levels).  Launched until one node is left: 2^20 tiles need three launches, a
//                  1242 x 375 frame two, the second a single workgroup of eight levels - there is no serial stage.  A node beyond the padded count
//                  does not exist: its partner passes through unchanged, as the contract's tree over the next power of two has it.
#pragma once
#include <hip/hip_runtime.h>

namespace vdo {

constexpr int kPtVals = 32;                                                // the 28 terms, then used, masked, no model, far as doubles
constexpr int kPtSpan = 256;                                               // nodes per workgroup of pt_tree

// Eight levels of the tree over the nodes [256 * block, 256 * block + 256) of every value: in [n_real][32] (a node >= n_real holds +0.0), P the
// padded node count (a power of two >= n_real), out [max(P / 256, 1)][32].  A pair whose second node lies beyond P's level does not exist.
// lds: the workgroup's [8][32] doubles.
__device__ __forceinline__ void pt_tree(const double* __restrict__ in, int n_real, int P, double* __restrict__ out, double (*lds)[kPtVals]) {
  const int term = threadIdx.x & 31, sub = threadIdx.x >> 5;
  const int n_loc = P < kPtSpan ? P : kPtSpan;
  const long long base = (long long)blockIdx.x * kPtSpan + sub * 32;
  double v[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) v[k] = base + k < n_real ? in[(size_t)(base + k) * kPtVals + term] : 0.0;
#pragma unroll
  for (int L = 0; L < 5; ++L) {
#pragma unroll
    for (int k = 0; k < (16 >> L); ++k) v[k] = sub * (32 >> L) + 2 * k + 1 < (n_loc >> L) ? v[2 * k] + v[2 * k + 1] : v[2 * k];
  }
  lds[sub][term] = v[0];
  __syncthreads();
  if (sub != 0) return;
  double r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = lds[k][term];
#pragma unroll
  for (int L = 5; L < 8; ++L) {
#pragma unroll
    for (int k = 0; k < (128 >> L); ++k) r[k] = 2 * k + 1 < (n_loc >> L) ? r[2 * k] + r[2 * k + 1] : r[2 * k];
  }
  out[(size_t)blockIdx.x * kPtVals + term] = r[0];
}

inline int pt_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }

}  // namespace vdo
