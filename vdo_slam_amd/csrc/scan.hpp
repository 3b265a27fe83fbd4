// Wave and workgroup exclusive scans of one int per thread: the ordered-compaction building block of frame.hip (K9, K10) and labels.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace vdo {

__device__ __forceinline__ int wave_excl_scan(int v, int lane, int* total) {
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off, 64); if (lane >= off) incl += t; }
  *total = __shfl(incl, 63, 64);
  return incl - v;
}

// workgroup exclusive scan (<=1024 threads); returns exclusive prefix, *total = sum. lds: int[17]
__device__ __forceinline__ int block_excl_scan(int v, int* lds, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  int wt;
  const int ex = wave_excl_scan(v, lane, &wt);
  __syncthreads();
  if (lane == 0) lds[wv] = wt;
  __syncthreads();
  if (threadIdx.x == 0) { int a = 0; for (int q = 0; q < nw; ++q) { const int t = lds[q]; lds[q] = a; a += t; } lds[16] = a; }
  __syncthreads();
  *total = lds[16];
  return ex + lds[wv];
}

// exclusive scan of per-workgroup counts (single workgroup of THREADS, each count below 2^31 / THREADS) with a 64-bit carry; the total goes to
// total_out[0].  The middle step of the ordered compactions of dense.hip and mesh.hip (a template, so that each of them launches its own copy)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_counts_scan(long long* __restrict__ blk, long long nblk, unsigned long long* __restrict__ total_out) {
  __shared__ int lds[17];
  long long carry = 0;
  for (long long b0 = 0; b0 < nblk; b0 += THREADS) {
    const long long i = b0 + threadIdx.x;
    const int v = i < nblk ? (int)blk[i] : 0;
    int total;
    const int ex = block_excl_scan(v, lds, &total);
    if (i < nblk) blk[i] = carry + ex;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) total_out[0] = (unsigned long long)carry;
}

}  // namespace vdo
