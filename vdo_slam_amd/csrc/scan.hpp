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

}  // namespace vdo
