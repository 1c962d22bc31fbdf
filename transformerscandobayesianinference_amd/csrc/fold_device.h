// Device code shared by the fold-based kernels of the tabular study that run one block of 256 threads per fit (logistic.hip, gpc.hip).  Only the block sum is
// here: the kernels' staging stays apart ("Tabular study, one copy of what the three baseline arms share").
#pragma once
#include "pfn_kernels.h"

namespace pfn {
namespace {

// the sum of v over the block's four waves; every thread calls, the result is the same bits in every thread.  red: 4 floats of LDS
__device__ __forceinline__ float block_sum(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();      // the previous use of red is over
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace
}  // namespace pfn
