// What the fold-based kernels of the tabular study share: the block sum of those that run one block of 256 threads per fit (logistic.hip, gpc.hip) -- the
// kernels' staging stays apart ("Tabular study, one copy of what the three baseline arms share") -- and, on the host, the shape check of their
// entry points and of pfn_knn_cv (tabular.hip).
#pragma once
#include <cstdio>
#include "pfn_host.h"

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

// The shape check of the four fold-based entry points (pfn_knn_cv, pfn_logistic_cv, pfn_gpc_lml_grad, pfn_gpc_predict): the ranges (PFN_ERR_UNSUPPORTED; `why` says
// what sets them) before P, n_splits and the pointers (PFN_ERR_ARGUMENT).  max_nc = 0: a call without candidates, max_splits = 0: one without n_splits (kNN).
inline int fold_shapes(const char* what, const char* why, int P, int n, int max_n, int T, int F, int NC, int max_nc, int n_splits, int max_splits, bool pointers) {
  char own[48] = "";      // the clause of what only some of the calls have
  if (n < 4 || n > max_n || T < 1 || T > 128 || F < 1 || F > 128 || (max_nc && (NC < 1 || NC > max_nc))) {
    if (max_nc) snprintf(own, sizeof own, ", NC %d outside 1 .. %d", NC, max_nc);
    return fail(PFN_ERR_UNSUPPORTED, "%s: n %d outside 4 .. %d, T %d outside 1 .. 128, F %d outside 1 .. 128%s (%s)", what, n, max_n, T, F, own, why);
  }
  if (P < 1 || (max_splits && (n_splits < 2 || n_splits > max_splits)) || !pointers) {
    if (max_splits) snprintf(own, sizeof own, ", 2 <= n_splits %d <= %d", n_splits, max_splits);
    return fail(PFN_ERR_ARGUMENT, "bad %s arguments (P %d >= 1%s, no NULL buffer)", what, P, own);
  }
  return PFN_OK;
}

}  // namespace pfn
