// Potential and gradient of the two-layer Bayesian neural network of the BNN study (reference mcmc_svi_transformer_on_bayesian.py:28-67, `BayesianModel`:
// fc1 F -> H, fc2 H -> 2, N(0,1) on every weight and bias, a categorical likelihood on softmax(out)), for every chain of every problem in ONE launch, and the
// class-1 probability of every chain at test points.  The caller is mcmc.batched_nuts: one call of pfn_bnn_logp_grad per leapfrog of all chains.
// DESIGN.md section 16 has the mapping and its bound; include/pfn_hip.h the contract.
//
// Mapping: lane = hidden unit, a group of Hp lanes holds one CHAIN and 64 / Hp chains share a wave (bnn_device.h has the mapping and the shared pieces).  The
// gradient needs no cross-lane reduction and no LDS; the one butterfly per data row has a fixed order, which makes a chain's result a bitwise function of its
// own inputs, wherever it sits in the launch.  All chains of a block belong to one problem; the block stages that problem's rows in LDS in chunks of 64 and
// every lane reads them as broadcasts.  Rows >= n are never read.  Padding lanes (j >= H) and the lanes of chains beyond K hold zeros for every parameter:
// they add exact zeros.
#include <algorithm>
#include "bnn_device.h"

namespace pfn {

struct BnnArgs {
  const float* x;        // [P,S,F]
  const float* y;        // [P,S]: class = y > 0.5
  const int32_t* n_of;   // [P] rows in use per problem (device; clamped to [0,S]); null = S
  const float* theta;    // [P*K, ld]: W1 [H,F], b1 [H], W2 [2,H], b2 [2]
  long ld;
  int P, K, S, F, H, activation;      // activation: 0 identity, 1 tanh
  float* value;          // [P*K]
  float* grad;           // [P*K, ld] or null; columns >= D are never written
  const float* x_test;   // [P,m,F]   (predict)
  int m;
  float* prob1;          // [P*K, m]
};

namespace {

struct BnnChain {
  int p, k, j;
  long c;
  bool wave_on, chain, on;
};

template <int HP> PFN_DEV BnnChain bnn_chain(int K, int H) {
  constexpr int CPW = 64 / HP;
  const int cpb = (blockDim.x >> 6) * CPW, kblocks = (K + cpb - 1) / cpb;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  BnnChain ch;
  ch.p = blockIdx.x / kblocks;
  const int k0 = (blockIdx.x % kblocks) * cpb + wave * CPW;
  ch.k = k0 + lane / HP;
  ch.j = lane & (HP - 1);
  ch.c = (long)ch.p * K + ch.k;
  ch.wave_on = k0 < K;
  ch.chain = ch.k < K;
  ch.on = ch.chain && ch.j < H;
  return ch;
}

template <int HP, int FP, int ACT> __global__ void __launch_bounds__(64 * BNN_MAX_WAVES) bnn_logp_grad_kernel(BnnArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[BNN_CHUNK * FP];
  __shared__ float ys[BNN_CHUNK];
  const int F = a.F, H = a.H;
  const BnnChain ch = bnn_chain<HP>(a.K, H);
  const int j = ch.j;
  const float* th = a.theta + ch.c * a.ld;      // read only where ch.on / ch.chain
  const BnnSlots<FP> sl(F, H, j);
  BnnLane<FP> L;
#pragma unroll
  for (int f = 0; f < FP; ++f) L.w1[f] = (ch.on && f < F) ? th[j * F + f] : 0.f;
  L.b1 = ch.on ? th[sl.oB1 + j] : 0.f;
  const float w20 = ch.on ? th[sl.oW2 + j] : 0.f, w21 = ch.on ? th[sl.oW2 + H + j] : 0.f;
  const float b20 = ch.chain ? th[sl.oB2] : 0.f, b21 = ch.chain ? th[sl.oB2 + 1] : 0.f;
  L.w2d = w21 - w20;
  const float b2d = b21 - b20;
  const int n = bnn_n_rows(a.n_of, ch.p, a.S);

  BnnSums<FP> sm;      // dW1[j,:], db1[j], A = sum_i g_i a_j, G = sum_i g_i, U = sum_i softplus
  sm.clear();

  bnn_data_rows<HP, FP, ACT, BNN_ROWS>(L, b2d, xs, ys, a.x + (long)ch.p * a.S * F, a.y + (long)ch.p * a.S, n, F, false, ch.wave_on, sm);
  if (!ch.wave_on) return;
  float q = L.b1 * L.b1 + w20 * w20 + w21 * w21;
#pragma unroll
  for (int f = 0; f < FP; ++f) q = __builtin_fmaf(L.w1[f], L.w1[f], q);
  q = bnn_group_sum<HP>(q) + b20 * b20 + b21 * b21;
  if (!ch.on) return;
  const int D = H * (F + 3) + 2;
  if (j == 0) a.value[ch.c] = 0.5f * q + (float)D * HALF_LOG_2PI + sm.U;
  if (!a.grad) return;
  float* gr = a.grad + ch.c * a.ld;
#pragma unroll
  for (int f = 0; f < FP; ++f)
    if (f < F) gr[j * F + f] = sm.dw1[f] + L.w1[f];
  gr[sl.oB1 + j] = sm.db1 + L.b1;
  gr[sl.oW2 + j] = w20 - sm.A;
  gr[sl.oW2 + H + j] = w21 + sm.A;
  if (j == 0) {
    gr[sl.oB2] = b20 - sm.G;
    gr[sl.oB2 + 1] = b21 + sm.G;
  }
}

template <int HP, int FP, int ACT> __global__ void __launch_bounds__(64 * BNN_MAX_WAVES) bnn_predict_kernel(BnnArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[BNN_CHUNK * FP];
  const int F = a.F, H = a.H;
  const BnnChain ch = bnn_chain<HP>(a.K, H);
  const int j = ch.j;
  const float* th = a.theta + ch.c * a.ld;
  const BnnSlots<FP> sl(F, H, j);
  BnnLane<FP> L;
#pragma unroll
  for (int f = 0; f < FP; ++f) L.w1[f] = (ch.on && f < F) ? th[j * F + f] : 0.f;
  L.b1 = ch.on ? th[sl.oB1 + j] : 0.f;
  L.w2d = ch.on ? th[sl.oW2 + H + j] - th[sl.oW2 + j] : 0.f;
  const float b2d = ch.chain ? th[sl.oB2 + 1] - th[sl.oB2] : 0.f;
  for (int r0 = 0; r0 < a.m; r0 += BNN_CHUNK) {
    const int rows = min(BNN_CHUNK, a.m - r0);
    __syncthreads();
    bnn_stage<FP>(xs, a.x_test + (long)ch.p * a.m * F, r0, rows, F);
    __syncthreads();
    if (!ch.wave_on) continue;
    for (int r = 0; r < rows; r += BNN_ROWS) {      // rows of the chunk beyond `rows` are zeros in LDS: computed, not stored
      float pv[BNN_ROWS];
#pragma unroll
      for (int q = 0; q < BNN_ROWS; ++q) pv[q] = L.w2d * bnn_hidden<FP, ACT>(L, xs + (r + q) * FP);
#pragma unroll
      for (int o = 1; o < HP; o <<= 1) {
#pragma unroll
        for (int q = 0; q < BNN_ROWS; ++q) pv[q] += __shfl_xor(pv[q], o, 64);
      }
#pragma unroll
      for (int q = 0; q < BNN_ROWS; ++q) {
        const float d = pv[q] + b2d;
        if (ch.chain && j == 0 && r + q < rows) a.prob1[ch.c * a.m + r0 + r + q] = bnn_sigmoid(d, expf(-fabsf(d)));
      }
    }
  }
}

int bnn_launch(const BnnArgs& a, bool predict, hipStream_t s) {
  return bnn_dispatch(a.H, a.F, a.activation, [&](auto hp, auto fp, auto act) {
    constexpr int HP = decltype(hp)::value, FP = decltype(fp)::value, ACT = decltype(act)::value, CPW = 64 / HP;
    const int waves = std::min(BNN_MAX_WAVES, (a.K + CPW - 1) / CPW), cpb = waves * CPW;
    const long blocks = (long)a.P * ((a.K + cpb - 1) / cpb);
    const dim3 grid((unsigned)blocks), block(64 * waves);
    if (predict) bnn_predict_kernel<HP, FP, ACT><<<grid, block, 0, s>>>(a);
    else bnn_logp_grad_kernel<HP, FP, ACT><<<grid, block, 0, s>>>(a);
    return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
  });
}

}  // namespace
}  // namespace pfn

using namespace pfn;

extern "C" {
int pfn_bnn_logp_grad(const float* x, const float* y, const int32_t* n_of, const float* theta, int64_t ld, int P, int K, int S, int F, int H, int activation,
                      float* value, float* grad, void* stream) {
  if (int rc = bnn_check(P, K, F, H, activation, ld)) return rc;
  if (S < 1 || !x || !y || !theta || !value) return fail(PFN_ERR_ARGUMENT, "bad bnn_logp_grad arguments (S %d >= 1, x, y, theta, value not NULL)", S);
  BnnArgs a{};
  a.x = x; a.y = y; a.n_of = n_of; a.theta = theta; a.ld = ld; a.P = P; a.K = K; a.S = S; a.F = F; a.H = H; a.activation = activation; a.value = value; a.grad = grad;
  PFN_TRY(bnn_launch(a, false, (hipStream_t)stream));
  return PFN_OK;
}
int pfn_bnn_predict(const float* x_test, const float* theta, int64_t ld, int P, int K, int m, int F, int H, int activation, float* prob1, void* stream) {
  if (int rc = bnn_check(P, K, F, H, activation, ld)) return rc;
  if (m < 0 || !theta || (m > 0 && (!x_test || !prob1))) return fail(PFN_ERR_ARGUMENT, "bad bnn_predict arguments (m %d >= 0, x_test, theta, prob1 not NULL)", m);
  if (m == 0) return PFN_OK;
  BnnArgs a{};
  a.theta = theta; a.ld = ld; a.P = P; a.K = K; a.F = F; a.H = H; a.activation = activation; a.x_test = x_test; a.m = m; a.prob1 = prob1;
  PFN_TRY(bnn_launch(a, true, (hipStream_t)stream));
  return PFN_OK;
}
}  // extern "C"
