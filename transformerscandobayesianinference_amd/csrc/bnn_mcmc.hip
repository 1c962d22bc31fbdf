// Potential and gradient of the two-layer Bayesian neural network of the BNN study (reference mcmc_svi_transformer_on_bayesian.py:28-67, `BayesianModel`:
// fc1 F -> H, fc2 H -> 2, N(0,1) on every weight and bias, a categorical likelihood on softmax(out)), for every chain of every problem in ONE launch, and the
// class-1 probability of every chain at test points.  The caller is mcmc.batched_nuts: one call of pfn_bnn_logp_grad per leapfrog of all chains.
// DESIGN.md section 16 has the mapping and its bound; include/pfn_hip.h the contract.
//
// Mapping: lane = hidden unit.  Hp = H rounded up to 8 / 16 / 32 / 64 is a template parameter and 64 / Hp chains share a wave; a lane keeps W1[j,:], b1[j] and
// W2[:,j] of its chain in registers and accumulates dW1[j,:], db1[j] and dW2[:,j] there, so the gradient needs no cross-lane reduction and no LDS.  Only ONE
// number per data row is reduced over the Hp lanes of a chain: the two-class softmax depends on the logits through d = o_1 - o_0 alone, so the lanes sum
// (W2[1,j] - W2[0,j]) a_j -- one __shfl_xor butterfly per row instead of two -- in a fixed order (offsets 1, 2, .. Hp/2), which makes a chain's result a bitwise
// function of its own inputs, wherever it sits in the launch.  BNN_ROWS rows are in flight at once so their butterflies overlap.  All chains of a block belong
// to one problem; the block stages that problem's rows in LDS in chunks of 64 (zero padded to Fp = 4 / 8 / 16 columns) and every lane reads them as broadcasts.
// Rows >= n are never read.  Padding lanes (j >= H) and the lanes of chains beyond K hold zeros for every parameter: they add exact zeros.
#include <algorithm>
#include "bnn_device.h"
#include "pfn_kernels.h"

namespace pfn {

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
  const int oB1 = H * F, oW2 = oB1 + H, oB2 = oW2 + 2 * H;
  BnnLane<FP> L;
#pragma unroll
  for (int f = 0; f < FP; ++f) L.w1[f] = (ch.on && f < F) ? th[j * F + f] : 0.f;
  L.b1 = ch.on ? th[oB1 + j] : 0.f;
  const float w20 = ch.on ? th[oW2 + j] : 0.f, w21 = ch.on ? th[oW2 + H + j] : 0.f;
  const float b20 = ch.chain ? th[oB2] : 0.f, b21 = ch.chain ? th[oB2 + 1] : 0.f;
  L.w2d = w21 - w20;
  const float b2d = b21 - b20;
  int n = a.S;
  if (a.n_of) n = min(max(a.n_of[ch.p], 0), a.S);

  BnnSums<FP> sm;      // dW1[j,:], db1[j], A = sum_i g_i a_j, G = sum_i g_i, U = sum_i softplus
  sm.clear();

  for (int r0 = 0; r0 < n; r0 += BNN_CHUNK) {
    const int rows = min(BNN_CHUNK, n - r0);
    __syncthreads();      // the previous chunk has been consumed
    bnn_stage<FP>(xs, a.x + (long)ch.p * a.S * F, r0, rows, F);
    if (threadIdx.x < BNN_CHUNK) ys[threadIdx.x] = ((int)threadIdx.x < rows && a.y[(long)ch.p * a.S + r0 + threadIdx.x] > 0.5f) ? 1.f : 0.f;
    __syncthreads();
    if (ch.wave_on) bnn_rows<HP, FP, ACT>(L, b2d, xs, ys, rows, sm);      // wave-uniform: the butterflies run with all 64 lanes
  }
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
  gr[oB1 + j] = sm.db1 + L.b1;
  gr[oW2 + j] = w20 - sm.A;
  gr[oW2 + H + j] = w21 + sm.A;
  if (j == 0) {
    gr[oB2] = b20 - sm.G;
    gr[oB2 + 1] = b21 + sm.G;
  }
}

template <int HP, int FP, int ACT> __global__ void __launch_bounds__(64 * BNN_MAX_WAVES) bnn_predict_kernel(BnnArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[BNN_CHUNK * FP];
  const int F = a.F, H = a.H;
  const BnnChain ch = bnn_chain<HP>(a.K, H);
  const int j = ch.j;
  const float* th = a.theta + ch.c * a.ld;
  const int oB1 = H * F, oW2 = oB1 + H, oB2 = oW2 + 2 * H;
  BnnLane<FP> L;
#pragma unroll
  for (int f = 0; f < FP; ++f) L.w1[f] = (ch.on && f < F) ? th[j * F + f] : 0.f;
  L.b1 = ch.on ? th[oB1 + j] : 0.f;
  L.w2d = ch.on ? th[oW2 + H + j] - th[oW2 + j] : 0.f;
  const float b2d = ch.chain ? th[oB2 + 1] - th[oB2] : 0.f;
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

template <int HP, int FP> int bnn_launch_hf(const BnnArgs& a, bool predict, dim3 grid, dim3 block, hipStream_t s) {
  if (predict) {
    if (a.activation) bnn_predict_kernel<HP, FP, 1><<<grid, block, 0, s>>>(a);
    else bnn_predict_kernel<HP, FP, 0><<<grid, block, 0, s>>>(a);
  } else {
    if (a.activation) bnn_logp_grad_kernel<HP, FP, 1><<<grid, block, 0, s>>>(a);
    else bnn_logp_grad_kernel<HP, FP, 0><<<grid, block, 0, s>>>(a);
  }
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

template <int HP> int bnn_launch_h(const BnnArgs& a, bool predict, hipStream_t s) {
  constexpr int CPW = 64 / HP;
  const int waves = std::min(BNN_MAX_WAVES, (a.K + CPW - 1) / CPW), cpb = waves * CPW;
  const long blocks = (long)a.P * ((a.K + cpb - 1) / cpb);
  const dim3 grid((unsigned)blocks), block(64 * waves);
  if (a.F <= 4) return bnn_launch_hf<HP, 4>(a, predict, grid, block, s);
  if (a.F <= 8) return bnn_launch_hf<HP, 8>(a, predict, grid, block, s);
  return bnn_launch_hf<HP, 16>(a, predict, grid, block, s);
}

int bnn_launch(const BnnArgs& a, bool predict, hipStream_t s) {
  if (a.H <= 8) return bnn_launch_h<8>(a, predict, s);
  if (a.H <= 16) return bnn_launch_h<16>(a, predict, s);
  if (a.H <= 32) return bnn_launch_h<32>(a, predict, s);
  return bnn_launch_h<64>(a, predict, s);
}

}  // namespace

int launch_bnn_logp_grad(const BnnArgs& a, hipStream_t s) { return bnn_launch(a, false, s); }
int launch_bnn_predict(const BnnArgs& a, hipStream_t s) { return bnn_launch(a, true, s); }

}  // namespace pfn
