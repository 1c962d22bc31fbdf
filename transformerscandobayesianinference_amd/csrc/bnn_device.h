// Device functions shared by the kernels of the two-layer BNN (bnn_mcmc.hip: potential / gradient / predictive of NUTS chains; bnn_svi.hip: the SVI step
// loop): the lane's registers, the forward of one hidden unit, the staging of data rows in LDS and the per-row step of the potential and its gradient.
// Mapping: lane = hidden unit, Hp = H rounded up to 8 / 16 / 32 / 64 lanes form a group that holds one parameter vector; a lane
// keeps W1[j,:], b1[j] and W2[1,j] - W2[0,j] in registers and accumulates its own part of the gradient there.  Only ONE number per data row is reduced over
// the Hp lanes of a group (the logit difference o_1 - o_0), with a __shfl_xor butterfly in a fixed order (offsets 1, 2, .. Hp/2).
#pragma once
#include "pfn_device.h"

namespace pfn {

namespace {

constexpr int BNN_CHUNK = 64;      // rows of x / y staged per pass
constexpr int BNN_ROWS = 4;        // rows in flight (independent butterflies)
constexpr int BNN_MAX_WAVES = 4;
constexpr float HALF_LOG_2PI = 0.91893853320467274178f;

template <int FP> struct BnnLane {
  float w1[FP];      // W1[j, :], zero beyond F
  float b1, w2d;     // b1[j], W2[1,j] - W2[0,j]
};

// what a lane accumulates over the data rows: dW1[j,:], db1[j], A = sum_i g_i a_j, G = sum_i g_i, U = sum_i softplus
template <int FP> struct BnnSums {
  float dw1[FP], db1, A, G, U;
  PFN_DEV void clear() {
#pragma unroll
    for (int f = 0; f < FP; ++f) dw1[f] = 0.f;
    db1 = 0.f, A = 0.f, G = 0.f, U = 0.f;
  }
};

template <int HP> PFN_DEV float bnn_group_sum(float v) {
#pragma unroll
  for (int o = 1; o < HP; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the forward device function of every entry: a_j = act(b1[j] + W1[j,:] . x) for the row at `xr` (LDS, Fp floats, 16-byte aligned)
template <int FP, int ACT> PFN_DEV float bnn_hidden(const BnnLane<FP>& L, const float* xr) {
  float h = L.b1;
#pragma unroll
  for (int q = 0; q < FP / 4; ++q) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(xr + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) h = __builtin_fmaf(L.w1[4 * q + e], v[e], h);
  }
  return ACT ? tanhf(h) : h;
}

// sigmoid(z) from e = exp(-|z|): no overflow, no cancellation on either side
PFN_DEV float bnn_sigmoid(float z, float e) { return (z >= 0.f ? 1.f : e) / (1.f + e); }

// rows [r0, r0 + rows) of src[p] ([*, F] row-major) into xs [cap, FP], zero padded in both directions; nothing beyond the last row is read
template <int FP> PFN_DEV void bnn_stage(float* xs, const float* src_p, int r0, int rows, int F, int cap = BNN_CHUNK) {
  for (int idx = threadIdx.x; idx < cap * FP; idx += blockDim.x) {
    const int r = idx / FP, f = idx % FP;
    xs[idx] = (r < rows && f < F) ? src_p[(long)(r0 + r) * F + f] : 0.f;
  }
}

// the row step: rows r .. r + RR - 1 of the staged chunk (xs [*, FP], ys [*] in {0, 1}) added to the lane's sums; b2d = b2[1] - b2[0].  All 64 lanes of
// the wave must be here (the butterflies).
template <int HP, int FP, int ACT, int RR> PFN_DEV void bnn_row_step(const BnnLane<FP>& L, float b2d, const float* xs, const float* ys, int r, BnnSums<FP>& s) {
  float av[RR], pv[RR];
#pragma unroll
  for (int q = 0; q < RR; ++q) {
    av[q] = bnn_hidden<FP, ACT>(L, xs + (r + q) * FP);
    pv[q] = L.w2d * av[q];
  }
#pragma unroll
  for (int o = 1; o < HP; o <<= 1) {
#pragma unroll
    for (int q = 0; q < RR; ++q) pv[q] += __shfl_xor(pv[q], o, 64);
  }
#pragma unroll
  for (int q = 0; q < RR; ++q) {
    const float d = pv[q] + b2d;      // o_1 - o_0
    const bool y1 = ys[r + q] > 0.5f;
    const float z = y1 ? -d : d;      // -log softmax(o)[y] = softplus(z)
    const float e = expf(-fabsf(z));
    s.U += fmaxf(z, 0.f) + log1pf(e);
    const float sg = bnn_sigmoid(z, e);
    const float g = y1 ? -sg : sg;      // d softplus(z) / d d
    s.G += g;
    s.A = __builtin_fmaf(g, av[q], s.A);
    const float dh = g * L.w2d * (ACT ? 1.f - av[q] * av[q] : 1.f);
    s.db1 += dh;
    const float* xr = xs + (r + q) * FP;
#pragma unroll
    for (int f4 = 0; f4 < FP / 4; ++f4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xr + 4 * f4);
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) s.dw1[4 * f4 + e4] = __builtin_fmaf(dh, v[e4], s.dw1[4 * f4 + e4]);
    }
  }
}

// `rows` staged rows: groups of RR from row 0, the rest one by one
// (the sums take the rows in row order whatever RR is: it sets how many butterflies overlap, not a single bit of the result)
template <int HP, int FP, int ACT, int RR = BNN_ROWS> PFN_DEV void bnn_rows(const BnnLane<FP>& L, float b2d, const float* xs, const float* ys, int rows, BnnSums<FP>& s) {
  int r = 0;
  for (; r + RR <= rows; r += RR) bnn_row_step<HP, FP, ACT, RR>(L, b2d, xs, ys, r, s);
  for (; r < rows; ++r) bnn_row_step<HP, FP, ACT, 1>(L, b2d, xs, ys, r, s);
}

}  // namespace

}  // namespace pfn
