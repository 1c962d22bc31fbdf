// Device functions shared by the kernels of the two-layer BNN (bnn_mcmc.hip: potential / gradient / predictive of NUTS chains; bnn_svi.hip: the SVI step
// loop; bnn_svgd.hip: the SVGD step loop): the lane's registers, the forward of one hidden unit, the staging of data rows in LDS and the per-row step of the
// potential and its gradient.
// Mapping: lane = hidden unit, Hp = H rounded up to 8 / 16 / 32 / 64 lanes form a group that holds one parameter vector; a lane
// keeps W1[j,:], b1[j] and W2[1,j] - W2[0,j] in registers and accumulates its own part of the gradient there.  Only ONE number per data row is reduced over
// the Hp lanes of a group (the logit difference o_1 - o_0), with a __shfl_xor butterfly in a fixed order (offsets 1, 2, .. Hp/2).
// Also here, each written once ("The shared pieces", says why the rest is not): the slot map of a lane's Fp + 5 parameters (BnnSlots:
// SVI and SVGD, and the offsets of the NUTS and predict kernels), slots -> lane registers (bnn_lane: SVI, SVGD), the data-row loop over resident or chunked
// rows (bnn_data_rows: all three gradient kernels, the NUTS kernel never resident) with its staging prologue (bnn_stage_all: SVI, SVGD) and the n_of clamp
// (bnn_n_rows: all three), Adam's bias corrections and its update of one coordinate (bnn_ipow, bnn_adam_at, bnn_adam: SVI's loc and u, SVGD's particle
// coordinate) and, on the host, bnn_dispatch (the H / F / activation dispatch of all three files) and the argument checks that more than one of their entry
// points make (bnn_limits, bnn_batch, bnn_check, bnn_steps_check).  SVI and SVGD launch through launch_lds (pfn_host.h: the launch with more than 64 KB of LDS).
#pragma once
#include <type_traits>
#include "pfn_device.h"
#include "pfn_host.h"

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

// a lane's parameters, slot by slot: W1[j,:] (FP), b1[j], W2[0,j], W2[1,j], and b2[0], b2[1]; index(s) is the slot's place in the parameter vector
template <int FP> struct BnnSlots {
  static constexpr int NS = FP + 5;
  int F, H, j, oB1, oW2, oB2;
  bool unit;
  PFN_DEV BnnSlots(int F_, int H_, int j_) : F(F_), H(H_), j(j_), oB1(H_ * F_), oW2(oB1 + H_), oB2(oW2 + 2 * H_), unit(j_ < H_) {}
  PFN_DEV int index(int s) const { return s < FP ? j * F + s : s == FP ? oB1 + j : s == FP + 1 ? oW2 + j : s == FP + 2 ? oW2 + H + j : oB2 + (s - FP - 3); }
  PFN_DEV bool held(int s) const { return s < FP ? unit && s < F : s < FP + 3 ? unit : true; }      // the lane reads it (every lane of a group reads b2)
  PFN_DEV bool owned(int s) const { return s < FP + 3 ? held(s) : j == 0; }                        // the lane reports it
};

// the lane's registers from its slots; b2d = b2[1] - b2[0]
template <int FP> PFN_DEV BnnLane<FP> bnn_lane(const float (&th)[FP + 5], float& b2d) {
  BnnLane<FP> L;
#pragma unroll
  for (int f = 0; f < FP; ++f) L.w1[f] = th[f];
  L.b1 = th[FP];
  L.w2d = th[FP + 2] - th[FP + 1];
  b2d = th[FP + 4] - th[FP + 3];
  return L;
}

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

// the n_of clamp: the rows of problem p that count
PFN_DEV int bnn_n_rows(const int* n_of, int p, int S) { return n_of ? min(max(n_of[p], 0), S) : S; }

// the resident staging prologue: all n rows of the problem into xs [n, FP], their thresholded labels into ys [n]; the caller's barrier follows
template <int FP> PFN_DEV void bnn_stage_all(float* xs, float* ys, const float* xp, const float* yp, int n, int F) {
  bnn_stage<FP>(xs, xp, 0, n, F, n);
  for (int r = threadIdx.x; r < n; r += blockDim.x) ys[r] = yp[r] > 0.5f ? 1.f : 0.f;
}

// the data-row loop: the n rows of the problem (xp [n, F], yp [n]) added to the lane's sums.  Resident rows are in xs / ys already (bnn_stage_all); otherwise
// they pass through xs [BNN_CHUNK, FP] / ys [BNN_CHUNK] in chunks.  Every thread of the block must be here (the barriers); wave_on (wave-uniform: the
// butterflies run with all 64 lanes) gates the row steps only.
template <int HP, int FP, int ACT, int RR> PFN_DEV void bnn_data_rows(const BnnLane<FP>& L, float b2d, float* xs, float* ys, const float* xp, const float* yp, int n, int F, bool resident, bool wave_on, BnnSums<FP>& s) {
  if (resident) {
    if (wave_on) bnn_rows<HP, FP, ACT, RR>(L, b2d, xs, ys, n, s);
    return;
  }
  for (int r0 = 0; r0 < n; r0 += BNN_CHUNK) {
    const int rows = min(BNN_CHUNK, n - r0);
    __syncthreads();      // the previous chunk has been consumed
    bnn_stage<FP>(xs, xp, r0, rows, F);
    if (threadIdx.x < BNN_CHUNK) ys[threadIdx.x] = ((int)threadIdx.x < rows && yp[r0 + threadIdx.x] > 0.5f) ? 1.f : 0.f;
    __syncthreads();
    if (wave_on) bnn_rows<HP, FP, ACT, RR>(L, b2d, xs, ys, rows, s);
  }
}

// beta^t for an integer t by squaring, in f64: a function of (beta, t) alone, so a run split over launches takes the same bias corrections
PFN_DEV double bnn_ipow(double b, unsigned long long t) {
  double r = 1.;
  while (t) {
    if (t & 1) r *= b;
    b *= b;
    t >>= 1;
  }
  return r;
}

// Adam (torch.optim.Adam, no weight decay) at the absolute step index t: the optimizer's step count is t + 1
struct BnnAdam {
  float lr, beta1, beta2, eps, bc1, bc2;
};

PFN_DEV BnnAdam bnn_adam_at(float lr, float beta1, float beta2, float eps, unsigned long long t) {
  return {lr, beta1, beta2, eps, (float)(1. - bnn_ipow((double)beta1, t + 1)), (float)(1. - bnn_ipow((double)beta2, t + 1))};
}

struct BnnAdamOut {
  float p, m, v;
};

// one coordinate: parameter p, moments m and v, gradient g -> the three after the step, all by value
PFN_DEV BnnAdamOut bnn_adam(float p, float m, float v, float g, const BnnAdam h) {
  const float m1 = h.beta1 * m + (1.f - h.beta1) * g, v1 = h.beta2 * v + (1.f - h.beta2) * g * g;
  return {p - h.lr * (m1 / h.bc1) / (sqrtf(v1 / h.bc2) + h.eps), m1, v1};
}

// ---- host: one dispatch for the three files ----

template <int V> using BnnInt = std::integral_constant<int, V>;

// fn(Hp, Fp, activation) with the three as integral constants: Hp = H rounded up to 8 / 16 / 32 / 64, Fp = F rounded up to 4 / 8 / 16
template <class Fn> int bnn_dispatch(int H, int F, int activation, Fn&& fn) {
  auto act = [&](auto hp, auto fp) { return activation ? fn(hp, fp, BnnInt<1>{}) : fn(hp, fp, BnnInt<0>{}); };
  auto feat = [&](auto hp) { return F <= 4 ? act(hp, BnnInt<4>{}) : F <= 8 ? act(hp, BnnInt<8>{}) : act(hp, BnnInt<16>{}); };
  return H <= 8 ? feat(BnnInt<8>{}) : H <= 16 ? feat(BnnInt<16>{}) : H <= 32 ? feat(BnnInt<32>{}) : feat(BnnInt<64>{});
}

}  // namespace

// ---- host: the argument checks the entry points of the three files share ----

inline int bnn_limits(int F, int H, int activation) {      // what the kernels are built for; the checks come shapes first: nothing here touches a pointer or HIP
  if (F < 1 || F > 16) return fail(PFN_ERR_UNSUPPORTED, "F %d outside 1 .. 16 (a lane keeps its row of W1 in registers)", F);
  if (H < 1 || H > 64) return fail(PFN_ERR_UNSUPPORTED, "H %d outside 1 .. 64 (lane = hidden unit, one wave per chain at most)", H);
  if (activation < 0 || activation > 1) return fail(PFN_ERR_UNSUPPORTED, "activation %d (0 identity, 1 tanh)", activation);
  return PFN_OK;
}
inline int bnn_batch(int P, int K, int F, int H, int64_t ld) {      // K parameter vectors of D numbers, ld apart, for each of P problems
  if (P < 1 || K < 1 || (int64_t)P * K > 0x7fffffff) return fail(PFN_ERR_ARGUMENT, "P %d x K %d chains: need P >= 1, K >= 1, P K < 2^31", P, K);
  if (ld < (int64_t)H * (F + 3) + 2) return fail(PFN_ERR_ARGUMENT, "ld %lld < D = H (F + 3) + 2 = %d", (long long)ld, H * (F + 3) + 2);
  return PFN_OK;
}
inline int bnn_check(int P, int K, int F, int H, int activation, int64_t ld) {
  if (int rc = bnn_limits(F, H, activation)) return rc;
  return bnn_batch(P, K, F, H, ld);
}
// what the two step loops (SVI, SVGD) ask of their common arguments, after the limits: the problem and step counts and the pointers, ld, Adam's numbers
inline int bnn_steps_check(const char* fn, int P, int S, int F, int H, int64_t ld, int64_t step0, int num_steps, const void* x, const void* y, const void* state, float lr,
                           float beta1, float beta2, float eps) {
  if (P < 1 || S < 1 || step0 < 0 || num_steps < 0 || !x || !y || !state)
    return fail(PFN_ERR_ARGUMENT, "bad %s arguments (P %d >= 1, S %d >= 1, step0 %lld >= 0, num_steps %d >= 0, x, y, state not NULL)", fn, P, S, (long long)step0, num_steps);
  if (int rc = bnn_batch(P, 1, F, H, ld)) return rc;      // ld >= D
  if (!(lr >= 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f))
    return fail(PFN_ERR_ARGUMENT, "bad %s arguments (lr %g >= 0, beta1 %g and beta2 %g in [0, 1), eps %g >= 0)", fn, lr, beta1, beta2, eps);
  return PFN_OK;
}

}  // namespace pfn
