// Stochastic variational inference on the two-layer BNN of the BNN study (reference mcmc_svi_transformer_on_bayesian.py:211-246, `eval_svi`: pyro's
// AutoDiagonalNormal guide, Trace_ELBO(num_particles), Adam): ONE launch advances the guides of P problems by num_steps steps of
// (draw noise -> ELBO gradient -> Adam).  DESIGN.md section 17 has the mapping; include/pfn_hip.h the contract.
//
// Mapping: one block per problem, nothing crosses blocks.  Section 16's lane = hidden unit (bnn_device.h, whose header lists the pieces shared with the
// other two kernels): a group of Hp lanes holds one PARTICLE
// theta_k = loc + scale eps_k, 64 / Hp particles share a wave, up to four waves; K beyond the block's capacity runs in rounds.  The six state rows, scale
// and log scale stay in LDS for the whole launch, and so do the problem's data rows when they fit (else they are staged in section 16's 64-row chunks in
// every round).  Per step: (1) the lanes of a group draw their particle's noise, four normals per Philox block, into LDS; (2) every lane forms its own
// parameters and runs the row loop of pfn_bnn_logp_grad; (3) a lane adds grad U and grad U * eps of its parameters into running sums over the rounds,
// the sums are reduced over the groups of a wave by __shfl_xor (offsets Hp, 2 Hp, .. 32) and leave through LDS, one row per wave; (4) parameter i is
// updated by thread i mod blockDim, which adds the waves' rows in wave order and takes the Adam step.  The order of every sum depends on (H, F, K) only.
#include <algorithm>
#include "bnn_device.h"

namespace pfn {

struct BnnSviArgs {
  const float* x;        // [P,S,F]
  const float* y;        // [P,S]: class = y > 0.5
  const int32_t* n_of;   // [P] rows in use per problem (device; clamped to [0,S]); null = S
  float* state;          // [P,6,ld]: loc, u (scale = softplus(u)), m_loc, v_loc, m_u, v_u; columns >= D are never touched
  long ld;
  int P, S, F, H, activation, K;      // K particles per step
  long step0;
  int num_steps;
  float lr, beta1, beta2, eps;
  unsigned long long seed;
  const int64_t* problem_ids;   // [P] or null (the problem's index): the Philox stream
  float* loss;           // [P,num_steps] or null
};

namespace {

constexpr long SVI_ROWS_BUDGET = 48 * 1024;      // bytes of x / y rows kept resident; the rest of the block's LDS reaches 98 KB at H 64, F 16, four waves

struct SviLaunch {
  int waves, Dp, cap, resident;
};

PFN_DEV float svi_softplus(float u) { return fmaxf(u, 0.f) + log1pf(expf(-fabsf(u))); }

template <int HP, int FP, int ACT> __global__ void __launch_bounds__(64 * BNN_MAX_WAVES, 2) bnn_svi_kernel(BnnSviArgs a, SviLaunch c) {
  extern __shared__ __attribute__((aligned(16))) float svi_lds[];
  constexpr int RR = FP == 16 ? 2 : BNN_ROWS;      // rows in flight: four of 16 columns beside the particle's parameters do not fit 256 registers
  constexpr int CPW = 64 / HP, NS = FP + 5;      // a lane's parameters: W1[j,:] (FP), b1[j], W2[0,j], W2[1,j], and b2[0], b2[1] (owned by j = 0)
  const int F = a.F, H = a.H, K = a.K, D = H * (F + 3) + 2, Dp = c.Dp;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cpb = waves * CPW, rounds = (K + cpb - 1) / cpb;
  const int grp = lane / HP, j = lane & (HP - 1), kk = wave * CPW + grp;
  const int p = blockIdx.x;
  float* st = svi_lds;                   // [6][Dp]: loc, u, m_loc, v_loc, m_u, v_u
  float* sc = st + 6 * Dp;               // [2][Dp]: scale = softplus(u), log scale
  float* ep = sc + 2 * Dp;               // [cpb][Dp]: the noise of the round's particles
  float* gs = ep + cpb * Dp;             // [waves][2][Dp]: sum over a wave's particles of grad U and of grad U * eps
  float* lw = gs + waves * 2 * Dp;       // [4]: sum over a wave's particles of the loss
  float* xs = lw + 4;                    // [cap][FP]
  float* ys = xs + c.cap * FP;           // [cap]
  const unsigned long long q = a.problem_ids ? (unsigned long long)a.problem_ids[p] : (unsigned long long)p;
  const int n = bnn_n_rows(a.n_of, p, a.S);
  const float* xp = a.x + (long)p * a.S * F;
  const float* yp = a.y + (long)p * a.S;
  float* sp = a.state + (long)p * 6 * a.ld;

  for (int idx = threadIdx.x; idx < 6 * D; idx += blockDim.x) {
    const int r = idx / D, i = idx - r * D;
    st[r * Dp + i] = sp[r * a.ld + i];
  }
  if (c.resident) bnn_stage_all<FP>(xs, ys, xp, yp, n, F);
  __syncthreads();
  for (int i = threadIdx.x; i < D; i += blockDim.x) {
    const float s = svi_softplus(st[Dp + i]);
    sc[i] = s;
    sc[Dp + i] = logf(s);
  }
  __syncthreads();

  const BnnSlots<FP> sl(F, H, j);
  const float inv_k = 1.f / (float)K;

  for (int it = 0; it < a.num_steps; ++it) {
    const unsigned long long t = (unsigned long long)a.step0 + it;
    float al = 0.f;      // the loss of the lane's particles over the rounds

    for (int rd = 0; rd < rounds; ++rd) {
      const int k0 = rd * cpb + wave * CPW, k = k0 + grp;
      const bool wave_on = k0 < K, part = k < K;      // wave_on is wave-uniform
      if (part) {
        for (int b = j; 4 * b < D; b += HP) {      // 4 b + 3 < Dp: the row's padding takes the block's tail
          float z[4];
          normal4(philox4x32_10(((t * (unsigned long long)K + (unsigned long long)k) << 10) | (unsigned)b, q, a.seed), z);
          *reinterpret_cast<f32x4*>(ep + kk * Dp + 4 * b) = f32x4{z[0], z[1], z[2], z[3]};
        }
      }
      __syncthreads();
      float th[NS], b2d;
      const float* e = ep + kk * Dp;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const bool on = part && sl.held(s);
        const int i = on ? sl.index(s) : 0;
        th[s] = on ? __builtin_fmaf(sc[i], e[i], st[i]) : 0.f;
      }
      const BnnLane<FP> L = bnn_lane<FP>(th, b2d);
      BnnSums<FP> sm;
      sm.clear();
      bnn_data_rows<HP, FP, ACT, RR>(L, b2d, xs, ys, xp, yp, n, F, c.resident, wave_on, sm);
      if (wave_on) {
        float g[NS];      // grad U(theta_k) of the lane's parameters, prior included
#pragma unroll
        for (int f = 0; f < FP; ++f) g[f] = sm.dw1[f] + th[f];
        g[FP] = sm.db1 + th[FP];
        g[FP + 1] = th[FP + 1] - sm.A;
        g[FP + 2] = th[FP + 2] + sm.A;
        g[FP + 3] = th[FP + 3] - sm.G;
        g[FP + 4] = th[FP + 4] + sm.G;
        float ql = 0.f;      // the lane's share of |theta|^2 / 2 - |eps|^2 / 2 - sum log scale; (D / 2) log 2 pi of U and of the entropy cancel
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const bool on = part && sl.owned(s);
          const int i = on ? sl.index(s) : 0;
          const float ez = e[i];
          ql += on ? 0.5f * (th[s] * th[s] - ez * ez) - sc[Dp + i] : 0.f;
          float sg = on ? g[s] : 0.f, sge = on ? g[s] * ez : 0.f;
#pragma unroll
          for (int o = HP; o < 64; o <<= 1) {      // over the groups of the wave, then onto the running sum of the rounds
            sg += __shfl_xor(sg, o, 64);
            sge += __shfl_xor(sge, o, 64);
          }
          if (lane < HP && on) {
            float* row = gs + (wave * 2) * Dp + i;
            row[0] = rd ? row[0] + sg : sg;
            row[Dp] = rd ? row[Dp] + sge : sge;
          }
        }
        ql = bnn_group_sum<HP>(ql) + sm.U;
        al += part ? ql : 0.f;
      }
    }
#pragma unroll
    for (int o = HP; o < 64; o <<= 1) al += __shfl_xor(al, o, 64);
    if (lane == 0) lw[wave] = al;
    __syncthreads();
    const BnnAdam ad = bnn_adam_at(a.lr, a.beta1, a.beta2, a.eps, t);      // Adam on loc and on u
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
      float sg = 0.f, sge = 0.f;
      for (int w = 0; w < waves; ++w) sg += gs[(w * 2) * Dp + i], sge += gs[(w * 2 + 1) * Dp + i];
      const float u = st[Dp + i];
      const float g_loc = sg * inv_k;
      const float g_scale = sge * inv_k - 1.f / sc[i];
      const float eu = expf(-fabsf(u));
      const float g_u = g_scale * bnn_sigmoid(u, eu);
      const BnnAdamOut nl = bnn_adam(st[i], st[2 * Dp + i], st[3 * Dp + i], g_loc, ad), nu = bnn_adam(u, st[4 * Dp + i], st[5 * Dp + i], g_u, ad);
      st[i] = nl.p, st[Dp + i] = nu.p;
      st[2 * Dp + i] = nl.m, st[3 * Dp + i] = nl.v, st[4 * Dp + i] = nu.m, st[5 * Dp + i] = nu.v;
      const float s = svi_softplus(nu.p);
      sc[i] = s;
      sc[Dp + i] = logf(s);
    }
    if (threadIdx.x == 0 && a.loss) {
      float l = 0.f;
      for (int w = 0; w < waves; ++w) l += lw[w];
      a.loss[(long)p * a.num_steps + it] = l * inv_k;
    }
    __syncthreads();
  }
  for (int idx = threadIdx.x; idx < 6 * D; idx += blockDim.x) {
    const int r = idx / D, i = idx - r * D;
    sp[r * a.ld + i] = st[r * Dp + i];
  }
}

int launch_bnn_svi_steps(const BnnSviArgs& a, hipStream_t s) {
  return bnn_dispatch(a.H, a.F, a.activation, [&](auto hp, auto fp, auto act) {
    constexpr int HP = decltype(hp)::value, FP = decltype(fp)::value, ACT = decltype(act)::value, CPW = 64 / HP;
    SviLaunch c;
    c.waves = std::min(BNN_MAX_WAVES, (a.K + CPW - 1) / CPW);
    c.Dp = (a.H * (a.F + 3) + 2 + 3) & ~3;
    c.resident = (long)a.S * (FP + 1) * 4 <= SVI_ROWS_BUDGET;
    c.cap = c.resident ? a.S : BNN_CHUNK;
    const size_t bytes = ((size_t)(8 + c.waves * CPW + 2 * c.waves) * c.Dp + 4 + (size_t)c.cap * (FP + 1)) * sizeof(float);
    static_assert((size_t)(8 + BNN_MAX_WAVES * CPW + 2 * BNN_MAX_WAVES) * (HP * (FP + 3) + 4) * 4 + 16 + SVI_ROWS_BUDGET + BNN_CHUNK * (FP + 1) * 4 <= 160 * 1024, "bnn_svi: LDS");
    static LdsAllowance allow;      // one per instantiation
    return launch_lds(bnn_svi_kernel<HP, FP, ACT>, allow, dim3((unsigned)a.P), dim3(64 * c.waves), bytes, s, a, c);
  });
}

}  // namespace
}  // namespace pfn

using namespace pfn;

extern "C" int pfn_bnn_svi_steps(const float* x, const float* y, const int32_t* n_of, float* state, int64_t ld, int P, int S, int F, int H, int activation,
                                 int num_particles, int64_t step0, int num_steps, float lr, float beta1, float beta2, float eps, uint64_t seed,
                                 const int64_t* problem_ids, float* loss, void* stream) {
  if (int rc = bnn_limits(F, H, activation)) return rc;
  if (int rc = bnn_steps_check("bnn_svi_steps", P, S, F, H, ld, step0, num_steps, x, y, state, lr, beta1, beta2, eps)) return rc;
  if (num_particles < 1) return fail(PFN_ERR_ARGUMENT, "bad bnn_svi_steps arguments (num_particles %d >= 1)", num_particles);
  if (step0 > (int64_t)1 << 40 || (step0 + num_steps + 1) * (int64_t)num_particles >= (int64_t)1 << 53)
    return fail(PFN_ERR_ARGUMENT, "step0 %lld must not exceed 2^40 and (step0 + num_steps + 1) num_particles must stay below 2^53 (the Philox counter of a particle's noise)", (long long)step0);
  if (num_steps == 0) return PFN_OK;
  BnnSviArgs a{};
  a.x = x; a.y = y; a.n_of = n_of; a.state = state; a.ld = ld; a.P = P; a.S = S; a.F = F; a.H = H; a.activation = activation; a.K = num_particles; a.step0 = step0;
  a.num_steps = num_steps; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.seed = seed; a.problem_ids = problem_ids; a.loss = loss;
  PFN_TRY(launch_bnn_svi_steps(a, (hipStream_t)stream));
  return PFN_OK;
}
