// Stein variational gradient descent on the two-layer BNN of the BNN study (reference mcmc_svi_transformer_on_bayesian.py:211-246, `eval_svi(svgd=True)`: pyro's
// SVGD(model, RBFSteinKernel(), adam, num_particles=50)): ONE launch advances the N particles of P problems by num_steps steps of
// (potential gradient -> per-coordinate median bandwidth -> Stein direction -> Adam).  DESIGN.md section 18 has the mapping; include/pfn_hip.h the contract.
//
// Mapping: one block of eight waves per problem (two per SIMD: a wave alone on its SIMD issues a vector instruction every four cycles, two share it at one
// every two, and each covers the other's LDS latency), nothing crosses blocks.
// Phase 1 is section 16's lane = hidden unit (bnn_device.h, whose header lists the pieces shared with the other two kernels): a group of Hp lanes holds one PARTICLE, 64 / Hp particles share a wave, N beyond the block's
// capacity runs in rounds; nothing is reduced over particles, each group writes grad U of its particle.
// Phases 2-4 are independent per coordinate: a WAVE takes a coordinate and lane n is particle n (N <= 64), four coordinates at a time so that their dependent
// LDS reads overlap.  (2) the lanes rank the coordinate's N values (ties by index) and scatter them sorted into the wave's scratch; the k-th smallest
// |x_i - x_j| over i < j is selected by bisection on its f32 bit pattern, one bit per iteration, 31 iterations: lane i counts the j > i with
// sorted_j - sorted_i < t by a six-step descent over the sorted values, and the wave's count is the sum over the steps of step size x popcount(ballot).
// (3) lane n sums the Stein direction over m = 0 .. N - 1 in that order (broadcast reads).  (4) lane n takes the Adam step of x_nd.  Every order
// depends on (H, F, N) only.
// Regimes: when particles, gradients and both moments fit the state budget they stay in LDS for the whole launch; otherwise the state stays in the
// caller's buffer and the gradients in the workspace (block-private, L2-resident), and phases 2-4 walk over them in tiles of 64 coordinate columns.
#include <algorithm>
#include <cmath>
#include "bnn_device.h"

namespace pfn {

struct BnnSvgdArgs {
  const float* x;        // [P,S,F]
  const float* y;        // [P,S]: class = y > 0.5
  const int32_t* n_of;   // [P] rows in use per problem (device; clamped to [0,S]); null = S
  float* state;          // [P,3,N,ld]: particles, m, v; columns >= D are never touched
  long ld;
  int P, S, F, H, activation, N;      // N particles per problem
  long step0;
  int num_steps;
  float lr, beta1, beta2, eps, bandwidth_factor;
  float* grads;          // [P,N,D] (the workspace) when the state is not resident in LDS, else unused
  float* potential;      // [P,num_steps] or null
  float* bandwidth;      // [P,ld] or null
};
// particles, gradients and both Adam moments ([4][N][D | 1] f32) stay in LDS for the whole launch when they fit this many bytes; otherwise the state stays in
// the caller's buffer, the gradients go through the workspace and LDS holds a tile of 64 coordinate columns
constexpr long BNN_SVGD_STATE_BUDGET = 66560;
inline bool bnn_svgd_resident(int N, int D) { return 16L * N * (D | 1) <= BNN_SVGD_STATE_BUDGET; }
inline int64_t bnn_svgd_workspace_bytes(int P, int N, int D) { return bnn_svgd_resident(N, D) ? 0 : (int64_t)P * N * D * 4; }

namespace {

constexpr long SVGD_ROWS_BUDGET = 48 * 1024;      // bytes of x / y rows kept resident (else section 16's 64-row chunks in every round)
constexpr int SVGD_TILE = 64;                     // coordinate columns per tile of the tiled regime
constexpr int SVGD_CI = 4;                        // coordinates a wave works on at a time
constexpr int SVGD_WAVES = 8;                     // waves of a block, in every phase
static_assert(16L * PFN_BNN_SVGD_MAX_PARTICLES * (SVGD_TILE + 1) <= BNN_SVGD_STATE_BUDGET, "bnn_svgd: a tile of 64 particles fits the state budget");

struct SvgdLaunch {
  int resident, LW, rows_resident, cap;      // LW: floats per particle row of the four LDS arrays (odd: lane = particle reads are conflict-free)
  float log_n1;                              // log(N + 1)
};

template <int HP, int FP, int ACT> __global__ void __launch_bounds__(64 * SVGD_WAVES, 2) bnn_svgd_kernel(BnnSvgdArgs a, SvgdLaunch c) {
  extern __shared__ __attribute__((aligned(16))) float svgd_lds[];
  constexpr int RR = FP == 16 ? 2 : BNN_ROWS;      // rows in flight: four of 16 columns beside the particle's parameters do not fit 256 registers
  constexpr int CPW = 64 / HP, NS = FP + 5, WAVES = SVGD_WAVES, CI = SVGD_CI;
  const int F = a.F, H = a.H, N = a.N, D = H * (F + 3) + 2, LW = c.LW;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cpb = WAVES * CPW, rounds = (N + cpb - 1) / cpb;
  const int grp = lane / HP, j = lane & (HP - 1);
  const int p = blockIdx.x;
  float* xs = svgd_lds;                       // [cap][FP]
  float* ys = xs + c.cap * FP;                // [cap], padded to a multiple of four
  float* X = ys + ((c.cap + 3) & ~3);         // [N][LW]: the particles (resident) or a tile of their columns
  float* G = X + N * LW;                      // [N][LW]: grad U
  float* M = G + N * LW;                      // [N][LW]: Adam's m
  float* V = M + N * LW;                      // [N][LW]: Adam's v
  float* srt = V + N * LW;                    // [WAVES][CI][64]: a coordinate's values, sorted
  float* up = srt + WAVES * CI * 64;          // [64]: U(x_n)
  const int n = bnn_n_rows(a.n_of, p, a.S);
  const float* xp = a.x + (long)p * a.S * F;
  const float* yp = a.y + (long)p * a.S;
  float* sp = a.state + (long)p * 3 * N * a.ld;      // rows [0, N) particles, [N, 2N) m, [2N, 3N) v
  float* gw = a.grads ? a.grads + (long)p * N * D : nullptr;      // [N][D], the tiled regime

  if (c.resident) {
    for (int idx = threadIdx.x; idx < N * D; idx += blockDim.x) {
      const int r = idx / D, i = idx - r * D;
      const float* src = sp + (long)r * a.ld + i;
      X[r * LW + i] = src[0];
      M[r * LW + i] = src[(long)N * a.ld];
      V[r * LW + i] = src[2L * N * a.ld];
    }
  }
  if (c.rows_resident) bnn_stage_all<FP>(xs, ys, xp, yp, n, F);
  __syncthreads();

  const BnnSlots<FP> sl(F, H, j);
  const unsigned kth = (unsigned)((N * (N - 1) / 2 - 1) / 2);      // torch.median: the lower middle of the N (N - 1) / 2 pairs, counted from 0
  const float inv_n = 1.f / (float)N;

  for (int it = 0; it < a.num_steps; ++it) {
    const unsigned long long t = (unsigned long long)a.step0 + it;

    // ---- phase 1: grad U and U of every particle ----
    for (int rd = 0; rd < rounds; ++rd) {
      const int k0 = rd * cpb + wave * CPW, k = k0 + grp;
      const bool wave_on = k0 < N, part = k < N;      // wave_on is wave-uniform
      const int kc = part ? k : 0;
      float th[NS], b2d;
      if (c.resident) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const bool on = part && sl.held(s);
          th[s] = on ? X[kc * LW + sl.index(s)] : 0.f;
        }
      } else {
        const float* row = sp + (long)kc * a.ld;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const bool on = part && sl.held(s);
          th[s] = on ? row[sl.index(s)] : 0.f;
        }
      }
      const BnnLane<FP> L = bnn_lane<FP>(th, b2d);
      BnnSums<FP> sm;
      sm.clear();
      bnn_data_rows<HP, FP, ACT, RR>(L, b2d, xs, ys, xp, yp, n, F, c.rows_resident, wave_on, sm);
      if (wave_on) {
        float g[NS];      // grad U(x_k) of the lane's parameters, prior included
#pragma unroll
        for (int f = 0; f < FP; ++f) g[f] = sm.dw1[f] + th[f];
        g[FP] = sm.db1 + th[FP];
        g[FP + 1] = th[FP + 1] - sm.A;
        g[FP + 2] = th[FP + 2] + sm.A;
        g[FP + 3] = th[FP + 3] - sm.G;
        g[FP + 4] = th[FP + 4] + sm.G;
        float ql = 0.f;      // the lane's share of |theta|^2 / 2
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const bool on = part && sl.owned(s);
          ql += on ? 0.5f * th[s] * th[s] : 0.f;
          if (on) {
            if (c.resident) G[kc * LW + sl.index(s)] = g[s];
            else gw[(long)kc * D + sl.index(s)] = g[s];
          }
        }
        ql = bnn_group_sum<HP>(ql) + sm.U + (float)D * HALF_LOG_2PI;
        if (part && j == 0) up[k] = ql;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0 && a.potential) {
      float u = 0.f;
      for (int k = 0; k < N; ++k) u += up[k];
      a.potential[(long)p * a.num_steps + it] = u * inv_n;
    }

    // ---- phases 2-4, coordinate by coordinate: bandwidth, Stein direction, Adam ----
    const BnnAdam ad = bnn_adam_at(a.lr, a.beta1, a.beta2, a.eps, t);
    const bool last = it == a.num_steps - 1;
    const int ntiles = c.resident ? 1 : (D + SVGD_TILE - 1) / SVGD_TILE;
    for (int tile = 0; tile < ntiles; ++tile) {
      const int c0 = tile * SVGD_TILE, cw = c.resident ? D : min(SVGD_TILE, D - c0);
      if (!c.resident) {
        for (int idx = threadIdx.x; idx < N * cw; idx += blockDim.x) {
          const int r = idx / cw, q = idx - r * cw;
          const float* src = sp + (long)r * a.ld + c0 + q;
          X[r * LW + q] = src[0];
          M[r * LW + q] = src[(long)N * a.ld];
          V[r * LW + q] = src[2L * N * a.ld];
          G[r * LW + q] = gw[(long)r * D + c0 + q];
        }
        __syncthreads();
      }
      for (int cb0 = 0; cb0 < cw; cb0 += WAVES * CI) {      // the trip count is the block's: the barrier below is reached by every wave
        const int cb = cb0 + wave * CI;
        const bool active = cb < cw;      // wave-uniform
        const int nl = lane < N ? lane : 0;
        float* sw = srt + wave * CI * 64;
        int dc[CI];
        float xn[CI];
#pragma unroll
        for (int q = 0; q < CI; ++q) dc[q] = min(cb + q, cw - 1);      // a coordinate beyond the tile repeats the last one and stores nothing
        if (active) {
          int rank[CI];
#pragma unroll
          for (int q = 0; q < CI; ++q) xn[q] = X[nl * LW + dc[q]], rank[q] = 0;
          for (int m = 0; m < N; ++m) {
#pragma unroll
            for (int q = 0; q < CI; ++q) {
              const float xm = X[m * LW + dc[q]];
              rank[q] += (xm < xn[q] || (xm == xn[q] && m < lane)) ? 1 : 0;
            }
          }
          if (lane < N) {
#pragma unroll
            for (int q = 0; q < CI; ++q) sw[q * 64 + rank[q]] = xn[q];      // rank <= N - 1 whatever the values are
          }
        }
        __syncthreads();
        if (active) {
          // (2) the k-th smallest |x_i - x_j|, i < j: the largest t with #{sorted_j - sorted_i < t} <= k, built bit by bit from the top (non-negative
          // floats order as their bit patterns); NaN values count nothing and leave t = NaN
          float si[CI];
          unsigned ans[CI];
#pragma unroll
          for (int q = 0; q < CI; ++q) si[q] = lane < N ? sw[q * 64 + lane] : 0.f, ans[q] = 0u;
          for (int bit = 30; bit >= 0; --bit) {
            float tc[CI];
            int pos[CI];
            unsigned tot[CI];      // the wave's count: a lane's count is the sum of the steps it took, so a step adds its size times the lanes that took it
#pragma unroll
            for (int q = 0; q < CI; ++q) tc[q] = __uint_as_float(ans[q] | (1u << bit)), pos[q] = lane, tot[q] = 0u;
#pragma unroll
            for (int st = 32; st; st >>= 1) {
#pragma unroll
              for (int q = 0; q < CI; ++q) {
                // no branch: the four reads of a step are in flight together (a slot beyond N is read, inside the row, and not used)
                const int at = pos[q] + st;
                const float v = sw[q * 64 + min(at, 63)];
                const bool ok = (at < N) & (v - si[q] < tc[q]);
                pos[q] = ok ? at : pos[q];
                tot[q] += (unsigned)__popcll(__ballot(ok)) * (unsigned)st;
              }
            }
#pragma unroll
            for (int q = 0; q < CI; ++q) {
              if (tot[q] <= kth) ans[q] |= 1u << bit;
            }
          }
          // (3) the Stein direction of particle `lane`, summed over m in index order
          float hd[CI], inv[CI], acc[CI];
#pragma unroll
          for (int q = 0; q < CI; ++q) {
            const float med = __uint_as_float(ans[q]);
            hd[q] = a.bandwidth_factor * (med * med) / c.log_n1;
            inv[q] = 1.f / hd[q];
            acc[q] = 0.f;
          }
          for (int m = 0; m < N; ++m) {
#pragma unroll
            for (int q = 0; q < CI; ++q) {
              const float xm = X[m * LW + dc[q]], gm = G[m * LW + dc[q]];
              const float df = xn[q] - xm;
              const float kk = __expf(-(df * df) * inv[q]);
              acc[q] = __builtin_fmaf(kk, gm - 2.f * df * inv[q], acc[q]);
            }
          }
          // (4) Adam
#pragma unroll
          for (int q = 0; q < CI; ++q) {
            if (cb + q < cw) {
              if (lane < N) {
                const int o = lane * LW + dc[q];
                const BnnAdamOut up1 = bnn_adam(xn[q], M[o], V[o], acc[q] * inv_n, ad);
                X[o] = up1.p, M[o] = up1.m, V[o] = up1.v;
              }
              if (last && a.bandwidth && lane == 0) a.bandwidth[(long)p * a.ld + c0 + dc[q]] = hd[q];
            }
          }
        }
      }
      if (!c.resident) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < N * cw; idx += blockDim.x) {
          const int r = idx / cw, q = idx - r * cw;
          float* dst = sp + (long)r * a.ld + c0 + q;
          dst[0] = X[r * LW + q];
          dst[(long)N * a.ld] = M[r * LW + q];
          dst[2L * N * a.ld] = V[r * LW + q];
        }
      }
      __syncthreads();
    }
  }
  if (c.resident) {
    for (int idx = threadIdx.x; idx < N * D; idx += blockDim.x) {
      const int r = idx / D, i = idx - r * D;
      float* dst = sp + (long)r * a.ld + i;
      dst[0] = X[r * LW + i];
      dst[(long)N * a.ld] = M[r * LW + i];
      dst[2L * N * a.ld] = V[r * LW + i];
    }
  }
}

int launch_bnn_svgd_steps(const BnnSvgdArgs& a, hipStream_t s) {
  return bnn_dispatch(a.H, a.F, a.activation, [&](auto hp, auto fp, auto act) {
    constexpr int HP = decltype(hp)::value, FP = decltype(fp)::value, ACT = decltype(act)::value;
    const int D = a.H * (a.F + 3) + 2;
    SvgdLaunch c;
    c.resident = bnn_svgd_resident(a.N, D);      // the rule pfn_bnn_svgd_workspace_bytes sizes the workspace by
    c.LW = c.resident ? (D | 1) : SVGD_TILE + 1;
    c.rows_resident = (long)a.S * (FP + 1) * 4 <= SVGD_ROWS_BUDGET;
    c.cap = c.rows_resident ? a.S : BNN_CHUNK;
    c.log_n1 = (float)std::log((double)(a.N + 1));
    const size_t bytes = ((size_t)c.cap * FP + ((c.cap + 3) & ~3) + (size_t)4 * a.N * c.LW + SVGD_WAVES * SVGD_CI * 64 + 64) * sizeof(float);
    static_assert(BNN_SVGD_STATE_BUDGET + SVGD_ROWS_BUDGET + 16 + BNN_CHUNK * (FP + 1) * 4 + (SVGD_WAVES * SVGD_CI * 64 + 64) * 4 <= 160 * 1024, "bnn_svgd: LDS");
    static LdsAllowance allow;      // one per instantiation
    return launch_lds(bnn_svgd_kernel<HP, FP, ACT>, allow, dim3((unsigned)a.P), dim3(64 * SVGD_WAVES), bytes, s, a, c);
  });
}

int bnn_svgd_limits(int F, int H, int activation, int N) {      // what the kernel is built for: nothing here touches a pointer or HIP
  if (int rc = bnn_limits(F, H, activation)) return rc;
  if (N < 2 || N > PFN_BNN_SVGD_MAX_PARTICLES)
    return fail(PFN_ERR_UNSUPPORTED, "num_particles %d outside 2 .. %d (lane = particle in the Stein step; the median needs a pair)", N, PFN_BNN_SVGD_MAX_PARTICLES);
  return PFN_OK;
}

}  // namespace
}  // namespace pfn

using namespace pfn;

extern "C" {
int64_t pfn_bnn_svgd_workspace_bytes(int P, int num_particles, int F, int H) {
  if (P < 1 || bnn_svgd_limits(F, H, 0, num_particles)) return -1;
  return bnn_svgd_workspace_bytes(P, num_particles, H * (F + 3) + 2);
}
int pfn_bnn_svgd_steps(const float* x, const float* y, const int32_t* n_of, float* state, int64_t ld, int P, int S, int F, int H, int activation, int num_particles,
                       int64_t step0, int num_steps, float lr, float beta1, float beta2, float eps, float bandwidth_factor, void* workspace,
                       int64_t workspace_bytes, float* potential, float* bandwidth, void* stream) {
  if (int rc = bnn_svgd_limits(F, H, activation, num_particles)) return rc;
  if (int rc = bnn_steps_check("bnn_svgd_steps", P, S, F, H, ld, step0, num_steps, x, y, state, lr, beta1, beta2, eps)) return rc;
  if (!(lr <= 3.4e38f) || !(bandwidth_factor > 0.f)) return fail(PFN_ERR_ARGUMENT, "bad bnn_svgd_steps arguments (lr %g finite, bandwidth_factor %g > 0)", lr, bandwidth_factor);
  const int D = H * (F + 3) + 2;
  const int64_t need = bnn_svgd_workspace_bytes(P, num_particles, D);
  if (workspace_bytes < need || (need > 0 && !workspace))
    return fail(PFN_ERR_ARGUMENT, "workspace_bytes %lld < pfn_bnn_svgd_workspace_bytes = %lld (or a NULL workspace)", (long long)workspace_bytes, (long long)need);
  if (num_steps == 0) return PFN_OK;
  BnnSvgdArgs a{};
  a.x = x; a.y = y; a.n_of = n_of; a.state = state; a.ld = ld; a.P = P; a.S = S; a.F = F; a.H = H; a.activation = activation; a.N = num_particles; a.step0 = step0;
  a.num_steps = num_steps; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.bandwidth_factor = bandwidth_factor;
  a.grads = need > 0 ? (float*)workspace : nullptr; a.potential = potential; a.bandwidth = bandwidth;
  PFN_TRY(launch_bnn_svgd_steps(a, (hipStream_t)stream));
  return PFN_OK;
}
}  // extern "C"
