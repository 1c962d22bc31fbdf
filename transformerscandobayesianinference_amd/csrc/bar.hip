// Fused bar-distribution ("Riemann distribution") loss kernels (gfx950).
//
// Replaces BarDistribution.forward / FullSupportBarDistribution.forward and .mean
// (reference bar_distribution.py:19-38, 83-117): bucket search, log-softmax, width scaling,
// gather, half-normal tail correction -- one pass over each logits row, one wave per row.
// HBM-bound: algorithmic traffic is one read of the logits row (+ one write in the backward).
#include <algorithm>
#include <cstring>
#include "pfn_device.h"
#include "pfn_host.h"

namespace pfn {

struct BarArgs {
  const float* logits; long ld;  // [R, nbars]
  const float* y;                // [R]
  const float* borders;          // [nbars+1]
  float* nll;                    // [R]
  float* lse;                    // [R] saved for backward
  int* bucket;                   // [R] saved for backward
  long R; int nbars; int full_support;
  // backward
  const float* gout; float* dlogits;
  // mean
  float* mean_out;
};
// posterior summaries and draws (definitions: the header of that section below)
struct BarStatsArgs {
  const float* logits; long ld;  // [R, nbars]
  const float* borders;          // [nbars+1]
  long R; int nbars; int full_support;
  int K; int kinds[PFN_BAR_STATS_MAX];      // PFN_BAR_STAT_*
  int has_var, has_icdf;                    // any statistic of that kind among the K
  const float* args; long arg_ld;           // [K] (arg_ld == 0) or [R, arg_ld]
  float* out;                               // [R, K] (read by the backward)
  const float* gout; float* dlogits;        // backward: [R, K], [R, nbars] with row stride ld
  int n_samples; unsigned long long seed; float* samples;      // draws: [n_samples, R]
};

constexpr float HALFNORMAL_ICDF_HALF = 0.6744897501960817f;  // HalfNormal(1).icdf(0.5), bar_distribution.py:85-87
constexpr float LOG_2 = 0.6931471805599453f;
constexpr float HALF_LOG_2PI = 0.9189385332046727f;
constexpr float SQRT_2_OVER_PI = 0.7978845608028654f;

// torch.searchsorted(borders, y) - 1 with the two edge fixes of map_to_bucket_idx
// (bar_distribution.py:19-23): count of borders strictly below y, minus one.
PFN_DEV int bucket_of(const float* borders, int nbars, float y) {
  int lo = 0, hi = nbars + 1;  // first index with borders[idx] >= y
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (borders[mid] < y) lo = mid + 1; else hi = mid;
  }
  int t = lo - 1;
  if (y == borders[0]) t = 0;
  if (y == borders[nbars]) t = nbars - 1;
  return t;
}

PFN_DEV float halfnormal_logprob(float scale, float v) {
  const float z = v / scale;
  return LOG_2 - __logf(scale) - HALF_LOG_2PI - 0.5f * z * z;
}

PFN_DEV void row_max_sumexp(const float* row, int n, int lane, float& mx, float& se) {
  mx = -INFINITY;
  const bool vec = ((reinterpret_cast<uintptr_t>(row) & 15) == 0);
  const int n4 = vec ? (n / 4) : 0;
  for (int i = lane; i < n4; i += 64) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * i);
    mx = fmaxf(mx, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
  }
  for (int i = n4 * 4 + lane; i < n; i += 64) mx = fmaxf(mx, row[i]);
  mx = wave_max(mx);
  se = 0.f;
  for (int i = lane; i < n4; i += 64) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * i);
    se += __expf(v[0] - mx) + __expf(v[1] - mx) + __expf(v[2] - mx) + __expf(v[3] - mx);
  }
  for (int i = n4 * 4 + lane; i < n; i += 64) se += __expf(row[i] - mx);
  se = wave_sum(se);
}

__global__ __launch_bounds__(256) void bar_nll_fwd_kernel(BarArgs a) {
  const int lane = threadIdx.x & 63;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < a.R; r += (long)gridDim.x * 4) {
    const float* row = a.logits + r * a.ld;
    float mx, se;
    row_max_sumexp(row, a.nbars, lane, mx, se);
    if (lane == 0) {
      const float lse = mx + __logf(se);
      const float y = a.y[r];
      int t = bucket_of(a.borders, a.nbars, y);
      const bool in_support = (t >= 0 && t < a.nbars);
      t = max(0, min(a.nbars - 1, t));
      const float w = a.borders[t + 1] - a.borders[t];
      float lp = row[t] - lse - __logf(w);
      if (a.full_support) {
        if (t == 0) {
          const float w0 = a.borders[1] - a.borders[0];
          lp += halfnormal_logprob(w0 / HALFNORMAL_ICDF_HALF, fmaxf(a.borders[1] - y, 1e-8f)) + __logf(w0);
        }
        if (t == a.nbars - 1) {
          const float w1 = a.borders[a.nbars] - a.borders[a.nbars - 1];
          lp += halfnormal_logprob(w1 / HALFNORMAL_ICDF_HALF, y - a.borders[a.nbars - 1]) + __logf(w1);
        }
      } else if (!in_support) {
        lp = __builtin_nanf("");  // the reference asserts here (bar_distribution.py:27)
      }
      a.nll[r] = -lp;
      a.lse[r] = lse;
      a.bucket[r] = t;
    }
  }
}

__global__ __launch_bounds__(256) void bar_nll_bwd_kernel(BarArgs a) {
  const int lane = threadIdx.x & 63;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < a.R; r += (long)gridDim.x * 4) {
    const float* row = a.logits + r * a.ld;
    float* drow = a.dlogits + r * a.ld;
    const float lse = a.lse[r], g = a.gout[r];
    const int t = a.bucket[r];
    const bool vec = ((reinterpret_cast<uintptr_t>(row) & 15) == 0) && ((reinterpret_cast<uintptr_t>(drow) & 15) == 0);
    const int n4 = vec ? (a.nbars / 4) : 0;
    for (int i = lane; i < n4; i += 64) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * i);
      f32x4 d;
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] = g * (__expf(v[e] - lse) - ((4 * i + e) == t ? 1.f : 0.f));
      *reinterpret_cast<f32x4*>(drow + 4 * i) = d;
    }
    for (int i = n4 * 4 + lane; i < a.nbars; i += 64) drow[i] = g * (__expf(row[i] - lse) - (i == t ? 1.f : 0.f));
  }
}

// mean of bucket i: its midpoint, or for full support the half-normal tail means (bar_distribution.py:110-117)
__device__ __forceinline__ float bar_bucket_mean(const BarArgs& a, int i) {
  const int nb = a.nbars;
  float bm = a.borders[i] + 0.5f * (a.borders[i + 1] - a.borders[i]);
  if (a.full_support) {
    if (i == 0) bm = a.borders[1] - (a.borders[1] - a.borders[0]) / HALFNORMAL_ICDF_HALF * SQRT_2_OVER_PI;
    if (i == nb - 1) bm = a.borders[nb - 1] + (a.borders[nb] - a.borders[nb - 1]) / HALFNORMAL_ICDF_HALF * SQRT_2_OVER_PI;
  }
  return bm;
}
// mean of the bar distribution: softmax(logits) . bucket_means (bar_distribution.py:35-38,110-117)
__global__ __launch_bounds__(256) void bar_mean_kernel(BarArgs a) {
  const int lane = threadIdx.x & 63;
  const int nb = a.nbars;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < a.R; r += (long)gridDim.x * 4) {
    const float* row = a.logits + r * a.ld;
    float mx, se;
    row_max_sumexp(row, nb, lane, mx, se);
    float acc = 0.f;
    for (int i = lane; i < nb; i += 64) acc += __expf(row[i] - mx) * bar_bucket_mean(a, i);
    acc = wave_sum(acc);
    if (lane == 0) a.mean_out[r] = acc / se;
  }
}
// its gradient: d mean / d logit_j = p_j (c_j - mean), times the incoming gout; one wave per row
__global__ __launch_bounds__(256) void bar_mean_bwd_kernel(BarArgs a) {
  const int lane = threadIdx.x & 63;
  const int nb = a.nbars;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < a.R; r += (long)gridDim.x * 4) {
    const float* row = a.logits + r * a.ld;
    float* drow = a.dlogits + r * a.ld;
    float mx, se;
    row_max_sumexp(row, nb, lane, mx, se);
    const float mean = a.mean_out[r], g = a.gout[r] / se;
    for (int i = lane; i < nb; i += 64) drow[i] = g * __expf(row[i] - mx) * (bar_bucket_mean(a, i) - mean);
  }
}

// every kernel of this file: four rows per workgroup of 256 threads, grid-stride over the a.R rows
template <class A> static int launch_rows(void (*kernel)(A), const A& a, size_t lds, hipStream_t s) {
  if (a.R == 0) return PFN_OK;
  hipLaunchKernelGGL(kernel, dim3((int)std::max<long>(1, std::min<long>((a.R + 3) / 4, 8192))), dim3(256), lds, s, a);
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

// ---------------------------------------------------------------------------------------------
// Posterior summaries and draws (pfn_bar_stats / pfn_bar_stats_backward / pfn_bar_sample): generalise BarDistribution.quantile /
// mode / ei (reference bar_distribution.py:40-80) and add variance, CDF, inverse CDF and sampling.  One wave per row, four rows per
// workgroup; the logits row comes from HBM once (the max sweep), the later sweeps of the same row hit the cache, and no [R, nbars]
// intermediate is stored.
//
//   p = softmax(logits), borders b_0 < ... < b_n (n = nbars), w_i = b_{i+1} - b_i, C_k = sum_{i <= k} p_i,
//   c = HALFNORMAL_ICDF_HALF, s_lo = w_0 / c, s_hi = w_{n-1} / c.
//   g_i(y), the conditional CDF of bucket i: clamp((y - b_i) / w_i, 0, 1) for the inner buckets and every bucket of the bounded class;
//     full support: g_0(y) = 1 - erf((b_1 - y) / (s_lo sqrt 2)) for y < b_1 (else 1), g_{n-1}(y) = erf((y - b_{n-1}) / (s_hi sqrt 2))
//     for y > b_{n-1} (else 0) -- the integral of the density of bar_nll_fwd_kernel.
//   CDF      F(y) = sum_i p_i g_i(y)
//   ICDF     Q(u): k = first index with C_k >= u and p_k > 0; inside a linear bucket b_k + w_k (u - C_{k-1}) / p_k clamped to
//            [b_k, b_{k+1}] (monotone in u in f32); in a full-support tail bucket g_k inverted with erfcinvf, the local fraction kept
//            >= 2^-24 so that every u inside (0, 1) gives a finite value.  u <= 0: b_0 (bounded) / -inf (full support); u >= 1: b_n / +inf.
//   VARIANCE sum_i p_i s2_i - mean^2, s2_i = m_i^2 + w_i^2 / 12 (m_i the midpoint); full-support tails m_0 = b_1 - s_lo sqrt(2/pi),
//            s2_0 = b_1^2 - 2 b_1 s_lo sqrt(2/pi) + s_lo^2, m_{n-1} = b_{n-1} + s_hi sqrt(2/pi), s2_{n-1} = b_{n-1}^2 + 2 b_{n-1} s_hi sqrt(2/pi)
//            + s_hi^2.  Evaluated about the centre of the support (b_0 + b_n) / 2 (the variance does not move; the f32 cancellation does).
//   MEAN     as bar_mean_kernel.    MODE  midpoint of the bucket with the largest logit, lowest index on ties (plain midpoint in the
//            tails too: the reference's definition); zero gradient.
//   EI_MAX / EI_MIN  the reference formula (bar_distribution.py:69-80) for BOTH classes: the outer buckets count as [b_0, b_1] and
//            [b_{n-1}, b_n] there, exactly as in BarDistribution.ei.
// Gradients in the logits (the arguments y / u / best_f are not differentiated): T = sum_i p_i c_i gives dT/dl_j = p_j (c_j - T);
//   VARIANCE p_j ((s2_j - E2) - 2 mean (m_j - mean)), E2 = sum_i p_i s2_i;  ICDF dQ/dl_j = -p_j (g_j(Q) - u) / f(Q), f the density at Q
//   (p_k / w_k, or the tail density).  Every one of them is p_j * sum_k G_k (c_k(j) - T_k) with row-uniform G_k, T_k: one write sweep.
//
// The prefix sum of the ICDF: lane l owns the contiguous chunk [l * ceil(n / 64), ...); the 64 chunk sums are scanned across the wave;
// the owning lane (the first whose inclusive sum reaches u * total) walks its chunk serially (icdf_chunk).  Any nbars.
//
// Draws: out[s, r] = Q_r(u(seed, r, s)) through the same icdf_chunk, each lane one draw;
//   a = mix32(lo32(seed) ^ lo32(r) * 0x9E3779B1),  b = mix32(a ^ hi32(seed) ^ hi32(r) * 0x85EBCA77),  h = mix32(b ^ s * 0xC2B2AE35),
//   u = ((h >> 9) + 0.5) * 2^-23      (exact in f32, strictly inside (0, 1); all products modulo 2^32)
// a function of (seed, row, draw index) only.  Only the 64 chunk sums are shared between lanes (in registers): no cap on nbars (the LDS copy of the
// row is an optimisation for nbars <= BAR_LDS_MAX, not a limit).
// ---------------------------------------------------------------------------------------------
constexpr float SQRT_2 = 1.4142135623730951f;
// Rows of up to BAR_LDS_MAX buckets are copied to LDS by the sweep that takes their maximum (the one read from HBM); every later sweep -- the ones with
// a serial dependence above all: the chunk sums and the walk inside the owning chunk -- then waits for LDS instead of the cache.  Longer rows are re-read
// through the cache.  Both give the same bits.
// The borders, read by every sweep of every row, are copied once per workgroup.
constexpr int BAR_LDS_MAX = 3072;      // (4 waves + the borders) x 3072 f32 = 60 KB of dynamic LDS
extern __shared__ __attribute__((aligned(16))) float bar_rows_lds[];

// max and sum of exp(. - max) of a row; srow != nullptr: the row is left there and returned (else the global row is)
// (the kernels are compiled for either case, LDS a template argument, so that every access of a staged row is an LDS instruction and not a flat one:
// flat loads go through the vector-memory address path, one instruction per 16 cycles per CU, and three per element made the sweeps wait for that)
template <bool LDS> PFN_DEV const float* row_stage_max_sumexp(const float* grow, float* srow, int n, int lane, float& mx, float& se) {
  if constexpr (!LDS) { row_max_sumexp(grow, n, lane, mx, se); return grow; }
  __builtin_amdgcn_wave_barrier();      // the wave's reads of the previous row are behind us (LDS operations of one wave retire in order)
  mx = -INFINITY;
  const bool vec = ((reinterpret_cast<uintptr_t>(grow) & 15) == 0);
  const int n4 = vec ? (n / 4) : 0;
  for (int i = lane; i < n4; i += 256) {      // four loads in flight per lane: this sweep waits for HBM
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = i + 64 * u < n4 ? *reinterpret_cast<const f32x4*>(grow + 4 * (i + 64 * u)) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i + 64 * u < n4) *reinterpret_cast<f32x4*>(srow + 4 * (i + 64 * u)) = v[u];
      mx = fmaxf(mx, fmaxf(fmaxf(v[u][0], v[u][1]), fmaxf(v[u][2], v[u][3])));
    }
  }
  for (int i = n4 * 4 + lane; i < n; i += 256) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = i + 64 * u < n ? grow[i + 64 * u] : -INFINITY;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i + 64 * u < n) srow[i + 64 * u] = v[u];
      mx = fmaxf(mx, v[u]);
    }
  }
  mx = wave_max(mx);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  se = 0.f;
  for (int i = lane; i < n / 4; i += 64) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(srow + 4 * i);
    se += __expf(v[0] - mx) + __expf(v[1] - mx) + __expf(v[2] - mx) + __expf(v[3] - mx);
  }
  for (int i = (n / 4) * 4 + lane; i < n; i += 64) se += __expf(srow[i] - mx);
  se = wave_sum(se);
  return srow;
}
template <bool LDS> PFN_DEV float* bar_wave_lds(int nbars) {
  if constexpr (LDS) return bar_rows_lds + (threadIdx.x >> 6) * ((nbars + 3) & ~3);
  else return nullptr;
}
// the borders behind the four rows; every thread of the workgroup calls it once, before its loop over rows
template <bool LDS> PFN_DEV const float* bar_borders_lds(const float* borders, int nbars) {
  if constexpr (!LDS) return borders;
  float* sb = bar_rows_lds + 4 * ((nbars + 3) & ~3);
  for (int i = threadIdx.x; i <= nbars; i += 256) sb[i] = borders[i];
  __syncthreads();
  return sb;
}
static size_t bar_lds_bytes(int nbars) { return nbars <= BAR_LDS_MAX ? ((size_t)4 * ((nbars + 3) & ~3) + nbars + 1) * sizeof(float) : 0; }

struct BarGeom {
  const float* b; int n; int full;
  float s_lo, s_hi, c0;
};
PFN_DEV BarGeom bar_geom(const float* borders, int n, int full) {
  BarGeom g; g.b = borders; g.n = n; g.full = full;
  g.s_lo = (borders[1] - borders[0]) / HALFNORMAL_ICDF_HALF;
  g.s_hi = (borders[n] - borders[n - 1]) / HALFNORMAL_ICDF_HALF;
  g.c0 = 0.5f * (borders[0] + borders[n]);
  return g;
}
// g_i(y)
PFN_DEV float bucket_cdf(const BarGeom& g, int i, float lo, float hi, float y) {
  if (g.full && i == 0) return y < hi ? erfcf((hi - y) / (g.s_lo * SQRT_2)) : 1.f;
  if (g.full && i == g.n - 1) return y > lo ? erff((y - lo) / (g.s_hi * SQRT_2)) : 0.f;
  return fminf(fmaxf((y - lo) / (hi - lo), 0.f), 1.f);
}
// first and second moment of bucket i about c0
PFN_DEV void bucket_moments(const BarGeom& g, int i, float lo, float hi, float& m, float& s2) {
  const float w = hi - lo;
  m = lo + 0.5f * w - g.c0;
  s2 = m * m + w * w * (1.f / 12.f);
  if (g.full && i == 0) {
    const float d = hi - g.c0, t = g.s_lo * SQRT_2_OVER_PI;
    m = d - t; s2 = d * d - 2.f * d * t + g.s_lo * g.s_lo;
  }
  if (g.full && i == g.n - 1) {
    const float d = lo - g.c0, t = g.s_hi * SQRT_2_OVER_PI;
    m = d + t; s2 = d * d + 2.f * d * t + g.s_hi * g.s_hi;
  }
}
// c_i of a statistic that is a sum over p_i c_i.  VARIANCE: s2_i - 2 aux m_i about c0 (aux = 0 in the forward, the mean about c0 in the backward)
PFN_DEV float stat_coef(int kind, float arg, float aux, const BarGeom& g, int i, float lo, float hi) {
  switch (kind) {
    case PFN_BAR_STAT_MEAN: {
      float bm = lo + 0.5f * (hi - lo);
      if (g.full && i == 0) bm = hi - g.s_lo * SQRT_2_OVER_PI;
      if (g.full && i == g.n - 1) bm = lo + g.s_hi * SQRT_2_OVER_PI;
      return bm;
    }
    case PFN_BAR_STAT_VARIANCE: {
      float m, s2;
      bucket_moments(g, i, lo, hi, m, s2);
      return s2 - 2.f * aux * m;
    }
    case PFN_BAR_STAT_CDF: return bucket_cdf(g, i, lo, hi, arg);
    case PFN_BAR_STAT_EI_MAX: return fmaxf(0.5f * (hi + fmaxf(lo, arg)) - arg, 0.f);
    case PFN_BAR_STAT_EI_MIN: return -fminf(0.5f * (fminf(hi, arg) + lo) - arg, 0.f);
    default: return 0.f;
  }
}

PFN_DEV float wave_incl_scan(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
// the lane's chunk of the row and the sum of exp(logit - mx) over it, in index order
PFN_DEV float chunk_sumexp(const float* row, int n, int lane, float mx, int& i0, int& i1) {
  const int chunk = (n + 63) / 64;
  i0 = min(n, lane * chunk); i1 = min(n, i0 + chunk);
  float s = 0.f;
  for (int i = i0; i < i1; ++i) s += __expf(row[i] - mx);
  return s;
}
// Q inside the chunk [i0, i1) that owns the target mass t (in units of exp(logit - mx); excl = the mass before the chunk): the first bucket whose running
// sum reaches t among those with mass, else the chunk's last bucket with mass (the chunk sum and the running sum round differently).  k / ek: that bucket
// and its mass; gk: the fraction of it below Q, i.e. g_k(Q) before Q is rounded to f32.
PFN_DEV float icdf_chunk(const float* row, float mx, const BarGeom& g, int i0, int i1, float excl, float t, int& k, float& ek, float& gk) {
  float c = excl, cprev = excl;
  k = i0; ek = 0.f;
  for (int i = i0; i < i1; ++i) {
    const float e = __expf(row[i] - mx);
    if (e > 0.f) {
      k = i; cprev = c; ek = e;
      if (c + e >= t) break;
    }
    c += e;
  }
  const float lo = g.b[k], hi = g.b[k + 1];
  if (g.full && k == 0) {
    const float frac = fminf(fmaxf((t - cprev) / ek, 5.9604644775390625e-8f), 1.f);
    gk = frac;
    return hi - g.s_lo * SQRT_2 * erfcinvf(frac);
  }
  if (g.full && k == g.n - 1) {
    const float rem = fminf(fmaxf(((cprev + ek) - t) / ek, 5.9604644775390625e-8f), 1.f);
    gk = 1.f - rem;
    return lo + g.s_hi * SQRT_2 * erfcinvf(rem);
  }
  const float frac = fminf(fmaxf((t - cprev) / ek, 0.f), 1.f);
  gk = frac;
  return fminf(fmaxf(lo + (hi - lo) * frac, lo), hi);
}
// u outside (0, 1)
PFN_DEV float icdf_edge(const BarGeom& g, float u) {
  if (u != u) return u;
  if (u <= 0.f) return g.full ? -INFINITY : g.b[0];
  return g.full ? INFINITY : g.b[g.n];
}
// Q(u) for a wave-uniform u: every lane returns it, with the bucket and its mass
PFN_DEV float icdf_wave(const float* row, float mx, const BarGeom& g, int lane, int i0, int i1, float S, float incl, float excl, float total, float u,
                        int& k, float& ek, float& gk) {
  k = -1; ek = 0.f; gk = 0.f;
  if (!(u > 0.f && u < 1.f)) return icdf_edge(g, u);
  const float t = u * total;
  unsigned long long mask = __ballot(incl >= t && S > 0.f);
  int owner;
  if (mask) owner = __ffsll((long long)mask) - 1;
  else owner = max(0, 63 - __clzll((long long)__ballot(S > 0.f)));      // the last chunk with mass
  float q = 0.f;
  if (lane == owner) q = icdf_chunk(row, mx, g, i0, i1, excl, t, k, ek, gk);
  k = __shfl(k, owner, 64); ek = __shfl(ek, owner, 64); gk = __shfl(gk, owner, 64);
  return __shfl(q, owner, 64);
}
// density at Q inside bucket k of mass pk
PFN_DEV float bar_density(const BarGeom& g, int k, float pk, float q) {
  if (g.full && (k == 0 || k == g.n - 1)) {
    const float s = k == 0 ? g.s_lo : g.s_hi;
    const float z = (k == 0 ? g.b[1] - q : q - g.b[g.n - 1]) / s;
    return pk * SQRT_2_OVER_PI / s * __expf(-0.5f * z * z);
  }
  return pk / (g.b[k + 1] - g.b[k]);
}

template <bool LDS> __global__ __launch_bounds__(256) void bar_stats_kernel(BarStatsArgs a) {
  const int lane = threadIdx.x & 63;
  const int nb = a.nbars;
  float* srow = bar_wave_lds<LDS>(nb);
  const float* borders = bar_borders_lds<LDS>(a.borders, nb);
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < a.R; r += (long)gridDim.x * 4) {
    const float* arg = a.args + r * a.arg_ld;
    float* out = a.out + r * a.K;
    float mx, se;
    const float* row = row_stage_max_sumexp<LDS>(a.logits + r * a.ld, srow, nb, lane, mx, se);
    const BarGeom g = bar_geom(borders, nb, a.full_support);
    // one sweep of the (LDS-resident) row per statistic, the kind resolved outside the sweep
    for (int k = 0; k < a.K; ++k) {
      const int kind = a.kinds[k];
      const float av = arg[k];
      if (kind == PFN_BAR_STAT_ICDF) continue;
      float res;
      if (kind == PFN_BAR_STAT_MODE) {
        int mode = nb - 1;
        for (int i = lane; i < nb; i += 64)
          if (row[i] == mx) mode = min(mode, i);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mode = min(mode, __shfl_xor(mode, o, 64));
        res = g.b[mode] + 0.5f * (g.b[mode + 1] - g.b[mode]);
      } else if (kind == PFN_BAR_STAT_VARIANCE) {
        float am = 0.f, as2 = 0.f;
#pragma unroll 4
        for (int i = lane; i < nb; i += 64) {
          float m, s2;
          bucket_moments(g, i, g.b[i], g.b[i + 1], m, s2);
          const float p = __expf(row[i] - mx);
          am += p * m; as2 += p * s2;
        }
        am = wave_sum(am) / se;
        res = fmaxf(wave_sum(as2) / se - am * am, 0.f);
      } else {
        float acc = 0.f;
#pragma unroll 4
        for (int i = lane; i < nb; i += 64) acc += __expf(row[i] - mx) * stat_coef(kind, av, 0.f, g, i, g.b[i], g.b[i + 1]);
        res = wave_sum(acc) / se;
      }
      if (lane == 0) out[k] = res;
    }
    if (a.has_icdf) {
      int i0, i1;
      const float S = chunk_sumexp(row, nb, lane, mx, i0, i1);
      const float incl = wave_incl_scan(S, lane);
      float excl = __shfl_up(incl, 1, 64);
      if (lane == 0) excl = 0.f;
      const float total = __shfl(incl, 63, 64);
      for (int k = 0; k < a.K; ++k) {
        if (a.kinds[k] != PFN_BAR_STAT_ICDF) continue;
        int kk; float ek, gk;
        const float q = icdf_wave(row, mx, g, lane, i0, i1, S, incl, excl, total, arg[k], kk, ek, gk);
        if (lane == 0) out[k] = q;
      }
    }
  }
}

// dlogits[r, j] = p_j sum_k G_k (c_k(j) - T_k): the row-uniform (kind, arg, G, T) of each statistic go through a per-wave LDS table.  An ICDF entry is a CDF
// entry at y = Q with T = u and G = -gout / f(Q); in Q's own bucket it uses the fraction the search found (entries 4, 5) instead of g_k of the rounded Q, which
// keeps sum_j p_j (g_j - u) at zero where one bucket holds nearly all the mass.
template <bool LDS> __global__ __launch_bounds__(256) void bar_stats_bwd_kernel(BarStatsArgs a) {
  __shared__ float tab[4][PFN_BAR_STATS_MAX][6];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nb = a.nbars;
  float* srow = bar_wave_lds<LDS>(nb);
  const float* borders = bar_borders_lds<LDS>(a.borders, nb);
  for (long r = (long)blockIdx.x * 4 + wv; r < a.R; r += (long)gridDim.x * 4) {
    float* drow = a.dlogits + r * a.ld;
    const float* arg = a.args + r * a.arg_ld;
    const float* out = a.out + r * a.K;
    const float* gout = a.gout + r * a.K;
    float mx, se;
    const float* row = row_stage_max_sumexp<LDS>(a.logits + r * a.ld, srow, nb, lane, mx, se);
    const BarGeom g = bar_geom(borders, nb, a.full_support);
    float mean0 = 0.f, e2 = 0.f;      // about c0
    if (a.has_var) {
      for (int i = lane; i < nb; i += 64) {
        float m, s2;
        bucket_moments(g, i, g.b[i], g.b[i + 1], m, s2);
        const float p = __expf(row[i] - mx);
        mean0 += p * m; e2 += p * s2;
      }
      mean0 = wave_sum(mean0) / se; e2 = wave_sum(e2) / se;
    }
    int i0 = 0, i1 = 0;
    float S = 0.f, incl = 0.f, excl = 0.f, total = 0.f;
    if (a.has_icdf) {
      S = chunk_sumexp(row, nb, lane, mx, i0, i1);
      incl = wave_incl_scan(S, lane);
      excl = __shfl_up(incl, 1, 64);
      if (lane == 0) excl = 0.f;
      total = __shfl(incl, 63, 64);
    }
    __builtin_amdgcn_wave_barrier();      // the previous row's readers of the table are done (one wave: LDS operations retire in order)
    for (int k = 0; k < a.K; ++k) {
      int kind = a.kinds[k];
      float av = arg[k], G = gout[k], T = out[k];
      if (kind == PFN_BAR_STAT_VARIANCE) T = e2 - 2.f * mean0 * mean0;
      if (kind == PFN_BAR_STAT_MODE) G = 0.f;
      int kk = -1; float gk = 0.f;
      if (kind == PFN_BAR_STAT_ICDF) {
        float ek;
        const float q = icdf_wave(row, mx, g, lane, i0, i1, S, incl, excl, total, av, kk, ek, gk);
        const float f = kk >= 0 ? bar_density(g, kk, ek / total, q) : 0.f;
        G = (f > 0.f && fabsf(q) < INFINITY) ? -G / f : 0.f;
        kind = PFN_BAR_STAT_CDF; T = av; av = q;
      }
      if (lane == 0) {
        tab[wv][k][0] = __int_as_float(kind); tab[wv][k][1] = av; tab[wv][k][2] = G; tab[wv][k][3] = T;
        tab[wv][k][4] = __int_as_float(kk); tab[wv][k][5] = gk;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float inv_se = 1.f / se;
    auto elem = [&](int i, float v) -> float {
      const float lo = g.b[i], hi = g.b[i + 1];
      float d = 0.f;
      for (int k = 0; k < a.K; ++k) {
        const float G = tab[wv][k][2];
        if (G != 0.f) {
          const float c = i == __float_as_int(tab[wv][k][4]) ? tab[wv][k][5] : stat_coef(__float_as_int(tab[wv][k][0]), tab[wv][k][1], mean0, g, i, lo, hi);
          d += G * (c - tab[wv][k][3]);
        }
      }
      return __expf(v - mx) * inv_se * d;
    };
    const bool vec = ((reinterpret_cast<uintptr_t>(row) & 15) == 0) && ((reinterpret_cast<uintptr_t>(drow) & 15) == 0);
    const int n4 = vec ? (nb / 4) : 0;
    for (int i = lane; i < n4; i += 64) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * i);
      f32x4 d;
      d[0] = elem(4 * i, v[0]); d[1] = elem(4 * i + 1, v[1]); d[2] = elem(4 * i + 2, v[2]); d[3] = elem(4 * i + 3, v[3]);
      *reinterpret_cast<f32x4*>(drow + 4 * i) = d;
    }
    for (int i = n4 * 4 + lane; i < nb; i += 64) drow[i] = elem(i, row[i]);
  }
}

// u(seed, r, s): see the header of this section
PFN_DEV float sample_uniform(unsigned long long seed, long r, int s) {
  const unsigned a = mix32((unsigned)seed ^ ((unsigned)r * 0x9E3779B1u));
  const unsigned b = mix32(a ^ (unsigned)(seed >> 32) ^ ((unsigned)((unsigned long long)r >> 32) * 0x85EBCA77u));
  const unsigned h = mix32(b ^ ((unsigned)s * 0xC2B2AE35u));
  return ((float)(h >> 9) + 0.5f) * 1.1920928955078125e-7f;
}

template <bool LDS> __global__ __launch_bounds__(256) void bar_sample_kernel(BarStatsArgs a) {
  const int lane = threadIdx.x & 63;
  const int nb = a.nbars;
  const int chunk = (nb + 63) / 64;
  float* srow = bar_wave_lds<LDS>(nb);
  const float* borders = bar_borders_lds<LDS>(a.borders, nb);
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < a.R; r += (long)gridDim.x * 4) {
    float mx, se;
    const float* row = row_stage_max_sumexp<LDS>(a.logits + r * a.ld, srow, nb, lane, mx, se);
    const BarGeom g = bar_geom(borders, nb, a.full_support);
    int i0, i1;
    const float S = chunk_sumexp(row, nb, lane, mx, i0, i1);
    const float incl = wave_incl_scan(S, lane);
    const float total = __shfl(incl, 63, 64);
    for (int s0 = 0; s0 < a.n_samples; s0 += 64) {
      const int s = s0 + lane;
      const float t = sample_uniform(a.seed, r, s) * total;
      // the owner of t as icdf_wave finds it: the first chunk with mass whose inclusive sum reaches t, else the last chunk with mass
      int owner = -1, last = 0;
      float oexcl = 0.f, lexcl = 0.f, prev = 0.f;
      for (int l = 0; l < 64; ++l) {
        const float il = __shfl(incl, l, 64), sl = __shfl(S, l, 64);
        if (sl > 0.f) {
          last = l; lexcl = prev;
          if (owner < 0 && il >= t) { owner = l; oexcl = prev; }
        }
        prev = il;
      }
      if (owner < 0) { owner = last; oexcl = lexcl; }
      if (s < a.n_samples) {
        const int o0 = min(nb, owner * chunk), o1 = min(nb, o0 + chunk);
        int k; float ek, gk;
        a.samples[(long)s * a.R + r] = icdf_chunk(row, mx, g, o0, o1, oexcl, t, k, ek, gk);
      }
    }
  }
}

// the checks shared by pfn_bar_stats / pfn_bar_stats_backward / pfn_bar_sample; fills the common fields
static int bar_stats_common(BarStatsArgs& a, const char* what, const float* logits, int64_t ld, const float* borders, int64_t R, int nbars, int full_support) {
  if (R < 0) return fail(PFN_ERR_ARGUMENT, "%s: R = %lld", what, (long long)R);
  if (nbars < 1 || (full_support && nbars < 2)) return fail(PFN_ERR_ARGUMENT, "%s: nbars = %d%s", what, nbars, full_support ? " (full support needs two buckets)" : "");
  if (ld < nbars) return fail(PFN_ERR_ARGUMENT, "%s: ld %lld < nbars %d", what, (long long)ld, nbars);
  if (!logits || !borders) return fail(PFN_ERR_ARGUMENT, "%s: null pointer", what);
  memset(&a, 0, sizeof(a));
  a.logits = logits; a.ld = ld; a.borders = borders; a.R = R; a.nbars = nbars; a.full_support = full_support ? 1 : 0;
  return PFN_OK;
}
static int bar_stats_spec(BarStatsArgs& a, const char* what, const int32_t* kinds, int K, const float* args, int64_t arg_ld) {
  if (K < 1 || K > PFN_BAR_STATS_MAX) return fail(PFN_ERR_ARGUMENT, "%s: K = %d outside 1 .. %d", what, K, PFN_BAR_STATS_MAX);
  if (!kinds || !args) return fail(PFN_ERR_ARGUMENT, "%s: null pointer", what);
  if (arg_ld != 0 && arg_ld < K) return fail(PFN_ERR_ARGUMENT, "%s: arg_ld %lld < K %d", what, (long long)arg_ld, K);
  for (int k = 0; k < K; ++k) {
    if (kinds[k] < PFN_BAR_STAT_MEAN || kinds[k] > PFN_BAR_STAT_EI_MIN) return fail(PFN_ERR_ARGUMENT, "%s: unknown statistic %d at position %d", what, (int)kinds[k], k);
    a.kinds[k] = kinds[k];
    a.has_var |= kinds[k] == PFN_BAR_STAT_VARIANCE; a.has_icdf |= kinds[k] == PFN_BAR_STAT_ICDF;
  }
  a.K = K; a.args = args; a.arg_ld = arg_ld;
  return PFN_OK;
}

}  // namespace pfn

using namespace pfn;

extern "C" {
int pfn_bar_nll_forward(const float* logits, int64_t ld, const float* y, const float* borders, int64_t R, int nbars,
                        int full_support, float* nll, float* lse, int32_t* bucket, void* stream) {
  if (R < 0 || nbars < 1 || (R > 0 && (!logits || !y || !borders || !nll || !lse || !bucket))) return fail(PFN_ERR_ARGUMENT, "bad bar_nll_forward arguments");
  BarArgs a; memset(&a, 0, sizeof(a));
  a.logits = logits; a.ld = ld; a.y = y; a.borders = borders; a.R = R; a.nbars = nbars; a.full_support = full_support;
  a.nll = nll; a.lse = lse; a.bucket = bucket;
  PFN_TRY(launch_rows(bar_nll_fwd_kernel, a, 0, (hipStream_t)stream));
  return PFN_OK;
}
int pfn_bar_nll_backward(const float* logits, int64_t ld, const float* lse, const int32_t* bucket, const float* gout,
                         int64_t R, int nbars, float* dlogits, void* stream) {
  if (R < 0 || nbars < 1 || (R > 0 && (!logits || !lse || !bucket || !gout || !dlogits))) return fail(PFN_ERR_ARGUMENT, "bad bar_nll_backward arguments");
  BarArgs a; memset(&a, 0, sizeof(a));
  a.logits = logits; a.ld = ld; a.R = R; a.nbars = nbars; a.lse = const_cast<float*>(lse); a.bucket = const_cast<int*>(bucket);
  a.gout = gout; a.dlogits = dlogits;
  PFN_TRY(launch_rows(bar_nll_bwd_kernel, a, 0, (hipStream_t)stream));
  return PFN_OK;
}
int pfn_bar_mean(const float* logits, int64_t ld, const float* borders, int64_t R, int nbars, int full_support, float* mean, void* stream) {
  if (R < 0 || nbars < 1 || (R > 0 && (!logits || !borders || !mean))) return fail(PFN_ERR_ARGUMENT, "bad bar_mean arguments");
  BarArgs a; memset(&a, 0, sizeof(a));
  a.logits = logits; a.ld = ld; a.borders = borders; a.R = R; a.nbars = nbars; a.full_support = full_support; a.mean_out = mean;
  PFN_TRY(launch_rows(bar_mean_kernel, a, 0, (hipStream_t)stream));
  return PFN_OK;
}
// dlogits = gout p (c - mean): mean_out holds the forward's means (read only)
int pfn_bar_mean_backward(const float* logits, int64_t ld, const float* borders, int64_t R, int nbars, int full_support, const float* mean, const float* gout,
                          float* dlogits, void* stream) {
  if (R < 0 || nbars < 1 || (R > 0 && (!logits || !borders || !mean || !gout || !dlogits))) return fail(PFN_ERR_ARGUMENT, "bad bar_mean_backward arguments");
  BarArgs a; memset(&a, 0, sizeof(a));
  a.logits = logits; a.ld = ld; a.borders = borders; a.R = R; a.nbars = nbars; a.full_support = full_support;
  a.mean_out = const_cast<float*>(mean); a.gout = gout; a.dlogits = dlogits;
  PFN_TRY(launch_rows(bar_mean_bwd_kernel, a, 0, (hipStream_t)stream));
  return PFN_OK;
}

int pfn_bar_stats(const float* logits, int64_t ld, const float* borders, int64_t R, int nbars, int full_support,
                  const int32_t* kinds, int K, const float* args, int64_t arg_ld, float* out, void* stream) {
  BarStatsArgs a;
  PFN_TRY(bar_stats_common(a, "pfn_bar_stats", logits, ld, borders, R, nbars, full_support));
  PFN_TRY(bar_stats_spec(a, "pfn_bar_stats", kinds, K, args, arg_ld));
  if (!out) return fail(PFN_ERR_ARGUMENT, "pfn_bar_stats: null pointer");
  a.out = out;
  PFN_TRY(launch_rows(nbars <= BAR_LDS_MAX ? bar_stats_kernel<true> : bar_stats_kernel<false>, a, bar_lds_bytes(nbars), (hipStream_t)stream));
  return PFN_OK;
}
int pfn_bar_stats_backward(const float* logits, int64_t ld, const float* borders, int64_t R, int nbars, int full_support,
                           const int32_t* kinds, int K, const float* args, int64_t arg_ld, const float* out, const float* gout,
                           float* dlogits, void* stream) {
  BarStatsArgs a;
  PFN_TRY(bar_stats_common(a, "pfn_bar_stats_backward", logits, ld, borders, R, nbars, full_support));
  PFN_TRY(bar_stats_spec(a, "pfn_bar_stats_backward", kinds, K, args, arg_ld));
  if (!out || !gout || !dlogits) return fail(PFN_ERR_ARGUMENT, "pfn_bar_stats_backward: null pointer");
  a.out = const_cast<float*>(out); a.gout = gout; a.dlogits = dlogits;
  PFN_TRY(launch_rows(nbars <= BAR_LDS_MAX ? bar_stats_bwd_kernel<true> : bar_stats_bwd_kernel<false>, a, bar_lds_bytes(nbars), (hipStream_t)stream));
  return PFN_OK;
}
int pfn_bar_sample(const float* logits, int64_t ld, const float* borders, int64_t R, int nbars, int full_support,
                   int n_samples, uint64_t seed, float* out, void* stream) {
  BarStatsArgs a;
  PFN_TRY(bar_stats_common(a, "pfn_bar_sample", logits, ld, borders, R, nbars, full_support));
  if (n_samples < 0) return fail(PFN_ERR_ARGUMENT, "pfn_bar_sample: n_samples = %d", n_samples);
  if (!out) return fail(PFN_ERR_ARGUMENT, "pfn_bar_sample: null pointer");
  a.n_samples = n_samples; a.seed = seed; a.samples = out;
  if (n_samples == 0) return PFN_OK;
  PFN_TRY(launch_rows(nbars <= BAR_LDS_MAX ? bar_sample_kernel<true> : bar_sample_kernel<false>, a, bar_lds_bytes(nbars), (hipStream_t)stream));
  return PFN_OK;
}
}  // extern "C"
