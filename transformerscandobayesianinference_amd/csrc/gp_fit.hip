// GP hyper-parameter fit on the device (gfx950): the MAP-II objective of reference priors/fast_gp_mix.py:156-169
// (`get_fitted_model`: botorch fit_gpytorch_model on gpytorch's ExactMarginalLogLikelihood), its gradient, and the
// posterior of the fitted model.  Objective, parameterisation and gradient formulas: DESIGN.md section 14.
//
//   J(theta) = -(1/n) [ log N(y_:n; c 1, K) + sum_d lg(l_d) + lg(os) + lg(noise) ],  K = os k(x, x; l) + noise I
//   theta    = (log l_1 .. log l_F, log os, log(noise - floor), c)
//
// Schedule of pfn_gp_mll_grad (problems = grid.y; every matrix is Sp x Sp, Sp = S rounded up to the 64-wide panel, rows and
// columns >= n_p are the identity, so every panel of the factorisation is a whole one):
//   prep     : theta -> os, noise, c, 1/l_d; residual y - c (0 in the masked rows); info = 0
//   gram     : lower-triangular 64x64 tiles of K with the mask (rows >= n_p of x are never read)
//   factor   : launch_gp_factor (gp_prior.hip), posterior mode WITHOUT the plane scratch: the whole factor L stays in the lower
//              triangle, w = L^-1 (y - c) falls out
//   value    : J from diag(L) and w, one workgroup per problem, fixed-order reduction
//   inverse  : M = L^-1, one workgroup per (problem, block column): M_jj is the 64x64 inverse gp_potrf_kernel left beside the
//              diagonal block, M_ij = -L_ii^-1 sum_{j<=k<i} L_ik M_kj            (exact f32 FMA, 64x64 tiles through LDS)
//   alpha    : alpha = M^T w
//   kinv     : K^-1 = M^T M, lower-triangular 64x64 tiles, written over the factor
//   grad     : lower-triangular 64x64 tiles of (i, j): W_ij = alpha_i alpha_j - K^-1_ij, k, g, and nf + 1 sums per tile -> workspace
//   finalize : adds the tile partials in tile order, the trace and mean terms, the hyper-prior, -1/n
// No atomics anywhere: problem p's outputs are a function of (x_p, y_p, n_p, theta_p) alone.
#include <algorithm>
#include "pfn_device.h"
#include "gp_prior.h"

namespace pfn {

struct GpFitArgs {
  const float* x;        // [P,S,nf]
  const float* y;        // [P,S]
  const int32_t* n_of;   // [P] rows in use per problem (device; clamped to [1,S]); null = S
  const float* theta;    // [P,nf+3]: log lengthscale_d, log outputscale, log(noise - floor), constant mean
  const float* prior;    // [8]: a_l, b_l, a_o, b_o, a_n, b_n, noise_floor, 0
  int P, S, nf, kernel, flags;
  void* ws;              // gp_fit_workspace_bytes(P, S)
  float* value;          // [P]
  float* grad;           // [P,nf+3] or null
  const float* x_test;   // [P,m,nf]   (predict)
  int m;
  float* mean;           // [P,m]
  float* var;            // [P,m]
  int32_t* info;         // [P]
};

namespace {

constexpr int FT = 64;        // tile / panel width
constexpr int LDT = 68;       // padded LDS row of a 64x64 f32 tile (16-byte aligned rows)
constexpr int PSTR = 128;     // floats per (problem, tile) partial and per problem of 1/l: nf + 1 <= 127

struct FitWs {
  float *K, *M, *res, *w, *alpha, *part, *ils, *os, *nz, *cm;
  int32_t* nn;
  int Sp, nb, ntiles;
};

inline int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }
inline int fit_sp(int S) { return (S + FT - 1) / FT * FT; }

int64_t carve(FitWs& w, char* base, int P, int S) {
  const int Sp = fit_sp(S), nb = Sp / FT, ntiles = nb * (nb + 1) / 2;
  w.Sp = Sp; w.nb = nb; w.ntiles = ntiles;
  int64_t off = 0;
  auto take = [&](int64_t bytes) { char* p = base ? base + off : nullptr; off += up256(bytes); return p; };
  w.K = (float*)take((int64_t)P * Sp * Sp * 4);
  w.M = (float*)take((int64_t)P * Sp * Sp * 4);
  w.res = (float*)take((int64_t)P * Sp * 4);
  w.w = (float*)take((int64_t)P * Sp * 4);
  w.alpha = (float*)take((int64_t)P * Sp * 4);
  w.part = (float*)take((int64_t)P * ntiles * PSTR * 4);
  w.ils = (float*)take((int64_t)P * PSTR * 4);
  w.os = (float*)take((int64_t)P * 4);
  w.nz = (float*)take((int64_t)P * 4);
  w.cm = (float*)take((int64_t)P * 4);
  w.nn = (int32_t*)take((int64_t)P * 4);
  return off;
}

PFN_DEV void fit_tri_decode(int t, int& ti, int& tj) {      // t = ti (ti + 1) / 2 + tj, tj <= ti
  ti = (int)((sqrtf(8.f * t + 1.f) - 1.f) * 0.5f);
  while (ti * (ti + 1) / 2 > t) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  tj = t - ti * (ti + 1) / 2;
}

// sum over the 256 threads of a workgroup in a fixed order (a tree over LDS); every thread gets the result
PFN_DEV float block_sum256(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// (k, g) of one pair from its scaled squared distance d2 = sum_d (x_id - x_jd)^2 / l_d^2:  dk/d(log l_d) = g (x_id - x_jd)^2 / l_d^2
PFN_DEV void kernel_and_slope(int kernel, float d2, float& k, float& g) {
  if (kernel == 0) { k = expf(-0.5f * d2); g = k; }
  else if (kernel == 1) { const float s = sqrtf(5.f * d2), e = expf(-s); k = (1.f + s + s * s * (1.f / 3.f)) * e; g = (5.f / 3.f) * (1.f + s) * e; }
  else if (kernel == 2) { const float s = sqrtf(3.f * d2), e = expf(-s); k = (1.f + s) * e; g = 3.f * e; }
  else { const float r = sqrtf(d2); k = expf(-r); g = r > 0.f ? k / r : 0.f; }
}

__global__ __launch_bounds__(256) void gpfit_prep_kernel(GpFitArgs a, FitWs w) {
  const int p = blockIdx.x, S = a.S, Sp = w.Sp, nf = a.nf;
  int n = a.n_of ? a.n_of[p] : S;
  n = max(1, min(n, S));
  const float* th = a.theta + (long)p * (nf + 3);
  const float c = th[nf + 2];
  if (threadIdx.x == 0) {
    w.os[p] = expf(th[nf]);
    w.nz[p] = a.prior[6] + expf(th[nf + 1]);
    w.cm[p] = c;
    w.nn[p] = n;
    a.info[p] = 0;
  }
  for (int f = threadIdx.x; f < nf; f += 256) w.ils[(long)p * PSTR + f] = expf(-th[f]);
  for (int t = threadIdx.x; t < Sp; t += 256) w.res[(long)p * Sp + t] = t < n ? a.y[(long)p * S + t] - c : 0.f;
}

// x rows [row0, row0 + 64) of problem p into LDS [64][ldx]; rows >= n are zeros and are never read from memory
PFN_DEV void stage_x(float* dst, const float* xb, int row0, int n, int nf, int ldx) {
  for (int i = threadIdx.x; i < 64 * nf; i += 256) {
    const int r = i / nf, f = i % nf;
    dst[r * ldx + f] = (row0 + r < n) ? xb[(long)(row0 + r) * nf + f] : 0.f;
  }
}

// this thread's 4 x 4 scaled squared distances: rows r0 .. r0 + 3 of xi against rows c0 .. c0 + 3 of xj
PFN_DEV void pair_d2(const float* xi, const float* xj, const float* ils, int nf, int ldx, int r0, int c0, float (&d2)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) d2[i][j] = 0.f;
  for (int f = 0; f < nf; ++f) {
    const float s = ils[f];
    float xa[4], xc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { xa[i] = xi[(r0 + i) * ldx + f] * s; xc[i] = xj[(c0 + i) * ldx + f] * s; }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float d = xa[i] - xc[j]; d2[i][j] += d * d; }
  }
}

// K with the theta layout and the mask: rows / columns >= n are the identity.  Same tiling as gp_gram_kernel (which the sampler keeps for itself).
__global__ __launch_bounds__(256) void gpfit_gram_kernel(GpFitArgs a, FitWs w) {
  extern __shared__ float gs[];      // xi[64][nf+1], xj[64][nf+1]
  const int nf = a.nf, ldx = nf + 1, p = blockIdx.y, Sp = w.Sp, n = w.nn[p];
  float* xi = gs; float* xj = gs + 64 * ldx;
  int ti, tj;
  fit_tri_decode(blockIdx.x, ti, tj);
  const float* xb = a.x + (long)p * a.S * nf;
  stage_x(xi, xb, ti * 64, n, nf, ldx);
  stage_x(xj, xb, tj * 64, n, nf, ldx);
  __syncthreads();
  const int r0 = (threadIdx.x >> 4) * 4, c0 = (threadIdx.x & 15) * 4;
  float d2[4][4];
  pair_d2(xi, xj, w.ils + (long)p * PSTR, nf, ldx, r0, c0, d2);
  const float os = w.os[p], nz = w.nz[p];
  float* Kb = w.K + (long)p * Sp * Sp;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gi = ti * 64 + r0 + i;
    f32x4 kv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gj = tj * 64 + c0 + j;
      float k, g;
      kernel_and_slope(a.kernel, d2[i][j], k, g);
      const float live = os * k + (gi == gj ? nz : 0.f);
      kv[j] = (gi < n && gj < n) ? live : (gi == gj ? 1.f : 0.f);
    }
    *reinterpret_cast<f32x4*>(Kb + (long)gi * Sp + tj * 64 + c0) = kv;
  }
}

// J(theta) per problem from the factor's diagonal and w = L^-1 (y - c)
__global__ __launch_bounds__(256) void gpfit_value_kernel(GpFitArgs a, FitWs w) {
  __shared__ float red[256];
  const int p = blockIdx.x, Sp = w.Sp, nf = a.nf, n = w.nn[p];
  const float* Kb = w.K + (long)p * Sp * Sp;
  float sl = 0.f, sq = 0.f;
  for (int t = threadIdx.x; t < n; t += 256) {
    sl += logf(Kb[(long)t * Sp + t]);
    const float v = w.w[(long)p * Sp + t];
    sq += v * v;
  }
  sl = block_sum256(sl, red);
  sq = block_sum256(sq, red);
  if (threadIdx.x != 0) return;
  if (a.info[p] != 0) { a.value[p] = __builtin_inff(); return; }
  const float* th = a.theta + (long)p * (nf + 3);
  const float al = a.prior[0], bl = a.prior[1], ao = a.prior[2], bo = a.prior[3], an = a.prior[4], bn = a.prior[5];
  float lp = 0.f;
  for (int f = 0; f < nf; ++f) lp += (al - 1.f) * th[f] - bl * expf(th[f]);
  lp += nf * (al * logf(bl) - lgammaf(al));
  lp += ao * logf(bo) - lgammaf(ao) + (ao - 1.f) * th[nf] - bo * w.os[p];
  lp += an * logf(bn) - lgammaf(an) + (an - 1.f) * logf(w.nz[p]) - bn * w.nz[p];
  const float ll = -0.5f * sq - sl - 0.9189385332046727f * n;
  a.value[p] = -(ll + lp) / n;
}

// ---- 64 x 64 f32 tiles through LDS ----------------------------------------------------------------------------------
// T[r][c] = src[r][c] (or T[c][r] with `transpose`): 256 threads, 16-byte loads
PFN_DEV void load_tile(float (*T)[LDT], const float* src, long ld, bool transpose) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (threadIdx.x >> 4) + 16 * i, c = (threadIdx.x & 15) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + (long)r * ld + c);
    if (!transpose) { T[r][c] = v[0]; T[r][c + 1] = v[1]; T[r][c + 2] = v[2]; T[r][c + 3] = v[3]; }
    else { T[c][r] = v[0]; T[c + 1][r] = v[1]; T[c + 2][r] = v[2]; T[c + 3][r] = v[3]; }
  }
}
// acc[i][j] += sum_k A[ty 4 + i][k] B[k][tx 4 + j]
PFN_DEV void tile_mac(const float (*A)[LDT], const float (*B)[LDT], float (&acc)[4][4], int ty, int tx) {
#pragma unroll 8
  for (int k = 0; k < 64; ++k) {
    float av[4], bv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { av[i] = A[ty * 4 + i][k]; bv[i] = B[k][tx * 4 + i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] += av[i] * bv[j];
  }
}
// the inverse of the 64 x 64 block factor L_ii: gp_potrf_kernel leaves the diagonal block as [L \ L^-T] with diag = L, so
// L^-1[r][c] (c < r) sits at (c, r) of the block and L^-1[r][r] = 1 / L[r][r]
PFN_DEV void load_block_inverse(float (*T)[LDT], const float* Kd, long ld) {
  for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
    const int c = idx >> 6, r = idx & 63;
    const float v = Kd[(long)c * ld + r];
    T[r][c] = c < r ? v : (c == r ? 1.f / v : 0.f);
  }
}

// M = L^-1, block column j of problem p.  Blocks at or beyond the first fully masked block row are the identity and are not formed (nobody reads them).
__global__ __launch_bounds__(256) void gpfit_inv_kernel(FitWs w) {
  __shared__ float As[64][LDT], Bs[64][LDT];
  const int j = blockIdx.x, p = blockIdx.y, Sp = w.Sp;
  const int nlive = (w.nn[p] + FT - 1) / FT;
  if (j >= nlive) return;
  const float* Kb = w.K + (long)p * Sp * Sp;
  float* Mb = w.M + (long)p * Sp * Sp;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  load_block_inverse(As, Kb + (long)(j * FT) * Sp + j * FT, Sp);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = ty * 4 + i;
    *reinterpret_cast<f32x4*>(Mb + (long)(j * FT + r) * Sp + j * FT + tx * 4) = f32x4{As[r][tx * 4], As[r][tx * 4 + 1], As[r][tx * 4 + 2], As[r][tx * 4 + 3]};
  }
  for (int ib = j + 1; ib < nlive; ++ib) {
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) acc[i][jj] = 0.f;
    for (int k = j; k < ib; ++k) {
      __syncthreads();      // the tiles are free again, and this workgroup's earlier stores of M_kj are visible to all of its waves
      load_tile(As, Kb + (long)(ib * FT) * Sp + k * FT, Sp, false);      // L_ik
      load_tile(Bs, Mb + (long)(k * FT) * Sp + j * FT, Sp, false);       // M_kj
      __syncthreads();
      tile_mac(As, Bs, acc, ty, tx);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) Bs[ty * 4 + i][tx * 4 + jj] = acc[i][jj];
    load_block_inverse(As, Kb + (long)(ib * FT) * Sp + ib * FT, Sp);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) acc[i][jj] = 0.f;
    tile_mac(As, Bs, acc, ty, tx);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<f32x4*>(Mb + (long)(ib * FT + ty * 4 + i) * Sp + j * FT + tx * 4) = f32x4{-acc[i][0], -acc[i][1], -acc[i][2], -acc[i][3]};
  }
}

// alpha = M^T w: one column per lane, four row groups per workgroup added in a fixed order
__global__ __launch_bounds__(256) void gpfit_alpha_kernel(FitWs w) {
  __shared__ float red[4][64];
  const int a0 = blockIdx.x * FT, p = blockIdx.y, Sp = w.Sp, n = w.nn[p];
  const int col = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const float* Mb = w.M + (long)p * Sp * Sp;
  const float* wv = w.w + (long)p * Sp;
  float s = 0.f;
  if (a0 < n)
    for (int r = a0 + rg; r < n; r += 4) s += Mb[(long)r * Sp + a0 + col] * wv[r];
  red[rg][col] = s;
  __syncthreads();
  if (rg == 0) w.alpha[(long)p * Sp + a0 + col] = (a0 + col < n) ? ((red[0][col] + red[1][col]) + red[2][col]) + red[3][col] : 0.f;
}

// K^-1 = M^T M, tile (A >= B) of problem p, written over the factor (the value and alpha have been taken from it)
__global__ __launch_bounds__(256) void gpfit_kinv_kernel(FitWs w) {
  __shared__ float As[64][LDT], Bs[64][LDT];
  const int p = blockIdx.y, Sp = w.Sp;
  const int nlive = (w.nn[p] + FT - 1) / FT;
  int A, B;
  fit_tri_decode(blockIdx.x, A, B);
  if (A >= nlive) return;
  const float* Mb = w.M + (long)p * Sp * Sp;
  float* Kb = w.K + (long)p * Sp * Sp;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) acc[i][jj] = 0.f;
  for (int R = A; R < nlive; ++R) {
    if (R > A) __syncthreads();
    load_tile(As, Mb + (long)(R * FT) * Sp + A * FT, Sp, true);      // (M_RA)^T
    load_tile(Bs, Mb + (long)(R * FT) * Sp + B * FT, Sp, false);     // M_RB
    __syncthreads();
    tile_mac(As, Bs, acc, ty, tx);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *reinterpret_cast<f32x4*>(Kb + (long)(A * FT + ty * 4 + i) * Sp + B * FT + tx * 4) = f32x4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
}

// The fused gradient reduction: tile (ti >= tj) of problem p.  Per pair W_ij, k, g; per tile nf + 1 sums:
//   part[d]  = 1/2 sum_ij W_ij os g_ij (x_id - x_jd)^2 / l_d^2     (d < nf)
//   part[nf] = 1/2 sum_ij W_ij os k_ij
// over the pairs j <= i < n of the tile, pairs off the diagonal counted twice (W, k and g are symmetric).  One read of K^-1.
constexpr int GR_CH = 8;      // features per pass over the 16 pair weights a thread keeps
__global__ __launch_bounds__(256) void gpfit_grad_kernel(GpFitArgs a, FitWs w) {
  extern __shared__ float gs[];      // xi[64][nf+1], xj[64][nf+1], red[4][GR_CH]
  const int nf = a.nf, ldx = nf + 1, p = blockIdx.y, Sp = w.Sp, n = w.nn[p];
  float* xi = gs; float* xj = gs + 64 * ldx; float* red = gs + 128 * ldx;
  int ti, tj;
  fit_tri_decode(blockIdx.x, ti, tj);
  float* part = w.part + ((long)p * w.ntiles + blockIdx.x) * PSTR;
  if (ti * 64 >= n) {
    for (int d = threadIdx.x; d <= nf; d += 256) part[d] = 0.f;
    return;
  }
  const float* xb = a.x + (long)p * a.S * nf;
  const float* ils = w.ils + (long)p * PSTR;
  stage_x(xi, xb, ti * 64, n, nf, ldx);
  stage_x(xj, xb, tj * 64, n, nf, ldx);
  __syncthreads();
  const int r0 = (threadIdx.x >> 4) * 4, c0 = (threadIdx.x & 15) * 4;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float d2[4][4];
  pair_d2(xi, xj, ils, nf, ldx, r0, c0, d2);
  const float os = w.os[p];
  const float* Kb = w.K + (long)p * Sp * Sp;
  const float* al = w.alpha + (long)p * Sp;
  float q[4][4];
  float sk = 0.f;
  float aj[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) aj[j] = al[tj * 64 + c0 + j];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gi = ti * 64 + r0 + i;
    const float ai = al[gi];
    const f32x4 kin = *reinterpret_cast<const f32x4*>(Kb + (long)gi * Sp + tj * 64 + c0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gj = tj * 64 + c0 + j;
      float k, g;
      kernel_and_slope(a.kernel, d2[i][j], k, g);
      const float wgt = (gi < n && gj <= gi) ? (gi == gj ? 1.f : 2.f) * (ai * aj[j] - kin[j]) * os : 0.f;
      q[i][j] = (gi < n && gj <= gi) ? wgt * g : 0.f;
      sk += (gi < n && gj <= gi) ? wgt * k : 0.f;
    }
  }
  auto wave_sum = [](float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
  };
  for (int f0 = 0; f0 < nf; f0 += GR_CH) {
    float acc[GR_CH];
#pragma unroll
    for (int e = 0; e < GR_CH; ++e) {
      acc[e] = 0.f;
      const int f = min(f0 + e, nf - 1);
      float xa[4], xc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { xa[i] = xi[(r0 + i) * ldx + f]; xc[i] = xj[(c0 + i) * ldx + f]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float d = xa[i] - xc[j]; acc[e] += q[i][j] * (d * d); }
    }
#pragma unroll
    for (int e = 0; e < GR_CH; ++e) {
      const float s = wave_sum(acc[e]);
      if (lane == 0) red[wave * GR_CH + e] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < GR_CH && f0 + (int)threadIdx.x < nf) {
      const int e = threadIdx.x, f = f0 + e;
      const float s = ((red[e] + red[GR_CH + e]) + red[2 * GR_CH + e]) + red[3 * GR_CH + e];
      part[f] = 0.5f * s * ils[f] * ils[f];
    }
    __syncthreads();
  }
  {
    const float s = wave_sum(sk);
    if (lane == 0) red[wave * GR_CH] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[nf] = 0.5f * (((red[0] + red[GR_CH]) + red[2 * GR_CH]) + red[3 * GR_CH]);
  }
}

__global__ __launch_bounds__(256) void gpfit_finalize_kernel(GpFitArgs a, FitWs w) {
  __shared__ float red[256];
  const int p = blockIdx.x, Sp = w.Sp, nf = a.nf, D = nf + 3, n = w.nn[p];
  float* gr = a.grad + (long)p * D;
  const float* Kb = w.K + (long)p * Sp * Sp;
  float tr = 0.f, sa = 0.f;
  for (int t = threadIdx.x; t < n; t += 256) {
    const float al = w.alpha[(long)p * Sp + t];
    tr += al * al - Kb[(long)t * Sp + t];
    sa += al;
  }
  tr = block_sum256(tr, red);
  sa = block_sum256(sa, red);
  const int d = threadIdx.x;
  if (d >= D) return;
  if (a.info[p] != 0) { gr[d] = 0.f; return; }
  const float* th = a.theta + (long)p * D;
  const float inv_n = 1.f / n;
  if (d <= nf) {
    const float* part = w.part + (long)p * w.ntiles * PSTR + d;
    float s = 0.f;
    for (int t = 0; t < w.ntiles; ++t) s += part[(long)t * PSTR];
    const float lp = d < nf ? (a.prior[0] - 1.f) - a.prior[1] * expf(th[d]) : (a.prior[2] - 1.f) - a.prior[3] * w.os[p];
    gr[d] = -(s + lp) * inv_n;
  } else if (d == nf + 1) {
    const float nz = w.nz[p], ge = nz - a.prior[6];
    gr[d] = -(0.5f * tr * ge + ((a.prior[4] - 1.f) / nz - a.prior[5]) * ge) * inv_n;
  } else {
    gr[d] = (a.flags & 1) ? 0.f : -sa * inv_n;
  }
}

// Posterior of the fitted model at one test point per workgroup: v = L^-1 k* = M k*, mean = c + v . w, var = os + noise - |v|^2 (the triangular form:
// k*^T K^-1 k* would cancel).  One wave per row of M, rows dealt to the four waves, sums in a fixed order.
__global__ __launch_bounds__(256) void gpfit_predict_kernel(GpFitArgs a, FitWs w) {
  extern __shared__ float gs[];      // ks[Sp], xt[nf], red[8]
  const int jt = blockIdx.x, p = blockIdx.y, Sp = w.Sp, nf = a.nf, n = w.nn[p];
  float* ks = gs; float* xt = gs + Sp; float* red = xt + nf;
  const float* xb = a.x + (long)p * a.S * nf;
  const float* ils = w.ils + (long)p * PSTR;
  for (int f = threadIdx.x; f < nf; f += 256) xt[f] = a.x_test[((long)p * a.m + jt) * nf + f];
  __syncthreads();
  const float os = w.os[p];
  for (int r = threadIdx.x; r < n; r += 256) {
    float d2 = 0.f;
    for (int f = 0; f < nf; ++f) { const float d = (xb[(long)r * nf + f] - xt[f]) * ils[f]; d2 += d * d; }
    float k, g;
    kernel_and_slope(a.kernel, d2, k, g);
    ks[r] = os * k;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* Mb = w.M + (long)p * Sp * Sp;
  const float* wv = w.w + (long)p * Sp;
  float sm = 0.f, sv = 0.f;
  for (int r = wave; r < n; r += 4) {
    float v = 0.f;
    for (int c = lane; c <= r; c += 64) v += Mb[(long)r * Sp + c] * ks[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    sm += v * wv[r];
    sv += v * v;
  }
  if (lane == 0) { red[wave] = sm; red[4 + wave] = sv; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.mean[(long)p * a.m + jt] = w.cm[p] + (((red[0] + red[1]) + red[2]) + red[3]);
    a.var[(long)p * a.m + jt] = os + w.nz[p] - (((red[4] + red[5]) + red[6]) + red[7]);
  }
}

// prep, Gram, factorisation (posterior mode, no plane scratch: every panel of L goes back to the matrix)
int fit_factor(const GpFitArgs& a, const FitWs& w, hipStream_t s) {
  const size_t lds = (size_t)128 * (a.nf + 1) * sizeof(float);
  if (lds + 4 * GR_CH * sizeof(float) > 64 * 1024) return PFN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gpfit_prep_kernel, dim3(a.P), dim3(256), 0, s, a, w);
  hipLaunchKernelGGL(gpfit_gram_kernel, dim3(w.ntiles, a.P), dim3(256), lds, s, a, w);
  GpArgs g{};
  g.y = w.res; g.K = w.K; g.outputscale = w.os; g.noise = w.nz; g.B = a.P; g.S = w.Sp; g.nf = a.nf; g.kernel = a.kernel;
  g.info = a.info; g.w = w.w; g.planes = nullptr; g.plane_rows = 0;
  return launch_gp_factor(g, s);
}

int64_t gp_fit_workspace_bytes(int P, int S) {
  FitWs w;
  return carve(w, nullptr, P, S);
}

int launch_gp_mll_grad(const GpFitArgs& a, hipStream_t s) {
  if (a.S % 4) return PFN_ERR_UNSUPPORTED;
  FitWs w;
  carve(w, (char*)a.ws, a.P, a.S);
  if (int rc = fit_factor(a, w, s)) return rc;
  hipLaunchKernelGGL(gpfit_value_kernel, dim3(a.P), dim3(256), 0, s, a, w);
  if (a.grad) {
    hipLaunchKernelGGL(gpfit_inv_kernel, dim3(w.nb, a.P), dim3(256), 0, s, w);
    hipLaunchKernelGGL(gpfit_alpha_kernel, dim3(w.nb, a.P), dim3(256), 0, s, w);
    hipLaunchKernelGGL(gpfit_kinv_kernel, dim3(w.ntiles, a.P), dim3(256), 0, s, w);
    const size_t lds = ((size_t)128 * (a.nf + 1) + 4 * GR_CH) * sizeof(float);
    hipLaunchKernelGGL(gpfit_grad_kernel, dim3(w.ntiles, a.P), dim3(256), lds, s, a, w);
    hipLaunchKernelGGL(gpfit_finalize_kernel, dim3(a.P), dim3(256), 0, s, a, w);
  }
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

int launch_gp_fit_predict(const GpFitArgs& a, hipStream_t s) {
  if (a.S % 4) return PFN_ERR_UNSUPPORTED;
  FitWs w;
  carve(w, (char*)a.ws, a.P, a.S);
  const size_t lds = ((size_t)w.Sp + a.nf + 8) * sizeof(float);
  if (lds > 64 * 1024) return PFN_ERR_UNSUPPORTED;
  if (int rc = fit_factor(a, w, s)) return rc;
  if (a.m > 0) {
    hipLaunchKernelGGL(gpfit_inv_kernel, dim3(w.nb, a.P), dim3(256), 0, s, w);
    hipLaunchKernelGGL(gpfit_predict_kernel, dim3(a.m, a.P), dim3(256), lds, s, a, w);
  }
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

int gp_fit_check(const float* x, const float* y, const float* theta, const float* prior, int P, int S, int nf, int kernel, void* ws, int64_t ws_bytes, int32_t* info) {
  if (!x || !y || !theta || !prior || !ws || !info || P < 1 || S < 1 || nf < 1) return fail(PFN_ERR_ARGUMENT, "bad gp_fit arguments");
  if (P > 65535) return fail(PFN_ERR_UNSUPPORTED, "P %d > 65535 problems per call", P);
  if (S % 4) return fail(PFN_ERR_UNSUPPORTED, "S %d is not a multiple of 4", S);
  if (nf > 126) return fail(PFN_ERR_UNSUPPORTED, "nf %d > 126 (the tiles stage 128 rows of x in 64 KB of LDS)", nf);
  if (kernel < 0 || kernel > 3) return fail(PFN_ERR_UNSUPPORTED, "kernel %d (0 = RBF, 1 / 2 / 3 = Matern nu 5/2, 3/2, 1/2)", kernel);
  if (ws_bytes < gp_fit_workspace_bytes(P, S)) return fail(PFN_ERR_ARGUMENT, "ws_bytes %lld < pfn_gp_fit_workspace_bytes = %lld", (long long)ws_bytes, (long long)gp_fit_workspace_bytes(P, S));
  return PFN_OK;
}

}  // namespace
}  // namespace pfn

using namespace pfn;

extern "C" {
int64_t pfn_gp_fit_workspace_bytes(int P, int S) {
  if (P < 1 || S < 1) return -1;
  return gp_fit_workspace_bytes(P, S);
}
int pfn_gp_mll_grad(const float* x, const float* y, const int32_t* n_of, const float* theta, const float* prior, int P, int S, int nf, int kernel, int flags,
                    void* ws, int64_t ws_bytes, float* value, float* grad, int32_t* info, void* stream) {
  if (int rc = gp_fit_check(x, y, theta, prior, P, S, nf, kernel, ws, ws_bytes, info)) return rc;
  if (!value) return fail(PFN_ERR_ARGUMENT, "bad gp_mll_grad arguments");
  GpFitArgs a{};
  a.x = x; a.y = y; a.n_of = n_of; a.theta = theta; a.prior = prior; a.P = P; a.S = S; a.nf = nf; a.kernel = kernel; a.flags = flags;
  a.ws = ws; a.value = value; a.grad = grad; a.info = info;
  PFN_TRY(launch_gp_mll_grad(a, (hipStream_t)stream));
  return PFN_OK;
}
int pfn_gp_fit_predict(const float* x, const float* y, const int32_t* n_of, const float* theta, const float* prior, int P, int S, int nf, int kernel,
                       const float* x_test, int m, void* ws, int64_t ws_bytes, float* mean, float* var, int32_t* info, void* stream) {
  if (int rc = gp_fit_check(x, y, theta, prior, P, S, nf, kernel, ws, ws_bytes, info)) return rc;
  if (m < 0 || (m > 0 && (!x_test || !mean || !var))) return fail(PFN_ERR_ARGUMENT, "bad gp_fit_predict arguments");
  GpFitArgs a{};
  a.x = x; a.y = y; a.n_of = n_of; a.theta = theta; a.prior = prior; a.P = P; a.S = S; a.nf = nf; a.kernel = kernel; a.flags = 0;
  a.ws = ws; a.x_test = x_test; a.m = m; a.mean = mean; a.var = var; a.info = info;
  PFN_TRY(launch_gp_fit_predict(a, (hipStream_t)stream));
  return PFN_OK;
}
}  // extern "C"
