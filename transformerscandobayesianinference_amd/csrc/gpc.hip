// The tabular study's GP-classifier baseline (reference tabular.py:480-503; DESIGN.md section 21, include/pfn_hip.h "GP classifier"): the Laplace approximation
// of scikit-learn's binary GaussianProcessClassifier under c * RBF(l), theta = (log c, log l), one block of 256 threads per fit (problem, candidate, slot).
//   kernel      K = c exp(-d^2 / 2 l^2) on the fit's training rows, compacted: held-out rows are not in K at all
//   mode        GPML algorithm 3.1 from f = 0:  pi = sigma(f), W = pi (1 - pi), B = I + W^1/2 K W^1/2 = L L^T, b = W f + (y - pi),
//               a = b - W^1/2 B^-1 W^1/2 K b, f = K a, Z = -1/2 a.f - sum softplus(-(2y - 1) f) - sum log L_ii.  As in scikit-learn pi, W and L are those of the
//               LAST iteration, one step behind f.
//   stop        the change of Z, summed from the rows' term differences, below 2^-20 max(1, |Z|) (or NaN), then GPC_EXTRA = 2 more iterations, which bring
//               the one-step-behind pi to f32's floor (Newton squares the error each time); at most PFN_GPC_MAX_NEWTON iterations
//   gradient    GPML algorithm 5.1 with K_0 = K, K_1 = K * d^2 / l^2; its trace and diagonal terms through B^-1, which does not cancel where K is near rank one
//   prediction  decision values as pairs (m, e), f* = m exp(-e), so that the sign survives where exp underflows in f32; var = c - |L^-1 W^1/2 k*|^2
// K, the factor (inverted in place for the gradient) and one more n x n matrix (the exponent arguments d^2 / 2 l^2) live in LDS at the odd stride n | 1.  No global
// atomics, no workspace, no communication between blocks, no warm start: a result is a bitwise function of its own (problem, theta, slot).
#include "fold_device.h"

namespace pfn {

struct GpcArgs {
  const float* theta;        // [P,NC,6,2] = (log c, log l) of every fit
  const float* train;        // [P,n,F]
  const float* labels;       // [P,n]: class = label > 0.5
  const float* test;         // [P,T,F] (predict)
  const int32_t* fold;       // [P,n]: the CV test fold of each train row
  int P, n, T, F, NC, n_splits;
  float* value;              // [P,NC,6] = -Z (lml_grad)
  float* grad;               // [P,NC,6,2] = -dZ/dtheta (lml_grad)
  int32_t* status;           // [P,NC,6,2] = (exit reason, Newton iterations)
  float* cv_f;               // [P,NC,n,2] (predict): (m, e) of every held-out row
  float* test_f;             // [P,NC,T,2] (predict)
  float* test_var;           // [P,NC,T] (predict)
};
// K, the exponent arguments and the factor (inverted in place for the gradient) at the odd stride n | 1, sixteen vectors over the rows, eight words of reduction space:
// 159,072 bytes at n = 112, 82,912 at the study's n = 80
inline size_t gpc_lds_bytes(int n) { return ((size_t)3 * n * (n | 1) + 16 * (size_t)n + 8) * 4; }

namespace {

#define GPC_DEV __device__ __forceinline__

constexpr int GPC_THREADS = 256;
constexpr int GPC_EXTRA = 2;                           // iterations after the first that meets the stopping level
constexpr float GPC_STOP = 9.5367431640625e-07f;       // 2^-20: eight f32 steps of |Z|

struct GpcLds {
  float *K, *M, *L;      // [n][ns] each; K and M are adjacent (the prediction reuses both as one table of query rows)
  float *y, *f, *a, *pi, *sw, *b, *r, *u0, *u1, *s2, *t0, *t1, *x0, *x1;      // [n] each
  float* px;             // [n]: B's pivots minus one (shares x1, which is written only after the last use of px)
  int *idx, *qidx;       // [n] each: the training rows of this fit, its held-out rows
  float* red;            // [8]
};

GPC_DEV GpcLds gpc_carve(float* base, int n, int ns) {
  GpcLds s;
  s.K = base; s.M = s.K + n * ns; s.L = s.M + n * ns;
  float* v = s.L + n * ns;
  s.y = v; s.f = v + n; s.a = v + 2 * n; s.pi = v + 3 * n; s.sw = v + 4 * n; s.b = v + 5 * n; s.r = v + 6 * n; s.u0 = v + 7 * n; s.u1 = v + 8 * n;
  s.s2 = v + 9 * n; s.t0 = v + 10 * n; s.t1 = v + 11 * n; s.x0 = v + 12 * n; s.x1 = v + 13 * n; s.px = s.x1;
  s.idx = reinterpret_cast<int*>(v + 14 * n); s.qidx = reinterpret_cast<int*>(v + 15 * n);
  s.red = v + 16 * n;
  return s;
}

// the exponent argument d^2 / 2 l^2 of two rows
GPC_DEV float gpc_arg(const float* xa, const float* xb, int F, float inv2l2) {
  float d2 = 0.f;
  for (int j = 0; j < F; ++j) { const float d = xa[j] - xb[j]; d2 = __builtin_fmaf(d, d, d2); }
  return d2 * inv2l2;
}

// The training rows of fit (p, s) compacted into s.idx (the held-out rows into s.qidx), labels into s.y, the exponent arguments into M and K = c exp(-M).
// Returns false when the training rows hold one class (nothing but idx / qidx / y is written then).
GPC_DEV bool gpc_stage(const GpcLds& s, const GpcArgs& a, int p, int slot, int ns, float c, float inv2l2, int* m_out, int* nq_out) {
  __shared__ int counts[4];
  const int n = a.n, tid = threadIdx.x;
  const bool refit = slot == a.n_splits;
  if (tid == 0) {
    int m = 0, q = 0, pos = 0;
    for (int i = 0; i < n; ++i) {
      const bool train = refit || a.fold[(long)p * n + i] != slot;
      if (train) { s.idx[m] = i; const bool one = a.labels[(long)p * n + i] > 0.5f; s.y[m] = one ? 1.f : 0.f; pos += one; ++m; }
      else s.qidx[q++] = i;
    }
    counts[0] = m; counts[1] = q; counts[2] = pos;
  }
  __syncthreads();
  const int m = counts[0];
  *m_out = m; *nq_out = counts[1];
  if (counts[2] == 0 || counts[2] == m) return false;
  const float* x = a.train + (long)p * n * a.F;
  for (int q = tid; q < m * m; q += GPC_THREADS) {
    const int i = q / m, k = q - i * m;
    if (k <= i) {
      const float arg = i == k ? 0.f : gpc_arg(x + (long)s.idx[i] * a.F, x + (long)s.idx[k] * a.F, a.F, inv2l2);
      const float v = c * expf(-arg);
      s.M[i * ns + k] = arg; s.M[k * ns + i] = arg;
      s.K[i * ns + k] = v; s.K[k * ns + i] = v;
    }
  }
  __syncthreads();
  return true;
}

// GPML algorithm 3.1 on K [m][ns].  Leaves pi, sw = W^1/2, L (the factor of B, lower triangle), a and f as scikit-learn's _posterior_mode leaves them.
GPC_DEV int gpc_mode(const GpcLds& s, int m, int ns, float* Z_out, int* iters_out) {
  const int tid = threadIdx.x, lane = tid & 63;
  float tprev = 0.f, Z = 0.f;
  int reason = PFN_GPC_CAPPED, it = 0, left = -1;
  if (tid < m) s.f[tid] = 0.f;
  __syncthreads();
  for (;;) {
    ++it;
    if (tid < m) {
      const float fi = s.f[tid], e = expf(-fabsf(fi)), hi = 1.f / (1.f + e), lo = e * hi, p = fi >= 0.f ? hi : lo, w = hi * lo;
      s.pi[tid] = p;
      s.sw[tid] = sqrtf(w);
      s.b[tid] = __builtin_fmaf(w, fi, s.y[tid] - p);
    }
    __syncthreads();
    for (int q = tid; q < m * m; q += GPC_THREADS) {
      const int i = q / m, k = q - i * m;
      if (k <= i) s.L[i * ns + k] = s.sw[i] * s.K[i * ns + k] * s.sw[k];      // B - I: the diagonal carries the pivot's excess over 1 until its column is reached
    }
    __syncthreads();
    // in-place Cholesky of the lower triangle (right-looking); B's pivots are >= 1 in exact arithmetic.  The excess pivot - 1 is kept (px): where c is small
    // B is I plus little, and log L_kk and 1 - (B^-1)_kk are that little
    bool bad = false;
    for (int k = 0; k < m; ++k) {
      const float ex = s.L[k * ns + k], piv = 1.f + ex;
      if (!(piv > 0.f)) { bad = true; break; }      // (the same in every thread)
      const float root = sqrtf(piv), inv = 1.f / root;
      __syncthreads();      // every thread has read the pivot
      const int mm = m - k - 1;
      if (tid == 0) { s.L[k * ns + k] = root; s.px[k] = ex; }
      for (int i = tid; i < mm; i += GPC_THREADS) s.L[(k + 1 + i) * ns + k] *= inv;
      __syncthreads();
      for (int q = tid; q < mm * mm; q += GPC_THREADS) {
        const int i = q / mm, j = q - i * mm;
        if (j <= i) s.L[(k + 1 + i) * ns + (k + 1 + j)] -= s.L[(k + 1 + i) * ns + k] * s.L[(k + 1 + j) * ns + k];
      }
      __syncthreads();
    }
    if (bad) { reason = PFN_GPC_NONPOSITIVE; break; }
    if (tid < m) {
      float acc = 0.f;
      for (int k = 0; k < m; ++k) acc = __builtin_fmaf(s.K[tid * ns + k], s.b[k], acc);
      s.u0[tid] = s.sw[tid] * acc;
    }
    __syncthreads();
    // L z = W^1/2 K b, L^T x = z: wave 0, row lane + 64 r in register r;  a = b - W^1/2 x
    if (tid < 64) {
      float r0 = lane < m ? s.u0[lane] : 0.f, r1 = lane + 64 < m ? s.u0[lane + 64] : 0.f;
      for (int k = 0; k < m; ++k) {
        const float zk = __shfl(k < 64 ? r0 : r1, k & 63, 64) / s.L[k * ns + k];
        if (lane == k) r0 = zk; else if (lane > k && lane < m) r0 = __builtin_fmaf(-zk, s.L[lane * ns + k], r0);
        if (lane + 64 == k) r1 = zk; else if (lane + 64 > k && lane + 64 < m) r1 = __builtin_fmaf(-zk, s.L[(lane + 64) * ns + k], r1);
      }
      for (int k = m - 1; k >= 0; --k) {
        const float xk = __shfl(k < 64 ? r0 : r1, k & 63, 64) / s.L[k * ns + k];
        if (lane == k) r0 = xk; else if (lane < k) r0 = __builtin_fmaf(-xk, s.L[k * ns + lane], r0);
        if (lane + 64 == k) r1 = xk; else if (lane + 64 < k) r1 = __builtin_fmaf(-xk, s.L[k * ns + lane + 64], r1);
      }
      if (lane < m) s.a[lane] = s.b[lane] - s.sw[lane] * r0;
      if (lane + 64 < m) s.a[lane + 64] = s.b[lane + 64] - s.sw[lane + 64] * r1;
    }
    __syncthreads();
    float t = 0.f;
    if (tid < m) {
      float acc = 0.f;
      for (int k = 0; k < m; ++k) acc = __builtin_fmaf(s.K[tid * ns + k], s.a[k], acc);
      s.f[tid] = acc;
      const float z = s.y[tid] > 0.5f ? -acc : acc;      // -(2y - 1) f
      t = -0.5f * s.a[tid] * acc - (fmaxf(z, 0.f) + log1pf(expf(-fabsf(z)))) - 0.5f * log1pf(s.px[tid]);      // log L_ii = 1/2 log(pivot)
    }
    const float dZ = block_sum(t - tprev, s.red);      // the rows' differences, not the difference of two totals
    Z = block_sum(t, s.red);
    tprev = t;
    if (left > 0) { if (--left == 0) { reason = PFN_GPC_CONVERGED; break; } }
    else if (it > 1 && !(dZ >= GPC_STOP * fmaxf(1.f, fabsf(Z)))) left = GPC_EXTRA;      // (a NaN counts as met: the fit ends, and is found non-finite below)
    if (it == PFN_GPC_MAX_NEWTON) break;
  }
  if (reason != PFN_GPC_NONPOSITIVE && !(fabsf(Z) < __builtin_inff())) reason = PFN_GPC_NONFINITE;
  *Z_out = Z; *iters_out = it;
  return reason;
}

__global__ void __launch_bounds__(GPC_THREADS) gpc_lml_grad_kernel(GpcArgs a) {
  extern __shared__ __attribute__((aligned(16))) float gpc_lds[];
  const int n = a.n, ns = n | 1, tid = threadIdx.x;
  const int slot = blockIdx.x, c = blockIdx.y, p = blockIdx.z;
  const GpcLds s = gpc_carve(gpc_lds, n, ns);
  const long fit = ((long)p * a.NC + c) * PFN_GPC_SLOTS + slot;
  if (slot > a.n_splits) {      // a slot this call does not use
    if (tid == 0) { a.status[fit * 2] = PFN_GPC_UNUSED; a.status[fit * 2 + 1] = 0; a.value[fit] = 0.f; a.grad[fit * 2] = 0.f; a.grad[fit * 2 + 1] = 0.f; }
    return;
  }
  const float amp = expf(a.theta[fit * 2]), len = expf(a.theta[fit * 2 + 1]), inv2l2 = 0.5f / (len * len);
  int m = 0, nq = 0, iters = 0, reason = PFN_GPC_ONE_CLASS;
  float Z = 0.f, g0 = 0.f, g1 = 0.f;
  if (gpc_stage(s, a, p, slot, ns, amp, inv2l2, &m, &nq)) reason = gpc_mode(s, m, ns, &Z, &iters);
  if (reason == PFN_GPC_CONVERGED || reason == PFN_GPC_CAPPED) {
    if (tid < m) s.r[tid] = s.y[tid] - s.pi[tid];
    __syncthreads();
    // L -> L^-1 in place, columns from the last to the first: column j of the inverse needs the inverse's columns beyond j and L's own column j
    for (int j = m - 1; j >= 0; --j) {
      const float dj = 1.f / s.L[j * ns + j];
      const int i = j + 1 + tid;
      float val = 0.f;
      if (i < m) {
        float acc = 0.f;
        for (int k = j + 1; k <= i; ++k) acc = __builtin_fmaf(s.L[i * ns + k], s.L[k * ns + j], acc);
        val = -acc * dj;
      }
      __syncthreads();
      if (i < m) s.L[i * ns + j] = val;
      if (tid == 0) s.L[j * ns + j] = dj;
      __syncthreads();
    }
    // Two identities from W^1/2 K W^1/2 = B - I keep the near-rank-one K of a long lengthscale from cancelling in f32:
    //   tr(R K) = m - tr(B^-1)   and   diag(K - C^T C) W = 1 - diag(B^-1),   so   s_2 = -1/2 (1 - diag(B^-1)) (1 - 2 pi);   C itself is never formed.
    // s_1 of theta_0: 1/2 a.f - 1/2 (m - tr(B^-1)), f = K a from the last iteration.  s_1 of theta_1: 1/2 sum (a a^T - R) * K_1 with R = W^1/2 L^-T L^-1 W^1/2
    // formed element by element and K_1 = K * 2 M.
    float p1 = 0.f;
    for (int q = tid; q < m * m; q += GPC_THREADS) {
      const int i = q / m, k = q - i * m;
      if (k <= i) {
        float acc = 0.f;
        for (int r = i; r < m; ++r) acc = __builtin_fmaf(s.L[r * ns + i], s.L[r * ns + k], acc);
        const float w = (i == k ? 0.5f : 1.f) * (s.a[i] * s.a[k] - s.sw[i] * s.sw[k] * acc);
        p1 = __builtin_fmaf(w, s.K[i * ns + k] * 2.f * s.M[i * ns + k], p1);
      }
    }
    float p0 = 0.f;
    if (tid < m) {
      // K_j (y - pi)
      float b0 = 0.f, b1 = 0.f;
      for (int k = 0; k < m; ++k) {
        const float kr = s.K[tid * ns + k] * s.r[k];
        b0 += kr;
        b1 = __builtin_fmaf(kr, 2.f * s.M[tid * ns + k], b1);
      }
      s.u0[tid] = b0; s.u1[tid] = b1;
      // 1 - (B^-1)_jj = 1 - |column j of L^-1|^2 = (pivot_j - 1) / pivot_j - sum_{r > j} (L^-1)_rj^2
      float below = 0.f;
      for (int r = tid + 1; r < m; ++r) { const float v = s.L[r * ns + tid]; below = __builtin_fmaf(v, v, below); }
      const float ex = s.px[tid], omb = ex / (1.f + ex) - below;
      s.s2[tid] = -0.5f * omb * (1.f - 2.f * s.pi[tid]);
      p0 = 0.5f * (s.a[tid] * s.f[tid] - omb);
    }
    g0 = block_sum(p0, s.red);
    g1 = block_sum(p1, s.red);      // (the barriers publish u0, u1 and s2)
    if (tid < m) {      // L^-1 W^1/2 b_j
      float t0 = 0.f, t1 = 0.f;
      for (int i = 0; i <= tid; ++i) {
        const float li = s.L[tid * ns + i] * s.sw[i];
        t0 = __builtin_fmaf(li, s.u0[i], t0);
        t1 = __builtin_fmaf(li, s.u1[i], t1);
      }
      s.t0[tid] = t0; s.t1[tid] = t1;
    }
    __syncthreads();
    if (tid < m) {      // R b_j
      float x0 = 0.f, x1 = 0.f;
      for (int r = tid; r < m; ++r) {
        const float li = s.L[r * ns + tid];
        x0 = __builtin_fmaf(li, s.t0[r], x0);
        x1 = __builtin_fmaf(li, s.t1[r], x1);
      }
      s.x0[tid] = s.sw[tid] * x0; s.x1[tid] = s.sw[tid] * x1;
    }
    __syncthreads();
    float q0 = 0.f, q1 = 0.f;
    if (tid < m) {      // s_2 . (b_j - K R b_j)
      float k0 = 0.f, k1 = 0.f;
      for (int k = 0; k < m; ++k) {
        const float kik = s.K[tid * ns + k];
        k0 = __builtin_fmaf(kik, s.x0[k], k0);
        k1 = __builtin_fmaf(kik, s.x1[k], k1);
      }
      q0 = s.s2[tid] * (s.u0[tid] - k0);
      q1 = s.s2[tid] * (s.u1[tid] - k1);
    }
    g0 += block_sum(q0, s.red);
    g1 += block_sum(q1, s.red);
    if (!(fabsf(g0) < __builtin_inff()) || !(fabsf(g1) < __builtin_inff())) reason = PFN_GPC_NONFINITE;
  }
  if (tid == 0) {
    const bool ok = reason == PFN_GPC_CONVERGED || reason == PFN_GPC_CAPPED;
    a.status[fit * 2] = reason; a.status[fit * 2 + 1] = iters;
    a.value[fit] = ok ? -Z : (reason == PFN_GPC_ONE_CLASS ? __builtin_nanf("") : __builtin_inff());
    a.grad[fit * 2] = ok ? -g0 : 0.f;
    a.grad[fit * 2 + 1] = ok ? -g1 : 0.f;
  }
}

__global__ void __launch_bounds__(GPC_THREADS) gpc_predict_kernel(GpcArgs a) {
  extern __shared__ __attribute__((aligned(16))) float gpc_lds[];
  const int n = a.n, ns = n | 1, T = a.T, F = a.F, tid = threadIdx.x;
  const int slot = blockIdx.x, c = blockIdx.y, p = blockIdx.z;
  const GpcLds s = gpc_carve(gpc_lds, n, ns);
  const long pc = (long)p * a.NC + c, fit = pc * PFN_GPC_SLOTS + slot;
  if (slot > a.n_splits) {
    if (tid == 0) { a.status[fit * 2] = PFN_GPC_UNUSED; a.status[fit * 2 + 1] = 0; }
    return;
  }
  const bool refit = slot == a.n_splits;
  const float amp = expf(a.theta[fit * 2]), len = expf(a.theta[fit * 2 + 1]), inv2l2 = 0.5f / (len * len);
  int m = 0, nq = 0, iters = 0, reason = PFN_GPC_ONE_CLASS;
  float Z = 0.f;
  if (gpc_stage(s, a, p, slot, ns, amp, inv2l2, &m, &nq)) reason = gpc_mode(s, m, ns, &Z, &iters);
  const bool ok = reason == PFN_GPC_CONVERGED || reason == PFN_GPC_CAPPED;
  if (tid == 0) { a.status[fit * 2] = reason; a.status[fit * 2 + 1] = iters; }
  if (tid < m) s.r[tid] = s.y[tid] - s.pi[tid];
  __syncthreads();      // K and M are free from here: together they hold up to 2 n query rows of exponent arguments at the stride ns
  const float* xtr = a.train + (long)p * n * F;
  const float* xte = a.test + (long)p * T * F;
  float* Q = s.K;
  const int total = refit ? T : nq, chunk = 2 * n;
  for (int q0 = 0; q0 < total; q0 += chunk) {
    const int nc = min(chunk, total - q0);
    if (ok) {
      for (int w = tid; w < nc * m; w += GPC_THREADS) {
        const int q = w / m, i = w - q * m;
        const float* xq = refit ? xte + (long)(q0 + q) * F : xtr + (long)s.qidx[q0 + q] * F;
        Q[q * ns + i] = gpc_arg(xq, xtr + (long)s.idx[i] * F, F, inv2l2);
      }
    }
    __syncthreads();
    if (tid < nc) {
      float* row = Q + tid * ns;
      float mval = __builtin_nanf(""), e = __builtin_nanf(""), var = __builtin_nanf("");
      if (ok) {
        e = row[0];
        for (int i = 1; i < m; ++i) e = fminf(e, row[i]);
        mval = 0.f;
        for (int i = 0; i < m; ++i) mval = __builtin_fmaf(amp * expf(e - row[i]), s.r[i], mval);
        if (refit) {      // |L^-1 W^1/2 k*|^2 by forward substitution over the row
          float ss = 0.f;
          for (int k = 0; k < m; ++k) {
            float acc = s.sw[k] * amp * expf(-row[k]);
            for (int j = 0; j < k; ++j) acc = __builtin_fmaf(-s.L[k * ns + j], row[j], acc);
            const float vk = acc / s.L[k * ns + k];
            row[k] = vk;
            ss = __builtin_fmaf(vk, vk, ss);
          }
          var = fmaxf(amp - ss, 0.f);
        }
      }
      if (refit) {
        a.test_f[(pc * T + q0 + tid) * 2] = mval; a.test_f[(pc * T + q0 + tid) * 2 + 1] = e;
        a.test_var[pc * T + q0 + tid] = var;
      } else {
        const long o = (pc * n + s.qidx[q0 + tid]) * 2;
        a.cv_f[o] = mval; a.cv_f[o + 1] = e;
      }
    }
    __syncthreads();
  }
}

int launch_gpc_lml_grad(const GpcArgs& a, hipStream_t s) {
  static LdsAllowance allowance;
  return launch_lds(gpc_lml_grad_kernel, allowance, dim3(PFN_GPC_SLOTS, (unsigned)a.NC, (unsigned)a.P), dim3(GPC_THREADS), gpc_lds_bytes(a.n), s, a);
}

int launch_gpc_predict(const GpcArgs& a, hipStream_t s) {
  static LdsAllowance allowance;
  return launch_lds(gpc_predict_kernel, allowance, dim3(PFN_GPC_SLOTS, (unsigned)a.NC, (unsigned)a.P), dim3(GPC_THREADS), gpc_lds_bytes(a.n), s, a);
}

int gpc_shapes(const char* what, int P, int n, int T, int F, int NC, int n_splits, bool pointers) {
  return fold_shapes(what, "one block per fit, three n x n matrices in LDS", P, n, PFN_GPC_MAX_N, T, F, NC, PFN_GPC_MAX_CANDIDATES, n_splits, PFN_GPC_FOLDS, pointers);
}

}  // namespace
}  // namespace pfn

using namespace pfn;

extern "C" {
int pfn_gpc_lml_grad(const float* theta, const float* train, const float* labels, const int32_t* fold, int P, int n, int F, int NC, int n_splits, float* value,
                     float* grad, int32_t* status, void* stream) {
  if (const int rc = gpc_shapes("gpc_lml_grad", P, n, 1, F, NC, n_splits, theta && train && labels && fold && value && grad && status)) return rc;
  GpcArgs a{};
  a.theta = theta; a.train = train; a.labels = labels; a.fold = fold; a.P = P; a.n = n; a.T = 1; a.F = F; a.NC = NC; a.n_splits = n_splits; a.value = value; a.grad = grad;
  a.status = status;
  PFN_TRY(launch_gpc_lml_grad(a, (hipStream_t)stream));
  return PFN_OK;
}
int pfn_gpc_predict(const float* theta, const float* train, const float* labels, const float* test, const int32_t* fold, int P, int n, int T, int F, int NC, int n_splits,
                    float* cv_f, float* test_f, float* test_var, int32_t* status, void* stream) {
  if (const int rc = gpc_shapes("gpc_predict", P, n, T, F, NC, n_splits, theta && train && labels && test && fold && cv_f && test_f && test_var && status)) return rc;
  GpcArgs a{};
  a.theta = theta; a.train = train; a.labels = labels; a.test = test; a.fold = fold; a.P = P; a.n = n; a.T = T; a.F = F; a.NC = NC; a.n_splits = n_splits; a.cv_f = cv_f;
  a.test_f = test_f; a.test_var = test_var; a.status = status;
  PFN_TRY(launch_gpc_predict(a, (hipStream_t)stream));
  return PFN_OK;
}
}  // extern "C"
