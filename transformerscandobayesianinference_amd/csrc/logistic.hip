// The tabular study's logistic-regression baseline with its grid search (reference tabular.py:325-346; DESIGN.md section 20, include/pfn_hip.h "Logistic
// regression"): logit_cv_kernel fits every (problem, candidate, fold slot) of a call in one launch, one block of 256 threads per fit.
//   objective   C sum_i m_i softplus(-y_i z_i) + r(w),  z = x w + b,  r = 1/2 |w|^2 (l2), |w|_1 (l1), 0 (none: C = 1);  the intercept is never penalised
//   solver      proximal Newton from w = 0: gradient, H = C X^T D X (+ I on the penalised coordinates for l2) + damping in LDS, direction by an in-LDS Cholesky
//               solve (l2, none) or by cyclic coordinate descent with soft-thresholding on the quadratic model (l1), Armijo backtracking on the true objective
//   stop        KKT_inf <= 64 2^-23 C max_j sum_i m_i |x_ij|, or no decrease, or the iteration cap; every loop has a constant cap and a NaN leaves every
//               comparison towards "stop"
// No global atomics, no workspace, no communication between blocks: a fit is a bitwise function of its own problem and candidate.
#include "fold_device.h"

namespace pfn {

struct LogitCvArgs {
  const float* train;        // [P,n,F]
  const float* labels;       // [P,n]: class = label > 0.5
  const float* test;         // [P,T,F]
  const int32_t* fold;       // [P,n]: the CV test fold of each train row
  const float* cand_C;       // [NC]
  const int32_t* cand_kind;  // [NC]: penalty code | PFN_LOGIT_FIT_INTERCEPT
  int P, n, T, F, NC, n_splits;
  int32_t* cv_correct;       // [P,NC,5]
  float* test_z;             // [P,NC,T]
  int32_t* status;           // [P,NC,6,2] = (exit reason, iterations)
  float* coef;               // [P,NC,6,F+1] or null
};
// the n rows at an odd stride of (F + 1) | 1 floats (features, then a column of ones), H [F+1] rows at the same stride, six vectors over the rows, five over
// the coordinates, eight words of reduction space: 138,296 bytes at n = F = 128, 37,576 at the study's n = 80, F = 60
inline size_t logit_cv_lds_bytes(int n, int F) { return ((size_t)(n + F + 1) * ((F + 1) | 1) + 6 * (size_t)n + 5 * (size_t)(F + 1) + 8) * 4; }

namespace {

#define LOGIT_DEV __device__ __forceinline__

constexpr int LOGIT_THREADS = 256;
constexpr int LOGIT_MAX_OUTER = 48;        // proximal-Newton iterations
constexpr int LOGIT_MAX_SWEEPS = 50;       // coordinate-descent sweeps per l1 direction
constexpr int LOGIT_MAX_BACKTRACKS = 30;   // step 1, 1/2, ... 2^-29
constexpr float LOGIT_EPS = 1.1920929e-07f;      // 2^-23
constexpr float LOGIT_DAMP = 1.52587890625e-05f; // 2^-16 of the mean diagonal: changes steps, never the optimum
constexpr float LOGIT_ARMIJO = 1e-4f;

// the block maximum, a reduction like block_sum (fold_device.h): every thread calls; the result is the same bits in every thread
LOGIT_DEV float block_max(float v, float* red) {      // a NaN in any lane comes out as NaN (so that the caller's comparison stops)
  bool bad = v != v;
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  bad = __any(bad);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bad ? __builtin_nanf("") : v;
  __syncthreads();
  const float a = red[0], b = red[1], c = red[2], e = red[3];
  if (a != a || b != b || c != c || e != e) return __builtin_nanf("");
  return fmaxf(fmaxf(a, b), fmaxf(c, e));
}

// one of three registers by a wave-uniform index
LOGIT_DEV float pick3(int r, float a, float b, float c) { return r == 0 ? a : (r == 1 ? b : c); }

// row i of the staged table times v[0 .. d): an fma chain in ascending column order
LOGIT_DEV float row_dot(const float* row, const float* v, int d) {
  float acc = 0.f;
  for (int j = 0; j < d; ++j) acc = __builtin_fmaf(row[j], v[j], acc);
  return acc;
}

__global__ void __launch_bounds__(LOGIT_THREADS) logit_cv_kernel(LogitCvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float logit_lds[];
  const int n = a.n, T = a.T, F = a.F, tid = threadIdx.x, lane = tid & 63;
  const int s = blockIdx.x, c = blockIdx.y, p = blockIdx.z;
  const int kind = a.cand_kind[c], penalty = kind & 3, icpt = (kind >> 2) & 1;
  const float C = penalty == PFN_LOGIT_NONE ? 1.f : a.cand_C[c];
  const int d = F + icpt, Xs = (F + 1) | 1, Hs = Xs;
  float* X = logit_lds;              // [n][Xs]: the features, then a column of ones
  float* H = X + n * Xs;             // [F+1][Hs]
  float* ys = H + (F + 1) * Hs;      // [n] +1 / -1
  float* msk = ys + n;               // [n] 1 on the training rows of this fit
  float* sig = msk + n;              // [n] sigma(-y z)
  float* cg = sig + n;               // [n] the row's gradient weight  -C m y sigma
  float* Dw = cg + n;                // [n] the row's curvature weight  C m sigma (1 - sigma)
  float* xd = Dw + n;                // [n] x . delta
  float* w = xd + n;                 // [F+1]
  float* g = w + (F + 1);            // [F+1] gradient of the smooth part (the l2 term included)
  float* dl = g + (F + 1);           // [F+1] direction
  float* act = dl + (F + 1);         // [F+1] 1 where the column is not zero on every training row
  float* wn = act + (F + 1);         // [F+1] trial point
  float* red = wn + (F + 1);         // [8]

  const long fit = ((long)p * a.NC + c) * PFN_LOGIT_SLOTS + s;
  int32_t* status = a.status + fit * 2;
  float* coef = a.coef ? a.coef + fit * (F + 1) : nullptr;
  int32_t* cvc = s < PFN_LOGIT_FOLDS ? a.cv_correct + ((long)p * a.NC + c) * PFN_LOGIT_FOLDS + s : nullptr;
  if (s > a.n_splits) {      // a slot this call does not use
    if (tid == 0) { status[0] = PFN_LOGIT_UNUSED; status[1] = 0; if (cvc) *cvc = 0; }
    if (coef) for (int j = tid; j <= F; j += LOGIT_THREADS) coef[j] = 0.f;
    return;
  }
  const bool refit = s == a.n_splits;

  // ---- stage ----
  const float* xtr = a.train + (long)p * n * F;
  for (int i = tid; i < n * F; i += LOGIT_THREADS) {
    const int r = i / F, f = i - r * F;
    X[r * Xs + f] = xtr[i];
  }
  for (int i = tid; i < n; i += LOGIT_THREADS) {
    X[i * Xs + F] = 1.f;
    ys[i] = a.labels[(long)p * n + i] > 0.5f ? 1.f : -1.f;
    msk[i] = (refit || a.fold[(long)p * n + i] != s) ? 1.f : 0.f;
  }
  for (int j = tid; j <= F; j += LOGIT_THREADS) { w[j] = 0.f; dl[j] = 0.f; }
  __syncthreads();
  const int npos = __syncthreads_count(tid < n && msk[tid] != 0.f && ys[tid] > 0.f);
  const int nneg = __syncthreads_count(tid < n && msk[tid] != 0.f && ys[tid] < 0.f);

  int reason = PFN_LOGIT_ONE_CLASS, iters = 0;
  if (npos > 0 && nneg > 0) {
    // the columns' training mass: the scale of the stopping rule, and which columns are alive
    float colmass = 0.f;
    if (tid < d) {
      for (int i = 0; i < n; ++i) colmass += msk[i] * fabsf(X[i * Xs + tid]);
      act[tid] = colmass > 0.f ? 1.f : 0.f;
    }
    const float thr = 64.f * LOGIT_EPS * C * block_max(colmass, red);
    reason = PFN_LOGIT_CAPPED;
    bool polished = false;
    for (int it = 0;; ++it) {
      // rows: margin, sigma and the two weights
      float arg = 0.f;
      if (tid < n) {
        const float z = row_dot(X + tid * Xs, w, d);
        arg = -ys[tid] * z;
        const float e = expf(-fabsf(arg)), hi = 1.f / (1.f + e), lo = e * hi;      // sigma(|arg|), sigma(-|arg|)
        const float pr = arg >= 0.f ? hi : lo;
        sig[tid] = pr;
        cg[tid] = -C * msk[tid] * ys[tid] * pr;
        Dw[tid] = C * msk[tid] * (hi * lo);
      }
      __syncthreads();
      // columns: gradient, curvature, KKT residual (the minimum-norm subgradient)
      float kkt = 0.f, hjj = 0.f;
      if (tid < d) {
        float gj = 0.f;
        if (act[tid] != 0.f) {
          for (int i = 0; i < n; ++i) {
            const float x = X[i * Xs + tid];
            gj = __builtin_fmaf(cg[i], x, gj);
            hjj = __builtin_fmaf(Dw[i] * x, x, hjj);
          }
          const bool pen = tid < F;
          const float wj = w[tid];
          if (penalty == PFN_LOGIT_L2 && pen) { gj += wj; hjj += 1.f; }
          if (penalty == PFN_LOGIT_L1 && pen) kkt = wj != 0.f ? fabsf(gj + (wj > 0.f ? 1.f : -1.f)) : fmaxf(fabsf(gj) - 1.f, 0.f);
          else kkt = fabsf(gj);
          if (gj != gj) kkt = gj;
        } else {
          hjj = 1.f;
        }
        g[tid] = gj;
      }
      const float kkt_inf = block_max(kkt, red);
      iters = it;
      // without a penalty, a w that separates the training rows proves that no optimum exists: its small residual certifies nothing and the fit goes on to the cap
      const bool separates = penalty == PFN_LOGIT_NONE && __syncthreads_count(tid < n && msk[tid] != 0.f && !(arg < 0.f)) == 0;
      const bool met = kkt_inf <= thr && !separates;
      if (!(kkt_inf > thr) && !(kkt_inf <= thr)) { reason = PFN_LOGIT_NONFINITE; break; }
      // the first iterate that meets the threshold is followed by one more Newton step (the residual falls quadratically there: the step costs one iteration and
      // leaves the coefficients at the precision's floor, not at the threshold); the fit ends at the next iterate that meets it
      if (met && polished) { reason = PFN_LOGIT_CONVERGED; break; }
      polished = met;
      if (it == LOGIT_MAX_OUTER) { if (met) reason = PFN_LOGIT_CONVERGED; break; }
      // damping where H can be singular (l1, none); under l2 it is positive definite as it stands, and its intercept's curvature (of the order C n) can be far
      // below the mean diagonal, so that a damping by the trace would stall that coordinate
      const float tau = penalty == PFN_LOGIT_L2 ? 0.f : LOGIT_DAMP * block_sum(hjj, red) / (float)d;
      const float pivot_floor = fmaxf(tau, 1e-30f);

      // H = C X^T D X (+ I) + tau I: 4 x 4 tiles of the lower triangle, written to both halves
      {
        const int nt = (d + 3) >> 2, pairs = nt * (nt + 1) / 2;
        for (int q = tid; q < pairs; q += LOGIT_THREADS) {
          int ti = 0;
          while ((ti + 1) * (ti + 2) / 2 <= q) ++ti;
          const int tj = q - ti * (ti + 1) / 2;
          int ca[4], cb[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) { ca[u] = min(4 * ti + u, d - 1); cb[u] = min(4 * tj + u, d - 1); }
          float acc[4][4];
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;
          for (int i = 0; i < n; ++i) {
            const float* row = X + i * Xs;
            const float dw = Dw[i];
            float xa[4], xb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { xa[u] = dw * row[ca[u]]; xb[u] = row[cb[u]]; }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
              for (int v = 0; v < 4; ++v) acc[u][v] = __builtin_fmaf(xa[u], xb[v], acc[u][v]);
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const int ra = 4 * ti + u, rb = 4 * tj + v;
              if (ra < d && rb < d && rb <= ra) {
                float h = acc[u][v];
                if (ra == rb) {
                  if (act[ra] == 0.f) h = 1.f;      // a dead column: its own unit pivot, nothing is divided by its curvature
                  else h += tau + ((penalty == PFN_LOGIT_L2 && ra < F) ? 1.f : 0.f);
                }
                H[ra * Hs + rb] = h;
                H[rb * Hs + ra] = h;
              }
            }
        }
      }
      __syncthreads();

      if (penalty != PFN_LOGIT_L1) {
        // in-place Cholesky of the lower triangle (right-looking), a pivot never below the damping (a NaN pivot too becomes the floor)
        for (int k = 0; k < d; ++k) {
          float piv = H[k * Hs + k];
          if (!(piv > pivot_floor)) piv = pivot_floor;
          const float root = sqrtf(piv), inv = 1.f / root;
          __syncthreads();      // every thread has read the pivot
          const int m = d - k - 1;
          if (tid == 0) H[k * Hs + k] = root;
          for (int i = tid; i < m; i += LOGIT_THREADS) H[(k + 1 + i) * Hs + k] *= inv;
          __syncthreads();
          for (int q = tid; q < m * m; q += LOGIT_THREADS) {
            const int i = q / m, j = q - i * m;
            if (j <= i) H[(k + 1 + i) * Hs + (k + 1 + j)] -= H[(k + 1 + i) * Hs + k] * H[(k + 1 + j) * Hs + k];
          }
          __syncthreads();
        }
        // L y = -g, L^T delta = y: wave 0, coordinate lane + 64 r in register r
        if (tid < 64) {
          float r0 = lane < d ? -g[lane] : 0.f, r1 = lane + 64 < d ? -g[lane + 64] : 0.f, r2 = lane + 128 < d ? -g[lane + 128] : 0.f;
          for (int k = 0; k < d; ++k) {
            const float yk = __shfl(pick3(k >> 6, r0, r1, r2), k & 63, 64) / H[k * Hs + k];
            if (lane == k) r0 = yk; else if (lane > k && lane < d) r0 = __builtin_fmaf(-yk, H[lane * Hs + k], r0);
            if (lane + 64 == k) r1 = yk; else if (lane + 64 > k && lane + 64 < d) r1 = __builtin_fmaf(-yk, H[(lane + 64) * Hs + k], r1);
            if (lane + 128 == k) r2 = yk; else if (lane + 128 > k && lane + 128 < d) r2 = __builtin_fmaf(-yk, H[(lane + 128) * Hs + k], r2);
          }
          for (int k = d - 1; k >= 0; --k) {
            const float xk = __shfl(pick3(k >> 6, r0, r1, r2), k & 63, 64) / H[k * Hs + k];
            if (lane == k) r0 = xk; else if (lane < k) r0 = __builtin_fmaf(-xk, H[k * Hs + lane], r0);
            if (lane + 64 == k) r1 = xk; else if (lane + 64 < k) r1 = __builtin_fmaf(-xk, H[k * Hs + lane + 64], r1);
            if (lane + 128 == k) r2 = xk; else if (lane + 128 < k) r2 = __builtin_fmaf(-xk, H[k * Hs + lane + 128], r2);
          }
          if (lane < d) dl[lane] = act[lane] != 0.f ? r0 : 0.f;
          if (lane + 64 < d) dl[lane + 64] = act[lane + 64] != 0.f ? r1 : 0.f;
          if (lane + 128 < d) dl[lane + 128] = act[lane + 128] != 0.f ? r2 : 0.f;
        }
      } else if (tid < 64) {
        // cyclic coordinate descent on  g.delta + 1/2 delta H delta + |w + delta|_1:  wave 0 keeps q = H delta in registers, one column axpy per change
        // (and delta too, coordinate lane + 64 r in register r; LDS is only read)
        float q0 = 0.f, q1 = 0.f, q2 = 0.f, e0 = 0.f, e1 = 0.f, e2 = 0.f;
        for (int sweep = 0; sweep < LOGIT_MAX_SWEEPS; ++sweep) {
          float moved = 0.f;
          bool bad = false;
          for (int j = 0; j < d; ++j) {
            if (act[j] == 0.f) continue;
            const int r = j >> 6, src = j & 63;
            const float hj = H[j * Hs + j], wj = w[j], cur = wj + __shfl(pick3(r, e0, e1, e2), src, 64);
            const float G = g[j] + __shfl(pick3(r, q0, q1, q2), src, 64);
            const float v = cur - G / hj, th = 1.f / hj;
            float u = v;
            if (j < F) u = v > th ? v - th : (v < -th ? v + th : 0.f);
            const float dz = u - cur;
            if (dz != 0.f) {      // (the same in every lane)
              const float dj = u - wj;
              if (lane == src) { if (r == 0) e0 = dj; else if (r == 1) e1 = dj; else e2 = dj; }
              if (lane < d) q0 = __builtin_fmaf(dz, H[j * Hs + lane], q0);
              if (lane + 64 < d) q1 = __builtin_fmaf(dz, H[j * Hs + lane + 64], q1);
              if (lane + 128 < d) q2 = __builtin_fmaf(dz, H[j * Hs + lane + 128], q2);
            }
            moved = fmaxf(moved, fabsf(dz) * hj);
            bad = bad || dz != dz;
          }
          if (bad || !(moved > 0.25f * thr)) break;
        }
        if (lane < d) dl[lane] = e0;
        if (lane + 64 < d) dl[lane + 64] = e1;
        if (lane + 128 < d) dl[lane + 128] = e2;
      }
      __syncthreads();

      // the model's decrease and the rows' x . delta
      float part = 0.f;
      if (tid < d) {
        const float dj = dl[tid];
        part = g[tid] * dj;
        if (penalty == PFN_LOGIT_L1 && tid < F) part += fabsf(w[tid] + dj) - fabsf(w[tid]);
      }
      if (tid < n) xd[tid] = row_dot(X + tid * Xs, dl, d);
      const float model = block_sum(part, red);      // (its barriers publish xd)
      bool moved_on = false;
      if (model < 0.f) {
        float t = 1.f;
        for (int bt = 0; bt < LOGIT_MAX_BACKTRACKS; ++bt, t *= 0.5f) {
          // objective(w + t delta) - objective(w), term by term without cancellation:
          //   softplus(b) - softplus(a) = log1p(sigma(a) expm1(b - a));  the penalties' differences in closed form
          float df = 0.f;
          if (tid < n && msk[tid] != 0.f) df = C * log1pf(sig[tid] * expm1f(-ys[tid] * t * xd[tid]));
          if (tid < d) {
            const float wj = w[tid], dj = dl[tid], nw = __builtin_fmaf(t, dj, wj);
            wn[tid] = nw;
            if (tid < F) {
              if (penalty == PFN_LOGIT_L2) df += t * dj * (wj + 0.5f * t * dj);
              if (penalty == PFN_LOGIT_L1) df += (wj != 0.f && (nw > 0.f) == (wj > 0.f) && nw != 0.f) ? (wj > 0.f ? t * dj : -t * dj) : fabsf(nw) - fabsf(wj);
            }
          }
          const float dfs = block_sum(df, red);
          if (dfs <= LOGIT_ARMIJO * t * model) { moved_on = true; break; }
        }
      }
      if (!moved_on) { reason = met ? PFN_LOGIT_CONVERGED : PFN_LOGIT_STALLED; break; }
      if (tid < d) w[tid] = wn[tid];
      __syncthreads();
    }
  }
  __syncthreads();

  // ---- outputs ----
  if (tid == 0) { status[0] = reason; status[1] = iters; }
  if (coef) for (int j = tid; j <= F; j += LOGIT_THREADS) coef[j] = j < d ? w[j] : 0.f;
  const bool ran = reason != PFN_LOGIT_ONE_CLASS;
  if (!refit) {
    bool ok = false;
    if (ran && tid < n && msk[tid] == 0.f) {
      const float z = row_dot(X + tid * Xs, w, d);
      ok = (z > 0.f) == (ys[tid] > 0.f);      // z == 0 predicts class 0
    }
    const int count = __syncthreads_count(ok);
    if (tid == 0) *cvc = count;
  } else {
    if (tid == 0 && cvc) *cvc = 0;
    const float* xte = a.test + (long)p * T * F;
    float* tz = a.test_z + ((long)p * a.NC + c) * T;
    for (int t = tid; t < T; t += LOGIT_THREADS) {
      float acc = 0.f;
      for (int j = 0; j < F; ++j) acc = __builtin_fmaf(xte[(long)t * F + j], w[j], acc);
      if (icpt) acc += w[F];
      tz[t] = ran ? acc : __builtin_nanf("");
    }
  }
}

int launch_logit_cv(const LogitCvArgs& a, hipStream_t s) {
  static LdsAllowance allowance;
  return launch_lds(logit_cv_kernel, allowance, dim3(PFN_LOGIT_SLOTS, (unsigned)a.NC, (unsigned)a.P), dim3(LOGIT_THREADS), logit_cv_lds_bytes(a.n, a.F), s, a);
}

}  // namespace
}  // namespace pfn

using namespace pfn;

extern "C" int pfn_logistic_cv(const float* train, const float* labels, const float* test, const int32_t* fold, const float* cand_C, const int32_t* cand_kind, int P,
                               int n, int T, int F, int NC, int n_splits, int32_t* cv_correct, float* test_z, int32_t* status, float* coef, void* stream) {
  if (const int rc = fold_shapes("logistic_cv", "one block per fit, its rows and its Hessian in LDS", P, n, 128, T, F, NC, PFN_LOGIT_MAX_CANDIDATES, n_splits, PFN_LOGIT_FOLDS,
                                 train && labels && test && fold && cand_C && cand_kind && cv_correct && test_z && status)) return rc;      // (coef may be NULL)
  LogitCvArgs a{};
  a.train = train; a.labels = labels; a.test = test; a.fold = fold; a.cand_C = cand_C; a.cand_kind = cand_kind; a.P = P; a.n = n; a.T = T; a.F = F; a.NC = NC;
  a.n_splits = n_splits; a.cv_correct = cv_correct; a.test_z = test_z; a.status = status; a.coef = coef;
  PFN_TRY(launch_logit_cv(a, (hipStream_t)stream));
  return PFN_OK;
}
