// The tabular study's Bayesian-neural-network baseline with its grid search (reference tabular.py:372-478, `bayes_net_metric`; DESIGN.md section 23,
// include/pfn_hip.h "BNN classifier with its grid search"): bnn_cv_kernel runs the SVI steps and the predictive of every (problem, candidate, fold slot) of a
// call in one launch, one block of 256 threads per fit.  The model and the step are those of pfn_bnn_svi_steps at activation = 0 with one particle:
//   theta = loc + softplus(u) eps,  o = W2 (W1 x + b1) + b2,  U = |theta|^2 / 2 + (D / 2) log 2 pi + sum_i m_i softplus(-+(o_1 - o_0))
// The model is linear in x, and the kernel uses that: with v = W2[1] - W2[0],
//   o_1 - o_0 = x . (W1^T v) + v . b1 + (b2[1] - b2[0]),   g_i = m_i (sigma - y_i),   r = X^T g,   G = sum g,
//   dU/dW1[j,f] = v_j r_f + W1[j,f],  dU/db1[j] = v_j G + b1[j],  dU/dW2[1,j] = A_j + W2[1,j],  dU/dW2[0,j] = -A_j + W2[0,j],  A_j = W1[j] . r + b1[j] G,
//   dU/db2[1] = G + b2[1],  dU/db2[0] = -G + b2[0]:
// O(H F + n F) multiply-adds per step and never the n x H hidden matrix.  Every sum over rows, features or hidden units is accumulated in f64 and rounded
// once; the transcendental parts are f32.
// Where things live: the fit's train rows [n][F | 1], one theta and one eps in LDS; the six state rows stay in global memory and are streamed, Philox block
// by Philox block (four coordinates), by the thread that owns the block -- the same thread in every step and in the predictive, so a launch needs no fence
// and a split run is the unsplit one.  One regime for every D: six rows of D = 8386 are 200 KB and fit nowhere else.
// No global atomics, no workspace, no communication between blocks: a fit is a bitwise function of its own problem, candidate and slot.
#include "bnn_device.h"
#include "fold_device.h"

namespace pfn {

struct BnnCvArgs {
  const float* train;        // [P,n,F]
  const float* labels;       // [P,n]: class = label > 0.5
  const float* test;         // [P,T,F]
  const int32_t* fold;       // [P,n]: the CV test fold of each train row
  int P, n, T, F, NC, n_splits;
  float* state;              // [P,NC,6,6,ld]
  long ld, step0;
  int num_steps, S;          // S predictive draws
  float beta1, beta2, eps;
  unsigned long long seed;
  const int64_t* problem_ids;      // [P] or null
  float* loss;               // [P,NC,6,num_steps] or null
  float* cv_prob;            // [P,NC,n]
  float* test_prob;          // [P,NC,T]
  float* cv_draw;            // [P,NC,n] or null
  float* test_draw;          // [P,NC,T] or null
  int32_t* status;           // [P,NC,6]
  int H[PFN_BNN_CV_MAX_CANDIDATES];      // the candidates, by value: the entry point takes them as host arrays
  float lr[PFN_BNN_CV_MAX_CANDIDATES];
};
// eight doubles of reduction space, max(n, T) rows at an odd stride of F | 1 floats, theta and eps (D rounded up to whole Philox blocks), v and A over the
// hidden units, w and r over the features, two vectors over the rows, the logit's constant: 135,792 bytes at n = T = F = 128, H = 64; 53,520 at the study's
// n = 80, T = 20, F = 60, H = 64
inline size_t bnn_cv_lds_bytes(int n, int T, int F, int H) {
  const size_t Dp = ((size_t)H * (F + 3) + 2 + 3) & ~(size_t)3;
  return (16 + (size_t)(n > T ? n : T) * (F | 1) + 2 * Dp + 2 * (size_t)H + 2 * (size_t)F + 2 * (size_t)n + 4) * 4;
}
static_assert((16 + 128 * 129 + 2 * ((64 * 131 + 2 + 3) & ~3) + 2 * 64 + 2 * 128 + 2 * 128 + 4) * 4 <= 160 * 1024, "bnn_cv: LDS");

namespace {

constexpr int CV_THREADS = 256;
constexpr unsigned long long CV_PRED_DOMAIN = 1ull << 41, CV_OBS_DOMAIN = 1ull << 42;      // the counters of the predictive's draws and of its observation uniforms

PFN_DEV float cv_softplus(float u) { return fmaxf(u, 0.f) + log1pf(expf(-fabsf(u))); }
PFN_DEV bool cv_finite(float x) { return fabsf(x) < __builtin_inff(); }

// two block sums at once, in f64: every thread calls; the results are the same bits in every thread.  red: 8 doubles of LDS
PFN_DEV void block_sum2(double& x, double& y, double* red) {
  for (int o = 32; o > 0; o >>= 1) { x += __shfl_xor(x, o, 64); y += __shfl_xor(y, o, 64); }
  __syncthreads();      // the previous use of red is over
  if ((threadIdx.x & 63) == 0) { red[2 * (threadIdx.x >> 6)] = x; red[2 * (threadIdx.x >> 6) + 1] = y; }
  __syncthreads();
  x = (red[0] + red[2]) + (red[4] + red[6]);
  y = (red[1] + red[3]) + (red[5] + red[7]);
}

// dU/dtheta_i from the step's vectors; th = theta_i (the prior's term)
PFN_DEV float cv_grad(int i, int H, int F, float th, const float* v, const float* r, const float* A, float G) {
  int k = i - H * F;
  if (k < 0) { const int j = i / F; return __builtin_fmaf(v[j], r[i - j * F], th); }
  if (k < H) return __builtin_fmaf(v[k], G, th);
  k -= H;
  if (k < H) return th - A[k];
  k -= H;
  if (k < H) return th + A[k];
  return k == H ? th - G : th + G;
}

// from theta in LDS: v = W2[1] - W2[0], w = W1^T v, cs[0] = v . b1 + b2[1] - b2[0].  The caller's barrier follows.
PFN_DEV void cv_collapse(const float* th, int H, int F, float* v, float* w, float* cs) {
  const int tid = threadIdx.x, oB1 = H * F, oW2 = oB1 + H, oB2 = oW2 + 2 * H;
  if (tid < H) v[tid] = th[oW2 + H + tid] - th[oW2 + tid];
  if (tid < F) {
    double acc = 0.;
    for (int j = 0; j < H; ++j) acc = __builtin_fma((double)th[j * F + tid], (double)(th[oW2 + H + j] - th[oW2 + j]), acc);
    w[tid] = (float)acc;
  } else if (tid == CV_THREADS - 1) {      // (F <= 128: never a feature's thread)
    double acc = 0.;
    for (int j = 0; j < H; ++j) acc = __builtin_fma((double)th[oB1 + j], (double)(th[oW2 + H + j] - th[oW2 + j]), acc);
    cs[0] = (float)(acc + (double)(th[oB2 + 1] - th[oB2]));
  }
}

// x . w + c for the row at `row`
PFN_DEV float cv_logit(const float* row, const float* w, int F, float c) {
  double acc = 0.;
  for (int f = 0; f < F; ++f) acc = __builtin_fma((double)row[f], (double)w[f], acc);
  return (float)(acc + (double)c);
}

__global__ void __launch_bounds__(CV_THREADS) bnn_cv_kernel(BnnCvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float cv_lds[];
  const int n = a.n, T = a.T, F = a.F, tid = threadIdx.x;
  const int s = blockIdx.x, c = blockIdx.y, p = blockIdx.z;
  const long pc = (long)p * a.NC + c, fit = pc * PFN_BNN_CV_SLOTS + s;
  if (s > a.n_splits) {      // a slot this call does not use
    if (tid == 0) a.status[fit] = PFN_BNN_CV_UNUSED;
    return;
  }
  const int H = a.H[c], D = H * (F + 3) + 2, Dp = (D + 3) & ~3, nblk = Dp >> 2, Xs = F | 1;
  const float lr = a.lr[c];
  double* red = reinterpret_cast<double*>(cv_lds);      // [8]
  float* X = cv_lds + 16;                // [max(n, T)][Xs]
  float* th = X + (n > T ? n : T) * Xs;  // [Dp] theta
  float* ep = th + Dp;                   // [Dp] eps of the step; the scale during the predictive
  float* v = ep + Dp;                    // [H]
  float* A = v + H;                      // [H]
  float* w = A + H;                      // [F]
  float* r = w + F;                      // [F]
  float* gv = r + F;                     // [n] g_i
  float* mk = gv + n;                    // [n] 1 on the training rows of this fit
  float* cs = mk + n;                    // [1]
  const bool refit = s == a.n_splits;
  float* st = a.state + fit * 6 * a.ld;
  const long ld = a.ld;
  const unsigned long long q = (a.problem_ids ? (unsigned long long)a.problem_ids[p] : (unsigned long long)p) * 8ull + (unsigned long long)s;

  // ---- stage ----
  const float* xtr = a.train + (long)p * n * F;
  for (int i = tid; i < n * F; i += CV_THREADS) {
    const int row = i / F, f = i - row * F;
    X[row * Xs + f] = xtr[i];
  }
  bool y1 = false, trains = false, held = false;      // of the thread's row
  if (tid < n) {
    const int fo = a.fold[(long)p * n + tid];
    y1 = a.labels[(long)p * n + tid] > 0.5f;
    trains = refit || fo != s;
    held = !refit && fo == s;
    mk[tid] = trains ? 1.f : 0.f;
  }
  bool bad = false;
  __syncthreads();

  // ---- the steps ----
  for (int it = 0; it < a.num_steps; ++it) {
    const unsigned long long t = (unsigned long long)a.step0 + it;
    double part = 0.;      // the thread's share of L = sum_i [theta_i^2 / 2 - eps_i^2 / 2 - log scale_i] + sum_rows softplus
    for (int b = tid; b < nblk; b += CV_THREADS) {
      float z[4];
      normal4(philox4x32_10((t << 12) | (unsigned)b, q, a.seed), z);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = 4 * b + e;
        if (i < D) {
          const float sc = cv_softplus(st[ld + i]), x = __builtin_fmaf(sc, z[e], st[i]);
          th[i] = x;
          ep[i] = z[e];
          part += (double)(0.5f * (x * x - z[e] * z[e]) - logf(sc));
        }
      }
    }
    __syncthreads();
    cv_collapse(th, H, F, v, w, cs);
    __syncthreads();
    double gsum = 0.;
    if (tid < n) {
      float g = 0.f;
      if (trains) {
        const float d = cv_logit(X + tid * Xs, w, F, cs[0]);
        const float zz = y1 ? -d : d;      // -log softmax(o)[y] = softplus(zz)
        const float e = expf(-fabsf(zz));
        part += (double)(fmaxf(zz, 0.f) + log1pf(e));
        const float sg = bnn_sigmoid(zz, e);
        g = y1 ? -sg : sg;
      }
      gv[tid] = g;
      gsum = (double)g;
    }
    block_sum2(part, gsum, red);      // (its barriers publish gv)
    const float G = (float)gsum;
    if (tid < F) {
      double acc = 0.;
      for (int i = 0; i < n; ++i)
        if (mk[i] != 0.f) acc = __builtin_fma((double)gv[i], (double)X[i * Xs + tid], acc);      // a held-out row is never read: a NaN there stays there
      r[tid] = (float)acc;
    }
    __syncthreads();
    {      // A_j = W1[j] . r + b1[j] G: four threads per hidden unit, features f = quarter, quarter + 4, ..
      const int j = tid >> 2, qt = tid & 3;
      double acc = 0.;
      if (j < H) for (int f = qt; f < F; f += 4) acc = __builtin_fma((double)th[j * F + f], (double)r[f], acc);
      acc += __shfl_xor(acc, 1, 64);
      acc += __shfl_xor(acc, 2, 64);
      if (j < H && qt == 0) A[j] = (float)__builtin_fma((double)th[H * F + j], (double)G, acc);
    }
    __syncthreads();
    const BnnAdam ad = bnn_adam_at(lr, a.beta1, a.beta2, a.eps, t);
    for (int b = tid; b < nblk; b += CV_THREADS) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = 4 * b + e;
        if (i < D) {
          const float u = st[ld + i], sc = cv_softplus(u), ez = ep[i];
          const float gU = cv_grad(i, H, F, th[i], v, r, A, G);
          const float g_scale = gU * ez - 1.f / sc;
          const float g_u = g_scale * bnn_sigmoid(u, expf(-fabsf(u)));
          const BnnAdamOut nl = bnn_adam(st[i], st[2 * ld + i], st[3 * ld + i], gU, ad), nu = bnn_adam(u, st[4 * ld + i], st[5 * ld + i], g_u, ad);
          st[i] = nl.p, st[ld + i] = nu.p;
          st[2 * ld + i] = nl.m, st[3 * ld + i] = nl.v, st[4 * ld + i] = nu.m, st[5 * ld + i] = nu.v;
          bad = bad || !cv_finite(nl.p) || !cv_finite(nu.p);
        }
      }
    }
    if (tid == 0 && a.loss) a.loss[fit * a.num_steps + it] = (float)part;
  }

  // ---- the predictive: a thread reads the state it wrote ----
  if (a.S > 0) {
    const int rows = refit ? T : n;
    __syncthreads();      // the steps' last use of X and ep is over
    if (refit) {
      const float* xte = a.test + (long)p * T * F;
      for (int i = tid; i < T * F; i += CV_THREADS) {
        const int row = i / F, f = i - row * F;
        X[row * Xs + f] = xte[i];
      }
    }
    for (int b = tid; b < nblk; b += CV_THREADS)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = 4 * b + e;
        if (i < D) {
          const float sc = cv_softplus(st[ld + i]);
          ep[i] = sc;
          bad = bad || !cv_finite(st[i]) || !cv_finite(sc);
        }
      }
    const bool mine = tid < rows && (refit || held);
    const bool draws = (refit ? a.test_draw : a.cv_draw) != nullptr;
    const unsigned orow = refit ? (unsigned)(n + tid) : (unsigned)tid;      // the row's index among the observation uniforms
    double acc = 0.;
    int hits = 0;
    for (int k = 0; k < a.S; ++k) {
      for (int b = tid; b < nblk; b += CV_THREADS) {
        float z[4];
        normal4(philox4x32_10(((CV_PRED_DOMAIN + (unsigned long long)k) << 12) | (unsigned)b, q, a.seed), z);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * b + e;
          if (i < D) th[i] = __builtin_fmaf(ep[i], z[e], st[i]);
        }
      }
      __syncthreads();
      cv_collapse(th, H, F, v, w, cs);
      __syncthreads();
      if (mine) {
        const float d = cv_logit(X + tid * Xs, w, F, cs[0]);
        const float pr = bnn_sigmoid(d, expf(-fabsf(d)));
        acc += (double)pr;
        if (draws) {
          const U4 o = philox4x32_10(((CV_OBS_DOMAIN + (unsigned long long)k) << 12) | (orow >> 2), q, a.seed);
          const unsigned word = (orow & 3) == 0 ? o.x : (orow & 3) == 1 ? o.y : (orow & 3) == 2 ? o.z : o.w;
          hits += u01(word) < pr ? 1 : 0;
        }
      }
    }
    if (mine) {
      const long at = refit ? pc * T + tid : pc * n + tid;
      (refit ? a.test_prob : a.cv_prob)[at] = (float)(acc / (double)a.S);
      if (draws) (refit ? a.test_draw : a.cv_draw)[at] = (float)((double)hits / (double)a.S);
    }
  }
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (tid == 0) a.status[fit] = any_bad ? PFN_BNN_CV_NONFINITE : PFN_BNN_CV_DONE;
}

int launch_bnn_cv(const BnnCvArgs& a, int Hmax, hipStream_t s) {
  static LdsAllowance allowance;
  return launch_lds(bnn_cv_kernel, allowance, dim3(PFN_BNN_CV_SLOTS, (unsigned)a.NC, (unsigned)a.P), dim3(CV_THREADS), bnn_cv_lds_bytes(a.n, a.T, a.F, Hmax), s, a);
}

}  // namespace
}  // namespace pfn

using namespace pfn;

extern "C" int pfn_bnn_cv(const float* train, const float* labels, const float* test, const int32_t* fold, const int32_t* cand_H, const float* cand_lr, int P, int n, int T,
                          int F, int NC, int n_splits, float* state, int64_t ld, int64_t step0, int num_steps, float beta1, float beta2, float eps, int num_pred_samples,
                          uint64_t seed, const int64_t* problem_ids, float* loss, float* cv_prob, float* test_prob, float* cv_draw, float* test_draw, int32_t* status,
                          void* stream) {
  const char* why = "one block per fit, its rows, one theta and one eps in LDS";
  // the limits first: the ranges of n, T, F, NC, then (the candidates are host arrays) every width; then the arguments
  if (const int rc = fold_shapes("bnn_cv", why, 1, n, 128, T, F, NC, PFN_BNN_CV_MAX_CANDIDATES, 2, PFN_BNN_CV_FOLDS, true)) return rc;
  int Hmax = 0;
  if (cand_H)
    for (int c = 0; c < NC; ++c) {
      if (cand_H[c] < 1 || cand_H[c] > 64) return fail(PFN_ERR_UNSUPPORTED, "bnn_cv: cand_H[%d] = %d outside 1 .. 64", c, cand_H[c]);
      Hmax = cand_H[c] > Hmax ? cand_H[c] : Hmax;
    }
  if (const int rc = fold_shapes("bnn_cv", why, P, n, 128, T, F, NC, PFN_BNN_CV_MAX_CANDIDATES, n_splits, PFN_BNN_CV_FOLDS,
                                 train && labels && test && fold && cand_H && cand_lr && state && status)) return rc;
  if (ld < (int64_t)Hmax * (F + 3) + 2) return fail(PFN_ERR_ARGUMENT, "bnn_cv: ld %lld < D = H (F + 3) + 2 = %d of the widest candidate", (long long)ld, Hmax * (F + 3) + 2);
  if (step0 < 0 || step0 > (int64_t)1 << 40 || num_steps < 0 || num_pred_samples < 0 || num_pred_samples > 1 << 20)
    return fail(PFN_ERR_ARGUMENT, "bad bnn_cv arguments (0 <= step0 %lld <= 2^40, num_steps %d >= 0, 0 <= num_pred_samples %d <= 2^20)", (long long)step0, num_steps,
                num_pred_samples);
  for (int c = 0; c < NC; ++c)
    if (!(cand_lr[c] >= 0.f) || !(cand_lr[c] < __builtin_inff())) return fail(PFN_ERR_ARGUMENT, "bnn_cv: cand_lr[%d] = %g must be finite and >= 0", c, cand_lr[c]);
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f))
    return fail(PFN_ERR_ARGUMENT, "bad bnn_cv arguments (beta1 %g and beta2 %g in [0, 1), eps %g >= 0)", beta1, beta2, eps);
  if (num_pred_samples > 0 && (!cv_prob || !test_prob)) return fail(PFN_ERR_ARGUMENT, "bnn_cv: num_pred_samples %d > 0 needs cv_prob and test_prob", num_pred_samples);
  if (num_steps == 0 && num_pred_samples == 0) return PFN_OK;
  BnnCvArgs a{};
  a.train = train; a.labels = labels; a.test = test; a.fold = fold; a.P = P; a.n = n; a.T = T; a.F = F; a.NC = NC; a.n_splits = n_splits; a.state = state; a.ld = ld;
  a.step0 = step0; a.num_steps = num_steps; a.S = num_pred_samples; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.seed = seed; a.problem_ids = problem_ids;
  a.loss = loss; a.cv_prob = cv_prob; a.test_prob = test_prob; a.cv_draw = cv_draw; a.test_draw = test_draw; a.status = status;
  for (int c = 0; c < NC; ++c) { a.H[c] = cand_H[c]; a.lr[c] = cand_lr[c]; }
  PFN_TRY(launch_bnn_cv(a, Hmax, (hipStream_t)stream));
  return PFN_OK;
}
