// The tabular study's gradient-boosting baseline with its grid search (reference tabular.py:599-626, `xgb_metric`; DESIGN.md section 26, include/pfn_hip.h
// "Gradient-boosted trees with their grid search"): xgb_cv_kernel runs every boosting round of every (problem, candidate, fold slot) of a call in one launch,
// one block of 256 threads per fit, persistent over the rounds.  The algorithm is the exact greedy one on logistic loss, stated in include/pfn_hip.h; what
// matters for the code:
//   * the gradient statistics are rounded to fixed point (2^-23) once per round and every node or prefix sum is an int32 sum -- exact and free of any order,
//     so two candidates that cut the same partition through two features have bit-equal gains and the tie rule (lower feature, then lower position) decides;
//   * a feature's sort order depends on the problem alone: xgb_order_kernel writes the stable argsort of every (problem, feature) once, every fit reads it;
//   * per level a wave takes the sampled features f = wave, wave + 4, ..; lane j holds sorted positions j and j + 64.  The prefix sums of both open nodes come
//     from wave scans over cross-lane moves (all sampled rows, and the rows of the first open node; the second node is the difference), the next sampled row
//     of the same node -- the distinct-value test -- from a reverse "first valid" scan.  Then a wave argmax on (gain, -feature, -position) and the block's
//     over the four waves' slots in LDS.
// Where things live: the problem's train rows [n][F | 1], the orders [F][n] uint8, gi, hi and the row state (sampled bit, leaf code) in LDS; a thread keeps the
// margin of "its" row (train row tid, or test row tid - n in the refit slot) in a register.
// Draws (B(idx) = philox4x32_10(idx, stream, key = seed), stream = ((problem id * 64 + candidate id) * 8 + slot)):
//   row i in round t is sampled iff      word i & 3 of B((t << 6) | (i >> 2))             < floor(subsample 2^32)      (i: the row's index in the window)
//   feature f of round t's tree has word word f & 3 of B(2^32 | (t << 6) | (f >> 2));  the k features of smallest (word, f) are used.
// No atomics, no floating-point sum at all besides margin += leaf: a fit is a bitwise function of its own problem, candidate, slot, ids and seed.
#include "bnn_device.h"
#include "fold_device.h"

namespace pfn {

struct XgbCvArgs {
  const float* train;        // [P,n,F]
  const float* labels;       // [P,n]: class = label > 0.5
  const float* test;         // [P,T,F]
  const int32_t* fold;       // [P,n]: the CV test fold of each train row
  int P, n, T, F, NC, n_splits, rounds;
  unsigned long long seed;
  const int64_t* problem_ids;      // [P] or null
  uint8_t* order;            // [P,F,n]: written by xgb_order_kernel
  float* cv_margin;          // [P,NC,n]
  float* test_margin;        // [P,NC,T]
  int32_t* status;           // [P,NC,6]
  int32_t* tree_feature;     // [P,NC,6,rounds,3] or null
  float* tree_threshold;     // [P,NC,6,rounds,3] or null
  float* tree_leaf;          // [P,NC,6,rounds,4] or null
  int depth[PFN_XGB_CV_MAX_CANDIDATES];      // the candidates, by value: the entry point takes them as host arrays
  float eta[PFN_XGB_CV_MAX_CANDIDATES];
  int mcwi[PFN_XGB_CV_MAX_CANDIDATES];       // rint(min_child_weight 2^23), at most 2^30
  unsigned long long sub_thr[PFN_XGB_CV_MAX_CANDIDATES];      // floor(subsample 2^32)
  int k[PFN_XGB_CV_MAX_CANDIDATES];          // max(1, floor(colsample F))
  int cand_id[PFN_XGB_CV_MAX_CANDIDATES];
};
// 32 words of argmax slots, n rows at an odd stride of F | 1 floats, gi, hi and the row state over the rows, the feature words and flags, the orders:
// 85,120 bytes at n = F = 128; 25,888 at the study's n = 80, F = 60
inline size_t xgb_cv_lds_bytes(int n, int F) { return (32 + (size_t)n * (F | 1) + 3 * (size_t)n + 2 * (size_t)F) * 4 + (((size_t)F * n + 3) & ~(size_t)3); }
static_assert((32 + 128 * 129 + 3 * 128 + 2 * 128) * 4 + 128 * 128 <= 160 * 1024, "xgb_cv: LDS");

namespace {

constexpr int XGB_THREADS = 256;
constexpr unsigned long long XGB_FEATURE_DOMAIN = 1ull << 32;
constexpr float XGB_FIX = 8388608.f, XGB_UNFIX = 1.f / 8388608.f;      // 2^23
constexpr int XGB_SAMPLED = 4;      // row state: the sampled bit over the leaf code 0 .. 3
constexpr float XGB_MIN_GAIN = 1e-6f;

PFN_DEV unsigned xgb_word(const U4& b, int i) { return (i & 3) == 0 ? b.x : (i & 3) == 1 ? b.y : (i & 3) == 2 ? b.z : b.w; }
PFN_DEV bool xgb_finite(float x) { return fabsf(x) < __builtin_inff(); }

// inclusive prefix sum over the wave's 64 lanes
PFN_DEV int xgb_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}
// the first number that is no NaN at or after the lane (NaN: none)
PFN_DEV float xgb_next(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float u = __shfl_down(v, o, 64);
    if (lane + o < 64 && v != v) v = u;
  }
  return v;
}
PFN_DEV int xgb_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// G^2 / (H + lambda) of integer statistics, lambda = 1
PFN_DEV float xgb_score(int Gi, int Hi) {
  const float G = (float)Gi * XGB_UNFIX, H = (float)Hi * XGB_UNFIX;
  return G * G / (H + 1.f);
}

struct XgbBest {
  float gain;      // -inf: none
  int code;        // feature * 128 + position: the smaller wins among equal gains
  float thr;
};
PFN_DEV void xgb_take(XgbBest& b, float gain, int code, float thr) {
  if (gain > b.gain || (gain == b.gain && code < b.code)) b = XgbBest{gain, code, thr};
}
PFN_DEV XgbBest xgb_wave_best(XgbBest b) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) xgb_take(b, __shfl_xor(b.gain, o, 64), __shfl_xor(b.code, o, 64), __shfl_xor(b.thr, o, 64));
  return b;
}

// one sorted position of one feature: the candidate between this row and the next sampled row of its node
PFN_DEV void xgb_candidate(XgbBest& b, bool in, float xv, float nx, int GLi, int HLi, int Gt, int Ht, int mcwi, int code) {
  if (!in || nx != nx || nx == xv) return;      // not sampled, the node's last row, or an equal value
  const int GRi = Gt - GLi, HRi = Ht - HLi;
  if (HLi < mcwi || HRi < mcwi) return;
  const float gain = (xgb_score(GLi, HLi) + xgb_score(GRi, HRi)) - xgb_score(Gt, Ht);
  float thr = 0.5f * (xv + nx);
  if (thr == xv) thr = nx;
  xgb_take(b, gain, code, thr);
}

// the stable argsort of every (problem, feature) column over all n rows, key (value, row): grid (F, P), 128 threads
__global__ void __launch_bounds__(128) xgb_order_kernel(const float* train, uint8_t* order, int n, int F) {
  __shared__ float col[128];
  const int f = blockIdx.x, p = blockIdx.y, i = threadIdx.x;
  uint8_t* out = order + ((long)p * F + f) * n;
  float xi = 0.f;
  if (i < n) {
    xi = train[((long)p * n + i) * F + f];
    col[i] = xi;
    out[i] = (uint8_t)i;      // (a column with a NaN has no order: whatever the ranks leave unwritten is a row index all the same)
  }
  __syncthreads();
  if (i < n) {
    int rank = 0;
    for (int k = 0; k < n; ++k) {
      const float xk = col[k];
      rank += (xk < xi || (xk == xi && k < i)) ? 1 : 0;
    }
    out[rank] = (uint8_t)i;      // rank < n: at most n - 1 rows compare below
  }
}

__global__ void __launch_bounds__(XGB_THREADS) xgb_cv_kernel(XgbCvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xgb_lds[];
  const int n = a.n, T = a.T, F = a.F, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x, c = blockIdx.y, p = blockIdx.z;
  const long pc = (long)p * a.NC + c, fit = pc * PFN_XGB_CV_SLOTS + s;
  if (s > a.n_splits) {      // a slot this call does not use
    if (tid == 0) a.status[fit] = PFN_XGB_CV_UNUSED;
    return;
  }
  const int Xs = F | 1;
  float* best = xgb_lds;                                     // [4 waves][2 open nodes][gain, code, thr]
  float* X = xgb_lds + 32;                                   // [n][Xs]
  int* gi = reinterpret_cast<int*>(X + n * Xs);              // [n]
  int* hi = gi + n;                                          // [n]
  int* st = hi + n;                                          // [n] row state
  unsigned* fw = reinterpret_cast<unsigned*>(st + n);        // [F] the features' words of the round
  int* sel = reinterpret_cast<int*>(fw + F);                 // [F] 1: in the round's column sample
  uint8_t* ord = reinterpret_cast<uint8_t*>(sel + F);        // [F][n]
  const bool refit = s == a.n_splits;
  const int depth = a.depth[c], mcwi = a.mcwi[c], kcols = a.k[c];
  const float eta = a.eta[c];
  const unsigned long long sub_thr = a.sub_thr[c];
  const unsigned long long q =
      (((a.problem_ids ? (unsigned long long)a.problem_ids[p] : (unsigned long long)p) * 64ull + (unsigned long long)a.cand_id[c]) * 8ull) + (unsigned long long)s;

  // ---- stage ----
  bool bad = false;
  const float* xtr = a.train + (long)p * n * F;
  for (int i = tid; i < n * F; i += XGB_THREADS) {
    const int row = i / F, f = i - row * F;
    const float v = xtr[i];
    X[row * Xs + f] = v;
    bad = bad || !xgb_finite(v);
  }
  const uint8_t* og = a.order + (long)p * F * n;
  for (int i = tid; i < n * F; i += XGB_THREADS) ord[i] = (uint8_t)min((int)og[i], n - 1);
  // the thread's row: train row tid, or in the refit slot test row tid - n
  const bool is_train = tid < n, is_test = refit && tid >= n && tid < n + T;
  const float* xte = a.test + ((long)p * T + (is_test ? tid - n : 0)) * F;      // (read where is_test only)
  bool y1 = false, trains = false, held = false;
  if (is_train) {
    const int fo = a.fold[(long)p * n + tid];
    y1 = a.labels[(long)p * n + tid] > 0.5f;
    trains = refit || fo != s;
    held = !refit && fo == s;
  }
  if (is_test)
    for (int f = 0; f < F; ++f) bad = bad || !xgb_finite(xte[f]);
  float margin = 0.f;
  __syncthreads();

  for (int t = 0; t < a.rounds; ++t) {
    // ---- the round's statistics and draws ----
    if (is_train) {
      const float pr = bnn_sigmoid(margin, expf(-fabsf(margin)));
      const float g = pr - (y1 ? 1.f : 0.f), h = pr * (1.f - pr);
      const unsigned word = xgb_word(philox4x32_10(((unsigned long long)t << 6) | (unsigned)(tid >> 2), q, a.seed), tid);
      const bool in = trains && (unsigned long long)word < sub_thr;
      gi[tid] = (int)rintf(g * XGB_FIX);
      hi[tid] = (int)rintf(h * XGB_FIX);
      st[tid] = in ? XGB_SAMPLED : 0;
    }
    if (tid < F) fw[tid] = xgb_word(philox4x32_10(XGB_FEATURE_DOMAIN | ((unsigned long long)t << 6) | (unsigned)(tid >> 2), q, a.seed), tid);
    int leaf = 0;      // of the thread's row: 2 (right of the root) + 1 (right of the child)
    __syncthreads();
    if (tid < F) {
      const unsigned w = fw[tid];
      int rank = 0;
      for (int f = 0; f < F; ++f) {
        const unsigned o = fw[f];
        rank += (o < w || (o == w && f < tid)) ? 1 : 0;
      }
      sel[tid] = rank < kcols ? 1 : 0;
    }
    __syncthreads();

    int nf[3] = {-1, -1, -1};
    float nt[3] = {0.f, 0.f, 0.f};
    for (int d = 0; d < depth; ++d) {
      // the open nodes' totals, in every wave: node 0 is the root (d = 0) or its left child, node 1 the right child
      const int s0 = lane < n ? st[lane] : 0, s1 = lane + 64 < n ? st[lane + 64] : 0;
      int G0 = 0, H0 = 0, G1 = 0, H1 = 0;
      if (s0 & XGB_SAMPLED) { if (d == 0 || !(s0 & 2)) G0 += gi[lane], H0 += hi[lane]; else G1 += gi[lane], H1 += hi[lane]; }
      if (s1 & XGB_SAMPLED) { if (d == 0 || !(s1 & 2)) G0 += gi[lane + 64], H0 += hi[lane + 64]; else G1 += gi[lane + 64], H1 += hi[lane + 64]; }
      G0 = xgb_wave_sum(G0), H0 = xgb_wave_sum(H0);
      if (d > 0) G1 = xgb_wave_sum(G1), H1 = xgb_wave_sum(H1);
      XgbBest b0{-__builtin_inff(), 0x7fffffff, 0.f}, b1 = b0;
      for (int f = wave; f < F; f += 4) {
        if (!sel[f]) continue;
        const uint8_t* of = ord + f * n;
        // sorted positions lane (lo) and lane + 64 (hi)
        const int rl = lane < n ? of[lane] : 0, rh = lane + 64 < n ? of[lane + 64] : 0;
        const int sl = lane < n ? st[rl] : 0, sh = lane + 64 < n ? st[rh] : 0;
        const bool inl = (sl & XGB_SAMPLED) != 0, inh = (sh & XGB_SAMPLED) != 0;
        const bool n1l = d > 0 && (sl & 2), n1h = d > 0 && (sh & 2);      // in the second open node
        const float xl = X[rl * Xs + f], xh = X[rh * Xs + f];
        const int gl = inl ? gi[rl] : 0, hl = inl ? hi[rl] : 0, gh = inh ? gi[rh] : 0, hh = inh ? hi[rh] : 0;
        const float nan = __builtin_nanf("");
        // prefix sums over all sampled rows, and (below the root) over the first open node's
        int GAl = xgb_scan(gl, lane), HAl = xgb_scan(hl, lane), GAh = 0, HAh = 0;
        int G0l = GAl, H0l = HAl, G0h = 0, H0h = 0;
        float x0l = xgb_next(inl && !n1l ? xl : nan, lane), x1l = nan, x0h = nan, x1h = nan;
        if (d > 0) {
          G0l = xgb_scan(n1l ? 0 : gl, lane), H0l = xgb_scan(n1l ? 0 : hl, lane);
          x1l = xgb_next(inl && n1l ? xl : nan, lane);
        }
        if (n > 64) {
          GAh = xgb_scan(gh, lane) + __shfl(GAl, 63, 64), HAh = xgb_scan(hh, lane) + __shfl(HAl, 63, 64);
          G0h = GAh, H0h = HAh;
          x0h = xgb_next(inh && !n1h ? xh : nan, lane);
          if (d > 0) {
            G0h = xgb_scan(n1h ? 0 : gh, lane) + __shfl(G0l, 63, 64), H0h = xgb_scan(n1h ? 0 : hh, lane) + __shfl(H0l, 63, 64);
            x1h = xgb_next(inh && n1h ? xh : nan, lane);
          }
        }
        // the next sampled row of the same node: after this lane in its half, else the first of the upper half
        const float f0h = __shfl(x0h, 0, 64), f1h = __shfl(x1h, 0, 64);
        float u;
        u = __shfl_down(x0l, 1, 64); float nx0l = lane < 63 ? u : nan; if (nx0l != nx0l) nx0l = f0h;
        u = __shfl_down(x1l, 1, 64); float nx1l = lane < 63 ? u : nan; if (nx1l != nx1l) nx1l = f1h;
        u = __shfl_down(x0h, 1, 64); const float nx0h = lane < 63 ? u : nan;
        u = __shfl_down(x1h, 1, 64); const float nx1h = lane < 63 ? u : nan;
        if (n1l) xgb_candidate(b1, inl, xl, nx1l, GAl - G0l, HAl - H0l, G1, H1, mcwi, f * 128 + lane);
        else xgb_candidate(b0, inl, xl, nx0l, G0l, H0l, G0, H0, mcwi, f * 128 + lane);
        if (n1h) xgb_candidate(b1, inh, xh, nx1h, GAh - G0h, HAh - H0h, G1, H1, mcwi, f * 128 + lane + 64);
        else xgb_candidate(b0, inh, xh, nx0h, G0h, H0h, G0, H0, mcwi, f * 128 + lane + 64);
      }
      b0 = xgb_wave_best(b0);
      if (d > 0) b1 = xgb_wave_best(b1);
      if (lane == 0) {
        best[(wave * 2) * 3] = b0.gain, best[(wave * 2) * 3 + 1] = __int_as_float(b0.code), best[(wave * 2) * 3 + 2] = b0.thr;
        best[(wave * 2 + 1) * 3] = b1.gain, best[(wave * 2 + 1) * 3 + 1] = __int_as_float(b1.code), best[(wave * 2 + 1) * 3 + 2] = b1.thr;
      }
      __syncthreads();
      // the block's best of each open node, the same bits in every thread
      XgbBest w0{-__builtin_inff(), 0x7fffffff, 0.f}, w1 = w0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xgb_take(w0, best[(k * 2) * 3], __float_as_int(best[(k * 2) * 3 + 1]), best[(k * 2) * 3 + 2]);
        xgb_take(w1, best[(k * 2 + 1) * 3], __float_as_int(best[(k * 2 + 1) * 3 + 1]), best[(k * 2 + 1) * 3 + 2]);
      }
      const bool split0 = w0.gain > XGB_MIN_GAIN, split1 = d > 0 && w1.gain > XGB_MIN_GAIN;
      const int f0 = w0.code >> 7, f1 = w1.code >> 7;
      if (d == 0) {
        if (split0) nf[0] = f0, nt[0] = w0.thr;
      } else {
        if (split0) nf[1] = f0, nt[1] = w0.thr;
        if (split1) nf[2] = f1, nt[2] = w1.thr;
      }
      // route the thread's row
      if (is_train || is_test) {
        const bool second = d > 0 && (leaf & 2);
        const bool splits = second ? split1 : split0;
        if (splits) {
          const int f = second ? f1 : f0;
          const float xv = is_train ? X[tid * Xs + f] : xte[f];
          const bool right = !(xv < (second ? w1.thr : w0.thr));
          if (right) leaf |= d == 0 ? 2 : 1;
        }
        if (is_train) st[tid] = (st[tid] & XGB_SAMPLED) | leaf;
      }
      __syncthreads();
      if (d == 0 && !split0) break;      // (the same decision in every thread)
    }

    // ---- the leaves: -eta G / (H + lambda) over each leaf's sampled rows ----
    float val[4];
    {
      const int s0 = lane < n ? st[lane] : 0, s1 = lane + 64 < n ? st[lane + 64] : 0;
#pragma unroll
      for (int L = 0; L < 4; ++L) {
        int G = 0, H = 0;
        if (s0 == (XGB_SAMPLED | L)) G += gi[lane], H += hi[lane];
        if (s1 == (XGB_SAMPLED | L)) G += gi[lane + 64], H += hi[lane + 64];
        G = xgb_wave_sum(G), H = xgb_wave_sum(H);
        const float Gf = (float)G * XGB_UNFIX, Hf = (float)H * XGB_UNFIX;
        val[L] = eta * -(Gf / (Hf + 1.f));
      }
    }
    margin += leaf == 0 ? val[0] : leaf == 1 ? val[1] : leaf == 2 ? val[2] : val[3];
    if (tid == 0 && a.tree_feature) {
      const long at = fit * a.rounds + t;
#pragma unroll
      for (int k = 0; k < 3; ++k) a.tree_feature[at * 3 + k] = nf[k], a.tree_threshold[at * 3 + k] = nt[k];
#pragma unroll
      for (int L = 0; L < 4; ++L) a.tree_leaf[at * 4 + L] = val[L];
    }
    __syncthreads();      // the round's last reads of the row state are over
  }

  if (held) a.cv_margin[pc * n + tid] = margin;
  if (is_test) a.test_margin[pc * T + (tid - n)] = margin;
  bad = bad || !xgb_finite(margin);
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (tid == 0) a.status[fit] = any_bad ? PFN_XGB_CV_NONFINITE : PFN_XGB_CV_DONE;
}

int launch_xgb_cv(const XgbCvArgs& a, hipStream_t s) {
  static LdsAllowance allowance;
  xgb_order_kernel<<<dim3((unsigned)a.F, (unsigned)a.P), dim3(128), 0, s>>>(a.train, a.order, a.n, a.F);
  if (hipGetLastError() != hipSuccess) return PFN_ERR_LAUNCH;
  return launch_lds(xgb_cv_kernel, allowance, dim3(PFN_XGB_CV_SLOTS, (unsigned)a.NC, (unsigned)a.P), dim3(XGB_THREADS), xgb_cv_lds_bytes(a.n, a.F), s, a);
}

}  // namespace
}  // namespace pfn

using namespace pfn;

extern "C" int pfn_xgb_cv(const float* train, const float* labels, const float* test, const int32_t* fold, const int32_t* cand_depth, const float* cand_lr,
                          const double* cand_mcw, const double* cand_subsample, const double* cand_colsample, const int32_t* cand_ids, int P, int n, int T, int F,
                          int NC, int n_splits, int num_rounds, uint64_t seed, const int64_t* problem_ids, uint8_t* order, float* cv_margin, float* test_margin,
                          int32_t* status, int32_t* tree_feature, float* tree_threshold, float* tree_leaf, void* stream) {
  const char* why = "one block per fit, its rows and their sort orders in LDS";
  // the limits first: the ranges of n, T, F, NC, then (the candidates are host arrays) every candidate's; then the arguments
  if (const int rc = fold_shapes("xgb_cv", why, 1, n, 128, T, F, NC, PFN_XGB_CV_MAX_CANDIDATES, 2, PFN_XGB_CV_FOLDS, true)) return rc;
  if (num_rounds < 0 || num_rounds > PFN_XGB_CV_MAX_ROUNDS) return fail(PFN_ERR_UNSUPPORTED, "xgb_cv: num_rounds %d outside 0 .. %d", num_rounds, PFN_XGB_CV_MAX_ROUNDS);
  if (cand_depth && cand_lr && cand_mcw && cand_subsample && cand_colsample)
    for (int c = 0; c < NC; ++c) {
      if (cand_depth[c] < 1 || cand_depth[c] > PFN_XGB_CV_MAX_DEPTH)
        return fail(PFN_ERR_UNSUPPORTED, "xgb_cv: cand_depth[%d] = %d outside 1 .. %d", c, cand_depth[c], PFN_XGB_CV_MAX_DEPTH);
      if (cand_subsample[c] <= 0. || cand_subsample[c] > 1. || cand_colsample[c] <= 0. || cand_colsample[c] > 1. || cand_mcw[c] < 0. || cand_lr[c] <= 0.f)
        return fail(PFN_ERR_UNSUPPORTED, "xgb_cv: candidate %d: subsample %g and colsample %g must lie in (0, 1], min_child_weight %g >= 0, learning_rate %g > 0", c,
                    cand_subsample[c], cand_colsample[c], cand_mcw[c], cand_lr[c]);
    }
  if (const int rc = fold_shapes("xgb_cv", why, P, n, 128, T, F, NC, PFN_XGB_CV_MAX_CANDIDATES, n_splits, PFN_XGB_CV_FOLDS,
                                 train && labels && test && fold && cand_depth && cand_lr && cand_mcw && cand_subsample && cand_colsample && order && cv_margin &&
                                     test_margin && status)) return rc;
  if ((tree_feature || tree_threshold || tree_leaf) && !(tree_feature && tree_threshold && tree_leaf))
    return fail(PFN_ERR_ARGUMENT, "xgb_cv: tree_feature, tree_threshold and tree_leaf come together or not at all");
  XgbCvArgs a{};
  for (int c = 0; c < NC; ++c) {
    if (!(cand_lr[c] > 0.f) || !(cand_lr[c] < __builtin_inff()) || !(cand_subsample[c] > 0.) || !(cand_colsample[c] > 0.) || !(cand_mcw[c] >= 0.) ||
        !(cand_mcw[c] < __builtin_inf()))
      return fail(PFN_ERR_ARGUMENT, "xgb_cv: candidate %d holds a number that is not finite", c);
    if (cand_ids && (cand_ids[c] < 0 || cand_ids[c] >= PFN_XGB_CV_MAX_CANDIDATES))
      return fail(PFN_ERR_ARGUMENT, "xgb_cv: cand_ids[%d] = %d outside 0 .. %d", c, cand_ids[c], PFN_XGB_CV_MAX_CANDIDATES - 1);
    a.depth[c] = cand_depth[c];
    a.eta[c] = cand_lr[c];
    const double m = __builtin_rint(cand_mcw[c] * 8388608.);      // (a sum of hi is at most 128 2^21 = 2^28: beyond 2^30 nothing changes)
    a.mcwi[c] = m > 1073741824. ? 1073741824 : (int)m;
    a.sub_thr[c] = (unsigned long long)__builtin_floor(cand_subsample[c] * 4294967296.);
    const int k = (int)__builtin_floor(cand_colsample[c] * (double)F);
    a.k[c] = k < 1 ? 1 : k;
    a.cand_id[c] = cand_ids ? cand_ids[c] : c;
  }
  a.train = train; a.labels = labels; a.test = test; a.fold = fold; a.P = P; a.n = n; a.T = T; a.F = F; a.NC = NC; a.n_splits = n_splits; a.rounds = num_rounds;
  a.seed = seed; a.problem_ids = problem_ids; a.order = order; a.cv_margin = cv_margin; a.test_margin = test_margin; a.status = status;
  a.tree_feature = tree_feature; a.tree_threshold = tree_threshold; a.tree_leaf = tree_leaf;
  PFN_TRY(launch_xgb_cv(a, (hipStream_t)stream));
  return PFN_OK;
}
