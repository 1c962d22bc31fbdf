// The tabular study's CatBoost baseline with its grid search (reference tabular.py:556-596, `catboost_metric`; DESIGN.md section 27, include/pfn_hip.h
// "Oblivious boosted trees with their grid search"): catboost_cv_kernel grows every tree of every (problem, candidate, slot) of a call in one launch, one block
// of 256 threads per fit, persistent over the trees and their levels.  The algorithm is stated in include/pfn_hip.h; what matters for the code:
//   * a tree is symmetric: one (feature, border) splits every leaf of a level, so a candidate's score needs the sums of BOTH children of EVERY leaf.  Only
//     the leaves that hold learn rows count (at most n of the 2^d): they live in a compact list in ascending code, a learn row carries its index in the list;
//   * per level a wave takes the features f = wave, wave + 4, ..; lane j holds sorted positions j and j + 64.  For every leaf of the list the prefix sum of gi
//     over the positions is a wave scan (cross-lane moves), the prefix count a ballot and a population count; the four running float sums of the header are
//     carried per lane through the list, in its order.  The next learn row with another value -- the border test -- comes from the ballot of the learn rows;
//   * the gradient statistics are 2^-23 fixed point (tree structure) and 2^-40 fixed point in int64 (Newton sums, the summed loss): integer sums have no order;
//     the float sums run over the leaf list in its order, the same in every thread.  No atomics: a fit is a bitwise function of its own inputs;
//   * this file is compiled with -ffp-contract=off (csrc/build.sh): the header rounds every operation once.
// Where things live: the window's rows [n][F | 1], the orders [F][n] uint8, gi, the rows' list index and bit, the Newton terms and the leaf list in LDS; a
// thread keeps the margin and the leaf code of "its" row (train row tid, or test row tid - n in the refit slot) in registers.
#include "fold_device.h"
#include "pfn_device.h"

namespace pfn {

struct CatCvArgs {
  const float* train;        // [P,n,F]
  const float* labels;       // [P,n]: class = label > 0.5
  const float* test;         // [P,T,F]
  const int32_t* fold;       // [P,n]: 0 = held out of the search fit
  int P, n, T, F, NC, NK, rounds;
  unsigned long long seed;
  const int64_t* problem_ids;      // [P] or null
  uint8_t* order;            // [P,F,n]: written by cat_order_kernel
  float* hold_margin;        // [P,NC,NK,n]
  float* test_margin;        // [P,NC,NK,T]
  int32_t* status;           // [P,NC,2]
  int32_t* tree_feature;     // [P,NC,2,rounds,7] or null
  float* tree_threshold;     // [P,NC,2,rounds,7] or null
  float* tree_leaf;          // [P,NC,2,rounds,128] or null
  int depth[PFN_CATBOOST_CV_MAX_CANDIDATES];      // the candidates, by value: the entry point takes them as host arrays
  float lr[PFN_CATBOOST_CV_MAX_CANDIDATES];
  float l2[PFN_CATBOOST_CV_MAX_CANDIDATES];
  int cand_id[PFN_CATBOOST_CV_MAX_CANDIDATES];
  int checkpoint[PFN_CATBOOST_CV_MAX_CHECKPOINTS];
};
// 32 words of reduction slots, the Newton terms (2 int64 per row), the rows at an odd stride of F | 1 floats, gi, list index and bit per row, 10 arrays over
// the 128 leaves, the orders: 91,264 bytes at n = F = 128; 31,808 at the study's n = 80, F = 60
inline size_t catboost_cv_lds_bytes(int n, int F) { return (32 + 4 * (size_t)n + (size_t)n * (F | 1) + 3 * (size_t)n + 10 * 128) * 4 + (((size_t)F * n + 3) & ~(size_t)3); }
static_assert((32 + 4 * 128 + 128 * 129 + 3 * 128 + 10 * 128) * 4 + 128 * 128 <= 160 * 1024, "catboost_cv: LDS");

namespace {

constexpr int CAT_THREADS = 256;
constexpr int CAT_LEAVES = PFN_CATBOOST_CV_MAX_LEAVES, CAT_DEPTH = PFN_CATBOOST_CV_MAX_DEPTH;
constexpr float CAT_FIX = 8388608.f, CAT_UNFIX = 1.f / 8388608.f;                    // 2^23
constexpr float CAT_FIX40 = 1099511627776.f, CAT_UNFIX40 = 1.f / 1099511627776.f;    // 2^40
constexpr float CAT_UNFIX46 = 1.f / 70368744177664.f;                                // 2^-46
constexpr int CAT_NEWTON = 10, CAT_HALVINGS = 10;

PFN_DEV bool cat_finite(float x) { return fabsf(x) < __builtin_inff(); }
PFN_DEV float cat_sig(float z) {
  const float e = expf(-fabsf(z));
  return (z >= 0.f ? 1.f : e) / (1.f + e);
}
PFN_DEV long long cat_fix40(float v) { return (long long)rintf(v * CAT_FIX40); }

// inclusive prefix sum over the wave's 64 lanes
PFN_DEV int cat_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}
// the sum of v over the block's four waves, the same bits in every thread; red: 4 int64 of LDS.  Every thread calls.
PFN_DEV long long cat_block_sum(long long v, long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();      // the previous use of red is over
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

struct CatBest {
  float value;     // -inf: none
  int code;        // feature * 128 + position: the smaller wins among equal values
  float thr;
};
PFN_DEV void cat_take(CatBest& b, float value, int code, float thr) {
  if (value > b.value || (value == b.value && code < b.code)) b = CatBest{value, code, thr};
}
PFN_DEV CatBest cat_wave_best(CatBest b) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cat_take(b, __shfl_xor(b.value, o, 64), __shfl_xor(b.code, o, 64), __shfl_xor(b.thr, o, 64));
  return b;
}

// the four running sums of one candidate, and one leaf's two children added to them
struct CatSums {
  float num_lo = 0.f, den_lo = 0.f, num_hi = 0.f, den_hi = 0.f;
};
PFN_DEV void cat_child(float& num, float& den, int Gi, int c, float l2) {
  if (c <= 0) return;
  const float G = (float)Gi * CAT_UNFIX, cf = (float)c;
  const float avg = G / (cf + l2);
  num += avg * G;
  den += (avg * avg) * cf;
}
PFN_DEV void cat_leaf(CatSums& s, int GLi, int cL, int Gt, int ct, float l2) {
  cat_child(s.num_lo, s.den_lo, GLi, cL, l2);
  cat_child(s.num_hi, s.den_hi, Gt - GLi, ct - cL, l2);
}
PFN_DEV float cat_score(const CatSums& s) {
  const float num = s.num_lo + s.num_hi, den = s.den_lo + s.den_hi;
  return den > 0.f ? num / sqrtf(den) : 0.f;
}
// the standard normal of candidate (t, d, f, j)
PFN_DEV float cat_normal(int t, int d, int f, int j, unsigned long long q, unsigned long long seed) {
  const U4 b = philox4x32_10(((unsigned long long)t << 17) | ((unsigned long long)d << 14) | ((unsigned long long)f << 7) | (unsigned long long)j, q, seed);
  const float u1 = ((float)(b.x >> 9) + 0.5f) * 1.1920928955078125e-7f, u2 = (float)(b.y >> 8) * 5.9604644775390625e-8f;      // 2^-23, 2^-24: both exact
  return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// the stable argsort of every (problem, feature) column over all n rows, key (value, row): grid (F, P), 128 threads (as xgb_cv.hip's, which stays its own)
__global__ void __launch_bounds__(128) cat_order_kernel(const float* train, uint8_t* order, int n, int F) {
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

__global__ void __launch_bounds__(CAT_THREADS) catboost_cv_kernel(CatCvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float cat_lds[];
  const int n = a.n, T = a.T, F = a.F, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x, c = blockIdx.y, p = blockIdx.z;
  const long pc = (long)p * a.NC + c, fit = pc * PFN_CATBOOST_CV_SLOTS + s;
  const int Xs = F | 1;
  float* best = cat_lds;                                               // [4 waves][value, code, thr]          words 0 .. 11
  int* shared = reinterpret_cast<int*>(cat_lds + 12);                  // [0]: the list's length after a split  words 12 .. 15
  long long* red = reinterpret_cast<long long*>(cat_lds + 16);         // [4]                                   words 16 .. 23
  long long* ri = reinterpret_cast<long long*>(cat_lds + 32);          // [n] Newton terms
  long long* hi = ri + n;                                              // [n]
  float* X = reinterpret_cast<float*>(hi + n);                         // [n][Xs]
  int* gi = reinterpret_cast<int*>(X + n * Xs);                        // [n]
  int* li = gi + n;                                                    // [n] a learn row's index in the leaf list, -1 for a row that does not learn
  int* rb = li + n;                                                    // [n] the row's bit of the level
  int* lcode = rb + n;                                                 // the leaf list, [128] each: code,
  int* lG = lcode + CAT_LEAVES;                                        //   sum of gi,
  int* lc = lG + CAT_LEAVES;                                           //   count,
  float* lv = reinterpret_cast<float*>(lc + CAT_LEAVES);               //   value,
  float* lstep = lv + CAT_LEAVES;                                      //   Newton step;
  int* tcL = reinterpret_cast<int*>(lstep + CAT_LEAVES);               // the children of a split: counts,
  int* tcR = tcL + CAT_LEAVES;
  int* mapL = tcR + CAT_LEAVES;                                        //   their places in the new list (-1: empty);
  int* mapR = mapL + CAT_LEAVES;
  int* slot_of = mapR + CAT_LEAVES;                                    // leaf code -> place in the list, -1
  uint8_t* ord = reinterpret_cast<uint8_t*>(slot_of + CAT_LEAVES);     // [F][n]
  const bool refit = s == 1;
  const int depth = a.depth[c];
  const float lr = a.lr[c], l2 = a.l2[c];
  const unsigned long long q =
      (((a.problem_ids ? (unsigned long long)a.problem_ids[p] : (unsigned long long)p) * 64ull + (unsigned long long)a.cand_id[c]) * 8ull) + (unsigned long long)s;

  // ---- stage ----
  bool bad = false;
  const float* xtr = a.train + (long)p * n * F;
  for (int i = tid; i < n * F; i += CAT_THREADS) {
    const int row = i / F, f = i - row * F;
    const float v = xtr[i];
    X[row * Xs + f] = v;
    bad = bad || !cat_finite(v);
  }
  const uint8_t* og = a.order + (long)p * F * n;
  for (int i = tid; i < n * F; i += CAT_THREADS) ord[i] = (uint8_t)min((int)og[i], n - 1);
  // the thread's row: train row tid, or in the refit slot test row tid - n
  const bool is_train = tid < n, is_test = refit && tid >= n && tid < n + T;
  const float* xte = a.test + ((long)p * T + (is_test ? tid - n : 0)) * F;      // (read where is_test only)
  bool y1 = false, learns = false, held = false;
  if (is_train) {
    const int fo = a.fold[(long)p * n + tid];
    y1 = a.labels[(long)p * n + tid] > 0.5f;
    learns = refit || fo != 0;
    held = !refit && fo == 0;
  }
  if (is_test)
    for (int f = 0; f < F; ++f) bad = bad || !cat_finite(xte[f]);
  const int m = (int)cat_block_sum(learns ? 1 : 0, red), m1 = (int)cat_block_sum(learns && y1 ? 1 : 0, red);      // (both syncs: the staging is over)
  if (__syncthreads_or(bad ? 1 : 0)) {
    if (tid == 0) a.status[fit] = PFN_CATBOOST_CV_NONFINITE;
    return;
  }
  if (m1 == 0 || m1 == m) {
    if (tid == 0) a.status[fit] = PFN_CATBOOST_CV_ONE_CLASS;
    return;
  }
  const float mf = (float)m, logm = logf(mf);
  float margin = 0.f;
  int next_checkpoint = 0;

  for (int t = 0; t < a.rounds; ++t) {
    // ---- the tree's statistics ----
    int g = 0;
    if (is_train) {
      if (learns) g = (int)rintf(((y1 ? 1.f : 0.f) - cat_sig(margin)) * CAT_FIX);
      gi[tid] = g;
      li[tid] = learns ? 0 : -1;
    }
    const long long Gall = cat_block_sum((long long)g, red), S2 = cat_block_sum((long long)g * (long long)g, red);
    if (tid == 0) lcode[0] = 0, lG[0] = (int)Gall, lc[0] = m;
    const float L = expf(logm - (float)t * lr);
    const float sigma = sqrtf(((float)S2 * CAT_UNFIX46) / mf) * (L / (1.f + L));
    int NL = 1, code = 0;      // the list's length; the leaf code of the thread's row
    int nf[CAT_DEPTH], used[CAT_DEPTH];
    float nt[CAT_DEPTH];
#pragma unroll
    for (int d = 0; d < CAT_DEPTH; ++d) nf[d] = -1, nt[d] = 0.f, used[d] = -1;
    __syncthreads();

    for (int d = 0; d < depth; ++d) {
      CatBest b{-__builtin_inff(), 0x7fffffff, 0.f};
      for (int f = wave; f < F; f += 4) {
        const uint8_t* of = ord + f * n;
        // sorted positions lane (l) and lane + 64 (h)
        const bool vl = lane < n, vh = lane + 64 < n;
        const int rl = vl ? of[lane] : 0, rh = vh ? of[lane + 64] : 0;
        const int kl = vl ? li[rl] : -1, kh = vh ? li[rh] : -1;
        const float xl = X[rl * Xs + f], xh = X[rh * Xs + f];
        const int gl = kl >= 0 ? gi[rl] : 0, gh = kh >= 0 ? gi[rh] : 0;
        // the next learn row: after this lane in its half, else the first of the upper half -- from the two ballots of "learns", by explicit lanes
        const unsigned long long lm = __ballot(kl >= 0), hm = n > 64 ? __ballot(kh >= 0) : 0ull;
        const unsigned long long al = lane < 63 ? lm >> (lane + 1) : 0ull, ah = lane < 63 ? hm >> (lane + 1) : 0ull;      // the learn rows after this lane
        const float nl_lo = __shfl(xl, al ? lane + __ffsll(al) : 0, 64), nl_hi = __shfl(xh, hm ? __ffsll(hm) - 1 : 0, 64);
        const float nxl = al ? nl_lo : nl_hi, nxh = __shfl(xh, ah ? lane + __ffsll(ah) : 0, 64);
        bool bl = kl >= 0 && (al || hm) && nxl != xl, bh = kh >= 0 && ah && nxh != xh;      // a border follows the position
#pragma unroll
        for (int k = 0; k < CAT_DEPTH; ++k) {
          bl = bl && used[k] != f * 128 + lane;
          bh = bh && used[k] != f * 128 + lane + 64;
        }
        if (!__any(bl || bh)) continue;      // (the wave's decision: a constant column, or every border used)
        CatSums sl, sh;
        for (int k = 0; k < NL; ++k) {
          const int Gt = lG[k], ct = lc[k];
          const bool inl = kl == k, inh = kh == k;
          const unsigned long long ml = __ballot(inl);
          const int Gl = cat_scan(inl ? gl : 0, lane), cl = __popcll(ml & ((2ull << lane) - 1ull));
          cat_leaf(sl, Gl, cl, Gt, ct, l2);
          if (n > 64) {
            const unsigned long long mh = __ballot(inh);
            const int Gh = cat_scan(inh ? gh : 0, lane) + __shfl(Gl, 63, 64), ch = __popcll(mh & ((2ull << lane) - 1ull)) + __popcll(ml);
            cat_leaf(sh, Gh, ch, Gt, ct, l2);
          }
        }
        if (bl) {
          float thr = 0.5f * (xl + nxl);
          if (thr == nxl) thr = xl;
          cat_take(b, cat_score(sl) + sigma * cat_normal(t, d, f, lane, q, a.seed), f * 128 + lane, thr);
        }
        if (bh) {
          float thr = 0.5f * (xh + nxh);
          if (thr == nxh) thr = xh;
          cat_take(b, cat_score(sh) + sigma * cat_normal(t, d, f, lane + 64, q, a.seed), f * 128 + lane + 64, thr);
        }
      }
      b = cat_wave_best(b);
      if (lane == 0) best[wave * 3] = b.value, best[wave * 3 + 1] = __int_as_float(b.code), best[wave * 3 + 2] = b.thr;
      __syncthreads();
      // the block's best, the same bits in every thread
      CatBest w{-__builtin_inff(), 0x7fffffff, 0.f};
#pragma unroll
      for (int k = 0; k < 4; ++k) cat_take(w, best[k * 3], __float_as_int(best[k * 3 + 1]), best[k * 3 + 2]);
      if (w.code == 0x7fffffff) break;      // no candidate is left: the tree ends (the same decision in every thread; the slots are rewritten after a sync)
      const int fs = w.code >> 7;
#pragma unroll
      for (int k = 0; k < CAT_DEPTH; ++k)
        if (k == d) nf[k] = fs, nt[k] = w.thr, used[k] = w.code;
      // the rows' bits
      if (is_train || is_test) {
        const float xv = is_train ? X[tid * Xs + fs] : xte[fs];
        const int bit = xv > w.thr ? 1 : 0;
        code |= bit << d;
        if (is_train) rb[tid] = bit;
      }
      __syncthreads();
      // the children of every leaf of the list, then their places in the new list: the low children in the list's order, then the high ones
      int myc = 0, GL = 0, GR = 0, cL = 0, cR = 0;
      if (tid < NL) {
        myc = lcode[tid];
        for (int i = 0; i < n; ++i) {
          const bool mine = li[i] == tid;
          const int gv = gi[i], bit = rb[i];
          if (mine && bit) GR += gv, ++cR;
          if (mine && !bit) GL += gv, ++cL;
        }
        tcL[tid] = cL, tcR[tid] = cR;
      }
      __syncthreads();
      if (tid < NL) {
        int rankL = 0, rankR = 0, totL = 0, totR = 0;
        for (int k = 0; k < NL; ++k) {
          const int hasL = tcL[k] > 0 ? 1 : 0, hasR = tcR[k] > 0 ? 1 : 0;
          totL += hasL, totR += hasR;
          if (k < tid) rankL += hasL, rankR += hasR;
        }
        const int pl = cL > 0 ? rankL : -1, pr = cR > 0 ? totL + rankR : -1;
        mapL[tid] = pl, mapR[tid] = pr;
        // every thread took its own entry of the list before the sync above; nobody reads the list here, and the places are distinct
        if (pl >= 0) lcode[pl] = myc, lG[pl] = GL, lc[pl] = cL;
        if (pr >= 0) lcode[pr] = myc | (1 << d), lG[pr] = GR, lc[pr] = cR;
        if (tid == 0) shared[0] = totL + totR;
      }
      __syncthreads();
      if (is_train && learns) li[tid] = rb[tid] ? mapR[li[tid]] : mapL[li[tid]];
      NL = shared[0];
      __syncthreads();
    }
    __syncthreads();      // (after a break: the argmax slots are read)

    // ---- the leaf values: Newton with backtracking over the list ----
    if (tid < CAT_LEAVES) lv[tid] = 0.f, lstep[tid] = 0.f, slot_of[tid] = -1;
    __syncthreads();
    if (tid < NL) slot_of[lcode[tid]] = tid;
    const int my = is_train && learns ? li[tid] : 0;
    const float pen_half = 0.5f * l2;
    float obj;
    {
      long long lossi = 0;
      if (is_train && learns) lossi = cat_fix40(fmaxf(y1 ? -margin : margin, 0.f) + log1pf(expf(-fabsf(margin))));
      obj = (float)cat_block_sum(lossi, red) * CAT_UNFIX40 + pen_half * 0.f;
    }
    for (int it = 0; it < CAT_NEWTON; ++it) {
      if (is_train && learns) {
        const float z = margin + lv[my];
        const float sp = cat_sig(z), sm = cat_sig(-z);
        ri[tid] = cat_fix40(y1 ? sm : -sp);
        hi[tid] = cat_fix40(sp * sm);
      }
      __syncthreads();
      if (tid < NL) {
        long long R = 0, H = 0;
        for (int i = 0; i < n; ++i)
          if (li[i] == tid) R += ri[i], H += hi[i];
        const float den = (float)H * CAT_UNFIX40 + l2;
        lstep[tid] = den > 0.f ? ((float)R * CAT_UNFIX40) / den : 0.f;
      }
      __syncthreads();
      float scale = 1.f;
      bool taken = false;
      for (int hv = 0; hv <= CAT_HALVINGS; ++hv, scale *= 0.5f) {
        long long lossi = 0;
        if (is_train && learns) {
          const float z = margin + (lv[my] + scale * lstep[my]);
          lossi = cat_fix40(fmaxf(y1 ? -z : z, 0.f) + log1pf(expf(-fabsf(z))));
        }
        float pen = 0.f;
        for (int k = 0; k < NL; ++k) {
          const float vt = lv[k] + scale * lstep[k];
          pen += vt * vt;
        }
        const float tried = (float)cat_block_sum(lossi, red) * CAT_UNFIX40 + pen_half * pen;
        if (tried <= obj) {      // (the same bits, the same decision in every thread)
          obj = tried;
          taken = true;
          break;
        }
      }
      if (!taken) break;
      __syncthreads();      // every thread has read lv and lstep
      if (tid < NL) lv[tid] = lv[tid] + scale * lstep[tid];
      __syncthreads();
    }
    __syncthreads();

    // ---- the rows take their leaf's value ----
    if (is_train || is_test) {
      const int k = slot_of[code];
      if (k >= 0) margin += lr * lv[k];
    }
    if (a.tree_feature) {
      const long at = fit * a.rounds + t;
      if (tid < CAT_DEPTH) {
        int fv = -1;
        float tv = 0.f;
#pragma unroll
        for (int k = 0; k < CAT_DEPTH; ++k)
          if (k == tid) fv = nf[k], tv = nt[k];
        a.tree_feature[at * CAT_DEPTH + tid] = fv, a.tree_threshold[at * CAT_DEPTH + tid] = tv;
      }
      if (tid < CAT_LEAVES) {
        const int k = slot_of[tid];
        a.tree_leaf[at * CAT_LEAVES + tid] = k >= 0 ? lr * lv[k] : 0.f;
      }
    }
    if (next_checkpoint < a.NK && t + 1 == a.checkpoint[next_checkpoint]) {
      if (held) a.hold_margin[(pc * a.NK + next_checkpoint) * n + tid] = margin;
      if (is_test) a.test_margin[(pc * a.NK + next_checkpoint) * T + (tid - n)] = margin;
      ++next_checkpoint;
    }
    __syncthreads();      // the tree's last reads of the list are over
  }

  const int any_bad = __syncthreads_or((is_train || is_test) && !cat_finite(margin) ? 1 : 0);
  if (tid == 0) a.status[fit] = any_bad ? PFN_CATBOOST_CV_NONFINITE : PFN_CATBOOST_CV_DONE;
}

int launch_catboost_cv(const CatCvArgs& a, hipStream_t s) {
  static LdsAllowance allowance;
  cat_order_kernel<<<dim3((unsigned)a.F, (unsigned)a.P), dim3(128), 0, s>>>(a.train, a.order, a.n, a.F);
  if (hipGetLastError() != hipSuccess) return PFN_ERR_LAUNCH;
  return launch_lds(catboost_cv_kernel, allowance, dim3(PFN_CATBOOST_CV_SLOTS, (unsigned)a.NC, (unsigned)a.P), dim3(CAT_THREADS), catboost_cv_lds_bytes(a.n, a.F), s, a);
}

}  // namespace
}  // namespace pfn

using namespace pfn;

extern "C" int pfn_catboost_cv(const float* train, const float* labels, const float* test, const int32_t* fold, const int32_t* cand_depth, const float* cand_lr,
                               const float* cand_l2, const int32_t* cand_ids, const int32_t* checkpoints, int P, int n, int T, int F, int NC, int NK, int num_rounds,
                               uint64_t seed, const int64_t* problem_ids, uint8_t* order, float* hold_margin, float* test_margin, int32_t* status,
                               int32_t* tree_feature, float* tree_threshold, float* tree_leaf, void* stream) {
  const char* why = "one block per fit, its rows and their sort orders in LDS";
  // the limits first: the ranges of n, T, F, NC, the tree count, then (the candidates are host arrays) every candidate's depth; then the arguments
  if (const int rc = fold_shapes("catboost_cv", why, 1, n, 128, T, F, NC, PFN_CATBOOST_CV_MAX_CANDIDATES, 0, 0, true)) return rc;
  if (num_rounds < 1 || num_rounds > PFN_CATBOOST_CV_MAX_ROUNDS)
    return fail(PFN_ERR_UNSUPPORTED, "catboost_cv: num_rounds %d outside 1 .. %d", num_rounds, PFN_CATBOOST_CV_MAX_ROUNDS);
  if (cand_depth)
    for (int c = 0; c < NC; ++c)
      if (cand_depth[c] < 1 || cand_depth[c] > PFN_CATBOOST_CV_MAX_DEPTH)
        return fail(PFN_ERR_UNSUPPORTED, "catboost_cv: cand_depth[%d] = %d outside 1 .. %d", c, cand_depth[c], PFN_CATBOOST_CV_MAX_DEPTH);
  if (const int rc = fold_shapes("catboost_cv", why, P, n, 128, T, F, NC, PFN_CATBOOST_CV_MAX_CANDIDATES, 0, 0,
                                 train && labels && test && fold && cand_depth && cand_lr && cand_l2 && checkpoints && order && hold_margin && test_margin && status))
    return rc;
  if ((tree_feature || tree_threshold || tree_leaf) && !(tree_feature && tree_threshold && tree_leaf))
    return fail(PFN_ERR_ARGUMENT, "catboost_cv: tree_feature, tree_threshold and tree_leaf come together or not at all");
  if (NK < 1 || NK > PFN_CATBOOST_CV_MAX_CHECKPOINTS) return fail(PFN_ERR_ARGUMENT, "catboost_cv: %d checkpoints outside 1 .. %d", NK, PFN_CATBOOST_CV_MAX_CHECKPOINTS);
  CatCvArgs a{};
  for (int k = 0; k < NK; ++k) {
    if (checkpoints[k] < 1 || (k > 0 && checkpoints[k] <= checkpoints[k - 1]) || (k == NK - 1 && checkpoints[k] != num_rounds))
      return fail(PFN_ERR_ARGUMENT, "catboost_cv: the checkpoints are ascending tree counts >= 1, the last equal to num_rounds %d", num_rounds);
    a.checkpoint[k] = checkpoints[k];
  }
  for (int c = 0; c < NC; ++c) {
    if (!(cand_lr[c] > 0.f) || !(cand_lr[c] < __builtin_inff()) || !(cand_l2[c] >= 0.f) || !(cand_l2[c] < __builtin_inff()))
      return fail(PFN_ERR_ARGUMENT, "catboost_cv: candidate %d: learning_rate %g must be > 0, l2_leaf_reg %g >= 0, both finite", c, cand_lr[c], cand_l2[c]);
    if (cand_ids && (cand_ids[c] < 0 || cand_ids[c] >= PFN_CATBOOST_CV_MAX_CANDIDATES))
      return fail(PFN_ERR_ARGUMENT, "catboost_cv: cand_ids[%d] = %d outside 0 .. %d", c, cand_ids[c], PFN_CATBOOST_CV_MAX_CANDIDATES - 1);
    a.depth[c] = cand_depth[c];
    a.lr[c] = cand_lr[c];
    a.l2[c] = cand_l2[c];
    a.cand_id[c] = cand_ids ? cand_ids[c] : c;
  }
  a.train = train; a.labels = labels; a.test = test; a.fold = fold; a.P = P; a.n = n; a.T = T; a.F = F; a.NC = NC; a.NK = NK; a.rounds = num_rounds;
  a.seed = seed; a.problem_ids = problem_ids; a.order = order; a.hold_margin = hold_margin; a.test_margin = test_margin; a.status = status;
  a.tree_feature = tree_feature; a.tree_threshold = tree_threshold; a.tree_leaf = tree_leaf;
  PFN_TRY(launch_catboost_cv(a, (hipStream_t)stream));
  return PFN_OK;
}
