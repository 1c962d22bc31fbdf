// The tabular study's evaluation protocol on the device (reference tabular.py:160-370; DESIGN.md section 19, include/pfn_hip.h "Tabular study"):
//   tab_windows_kernel   every (window, test row) column of an eval position gathered from the table and normalised, in the layout the embedding reads;
//   auc_counts_kernel    the integer pair counts ROC-AUC is a ratio of, per column;
//   knn_cv_kernel        k-nearest-neighbour lists (k = 1 .. 5) of every held-out row of every CV fold and of every test row, one block per window.
// Nothing here uses atomics on global memory or a workspace; every result is a function of its own window / column / problem alone, bit for bit.
#include "fold_device.h"      // fold_shapes

namespace pfn {

constexpr int TAB_MAX_FEATURES = 1024;      // table columns whose statistics one block keeps in LDS
struct TabWindowsArgs {
  const float* X;          // [N,F] the table
  const float* y;          // [N]
  const int32_t* starts;   // [W] first row of each window (device); a window that leaves the table is written as NaN, never read
  long N;
  int F, F_out, W, bptt, sep, mode;
  float rescale;
  float* x_out;            // WITH_TEST [sep+1, W T, F_out], TRAIN_ONLY [bptt, W, F_out]
  float* y_out;            // WITH_TEST [sep, W T], TRAIN_ONLY [bptt, W]; or null
};
struct KnnCvArgs {
  const float* train;      // [P,n,F]
  const float* labels;     // [P,n]: class = label > 0.5
  const float* test;       // [P,T,F]
  const int32_t* fold;     // [P,n] in 0 .. 4
  int P, n, T, F;
  int32_t* cv_correct;     // [P,5,5]
  int32_t* test_pos;       // [P,T,5]
  int32_t* test_nbr;       // [P,T,5]
};
// rows of both kinds at an odd stride, then the labels and folds of the train rows: 133,120 bytes at n = T = F = 128
inline size_t knn_cv_lds_bytes(int n, int T, int F) { return (size_t)(n + T) * (F | 1) * 4 + (size_t)n * 8; }

namespace {

#define TAB_DEV __device__ __forceinline__

// ---- windows -------------------------------------------------------------------------------------------------------------------------------------------------
// grid (W, row chunks), 256 threads.  Every block first reduces ITS window's sep train rows per feature (thread = feature, rows streamed: coalesced over the
// features): the mean m0 by a sum and a centred correction, the second moment about m0, the minimum and the maximum -- f64 accumulators, no sum of squares
// of the raw values anywhere.  Then it writes its TAB_ROWS output rows.  WITH_TEST: a thread owns (test row t, VEC features), folds that one test value into
// (m0, M2) by the one-step Welford update, and walks the block's rows with mean and std in registers.  The row chunks only split the writing; a column's
// statistics are the same numbers in whichever block they are formed.
constexpr int TAB_ROWS = 8;

struct TabStat { double m0, M2; float mn, mx; };

template <int VEC> TAB_DEV void tab_store(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

template <int VEC> __global__ void __launch_bounds__(256) tab_windows_kernel(TabWindowsArgs a) {
  __shared__ TabStat st[TAB_MAX_FEATURES];
  const int w = blockIdx.x, F = a.F, Fo = a.F_out, sep = a.sep, T = a.bptt - a.sep;
  const int rows_out = a.mode == PFN_TAB_NORM_WITH_TEST ? sep + 1 : a.bptt;
  const int r0 = blockIdx.y * TAB_ROWS, r1 = min(r0 + TAB_ROWS, rows_out);
  const long start = a.starts[w];
  const bool inside = start >= 0 && start + a.bptt <= a.N;      // a window that leaves the table is never read: its columns are NaN
  const float* X = a.X + (inside ? start : 0) * F;
  const float* Y = a.y + (inside ? start : 0);
  if (inside) {
    for (int f = threadIdx.x; f < F; f += blockDim.x) {
      double s = 0.;
      float mn = X[f], mx = mn;
      for (int r = 0; r < sep; ++r) {
        const float v = X[(long)r * F + f];
        s += (double)v;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
      }
      const double m = s / sep;
      double d1 = 0., d2 = 0.;
      for (int r = 0; r < sep; ++r) {
        const double d = (double)X[(long)r * F + f] - m;
        d1 += d;
        d2 += d * d;
      }
      st[f].m0 = m + d1 / sep;
      st[f].M2 = d2 - d1 * d1 / sep;
      st[f].mn = mn;
      st[f].mx = mx;
    }
  }
  __syncthreads();
  const float nan = __builtin_nanf("");
  if (a.mode == PFN_TAB_NORM_WITH_TEST) {
    const long cols = (long)a.W * T;
    const int groups = Fo / VEC;
    for (int it = threadIdx.x; it < T * groups; it += blockDim.x) {
      const int t = it / groups, f0 = (it - t * groups) * VEC;
      float mean[VEC], sd[VEC], xt[VEC];
      bool live[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const int f = f0 + v;
        live[v] = false;
        mean[v] = 0.f; sd[v] = 1.f; xt[v] = 0.f;
        if (f < F && inside) {
          const TabStat q = st[f];
          xt[v] = X[(long)(sep + t) * F + f];
          const double delta = (double)xt[v] - q.m0, mu = q.m0 + delta / (sep + 1);
          const double M2 = q.M2 + delta * ((double)xt[v] - mu);
          mean[v] = (float)mu;
          sd[v] = (float)sqrt(fmax(M2, 0.) / sep) + 1e-6f;
          live[v] = fminf(q.mn, xt[v]) != fmaxf(q.mx, xt[v]);      // all sep + 1 values bit-equal: exactly 0
        }
      }
      const long col = (long)w * T + t;
      for (int r = r0; r < r1; ++r) {
        float o[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const int f = f0 + v;
          float x = 0.f;
          if (live[v]) x = r < sep ? X[(long)r * F + f] : xt[v];
          o[v] = live[v] ? ((x - mean[v]) / sd[v]) / a.rescale : 0.f;
          if (!inside) o[v] = nan;
        }
        tab_store<VEC>(a.x_out + ((long)r * cols + col) * Fo + f0, o);
      }
    }
    if (a.y_out)
      for (int it = threadIdx.x; it < (r1 - r0) * T; it += blockDim.x) {
        const int r = r0 + it / T, t = it % T;
        if (r < sep) a.y_out[(long)r * cols + (long)w * T + t] = inside ? Y[r] : nan;
      }
  } else {
    const int groups = Fo / VEC;
    for (int it = threadIdx.x; it < (r1 - r0) * groups; it += blockDim.x) {
      const int r = r0 + it / groups, f0 = (it % groups) * VEC;
      float o[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const int f = f0 + v;
        o[v] = 0.f;
        if (f < F && inside) {
          const TabStat q = st[f];
          if (q.mn != q.mx) {
            const float sd = (float)sqrt(fmax(q.M2, 0.) / (sep - 1)) + 1e-6f;
            o[v] = (X[(long)r * F + f] - (float)q.m0) / sd;
          }
        }
        if (!inside) o[v] = nan;
      }
      tab_store<VEC>(a.x_out + ((long)r * a.W + w) * Fo + f0, o);
    }
    if (a.y_out)
      for (int r = r0 + threadIdx.x; r < r1; r += blockDim.x) a.y_out[(long)r * a.W + w] = inside ? Y[r] : nan;
  }
}

// ---- AUC counts ----------------------------------------------------------------------------------------------------------------------------------------------
// One block per column: 64 threads (one wave) up to 64 rows, 256 beyond.  The column is staged in LDS; a thread takes the positives among its rows and counts,
// against every negative (a broadcast read), the pairs it wins and the pairs it ties.  Integer counts: the block's sum has no order.
constexpr int AUC_MAX_T = 4096;

__global__ void __launch_bounds__(256) auc_counts_kernel(const float* scores, const float* labels, int T, int C, long long* counts) {
  __shared__ float sc[AUC_MAX_T];
  __shared__ unsigned char pos[AUC_MAX_T];
  __shared__ long long red[4][4];
  const int c = blockIdx.x;
  for (int i = threadIdx.x; i < T; i += blockDim.x) {
    sc[i] = scores[(long)i * C + c];
    pos[i] = labels[(long)i * C + c] > 0.5f;
  }
  __syncthreads();
  long long v[4] = {0, 0, 0, 0};      // P, Nn, gt, eq
  for (int i = threadIdx.x; i < T; i += blockDim.x) {
    if (!pos[i]) { v[1] += 1; continue; }
    v[0] += 1;
    const float s = sc[i];
    int gt = 0, eq = 0;
    for (int j = 0; j < T; ++j) {
      const bool neg = !pos[j];
      const float o = sc[j];
      gt += (neg && s > o);
      eq += (neg && s == o);
    }
    v[2] += gt;
    v[3] += eq;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v[q];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    long long s = 0;
    for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) s += red[wv][threadIdx.x];
    counts[(long)c * 4 + threadIdx.x] = s;
  }
}

// ---- kNN with its cross-validation ---------------------------------------------------------------------------------------------------------------------------
// One block of 256 threads per problem.  LDS: the n train rows and the T test rows at a row stride of F | 1 floats (odd: thread q reading its own row q and its
// neighbours theirs fall on different banks; the train row every thread compares against is one address, a broadcast), labels and folds.  Thread q < n is the
// held-out query "train row q" (it skips the train rows of its own fold), thread n + t the test row t (it skips nothing).  Four train rows per pass share one
// read of the query's feature; each row's squared distance is an f32 fma chain in ascending feature order; rows enter the sorted five-deep list in ascending
// index with a strict comparison, so equal distances keep the lower index in front.  The five prefixes of that list are the neighbours for k = 1 .. 5.
constexpr int KNN_K = 5, KNN_FOLDS = 5, KNN_JT = 4;

__global__ void __launch_bounds__(256) knn_cv_kernel(KnnCvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float knn_lds[];
  __shared__ int correct[KNN_K * KNN_FOLDS];
  const int n = a.n, T = a.T, F = a.F, Fs = F | 1, p = blockIdx.x, q = threadIdx.x;
  float* rows = knn_lds;                                   // [n + T][Fs]
  int* cls = reinterpret_cast<int*>(rows + (n + T) * Fs);  // [n]
  int* fold = cls + n;                                     // [n]
  const float* xtr = a.train + (long)p * n * F;
  const float* xte = a.test + (long)p * T * F;
  for (int i = threadIdx.x; i < (n + T) * F; i += blockDim.x) {
    const int r = i / F, f = i - r * F;
    rows[r * Fs + f] = r < n ? xtr[i] : xte[i - n * F];
  }
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    cls[i] = a.labels[(long)p * n + i] > 0.5f;
    fold[i] = a.fold[(long)p * n + i];
  }
  if (threadIdx.x < KNN_K * KNN_FOLDS) correct[threadIdx.x] = 0;
  __syncthreads();
  const bool active = q < n + T, cv = q < n;
  const int my_fold = cv ? fold[q] : -1;
  const float* mine = rows + (active ? q : 0) * Fs;
  float bd[KNN_K];
  int bi[KNN_K];
#pragma unroll
  for (int k = 0; k < KNN_K; ++k) { bd[k] = __builtin_inff(); bi[k] = -1; }
  for (int j0 = 0; j0 < n; j0 += KNN_JT) {
    const float* other[KNN_JT];
    float d[KNN_JT];
#pragma unroll
    for (int u = 0; u < KNN_JT; ++u) { other[u] = rows + min(j0 + u, n - 1) * Fs; d[u] = 0.f; }
    for (int f = 0; f < F; ++f) {
      const float x = mine[f];
#pragma unroll
      for (int u = 0; u < KNN_JT; ++u) {
        const float e = x - other[u][f];
        d[u] = __builtin_fmaf(e, e, d[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < KNN_JT; ++u) {
      const int j = j0 + u;
      if (j >= n || (cv && fold[j] == my_fold)) continue;
      float cd = d[u];
      int ci = j;
      bool moved = false;
#pragma unroll
      for (int k = 0; k < KNN_K; ++k) {
        moved = moved || cd < bd[k];
        if (moved) {
          const float td = bd[k]; const int ti = bi[k];
          bd[k] = cd; bi[k] = ci;
          cd = td; ci = ti;
        }
      }
    }
  }
  if (active) {
    int npos = 0;
    const int truth = cv ? cls[q] : 0;
    int* tp = a.test_pos + ((long)p * T + (q - n)) * KNN_K;
    int* tn = a.test_nbr + ((long)p * T + (q - n)) * KNN_K;
#pragma unroll
    for (int k = 0; k < KNN_K; ++k) {
      npos += bi[k] >= 0 ? cls[bi[k]] : 0;
      if (cv) {
        const int pred = 2 * npos > k + 1;      // a split vote at even k is class 0
        if (bi[k] >= 0 && pred == truth && my_fold >= 0 && my_fold < KNN_FOLDS) atomicAdd(&correct[k * KNN_FOLDS + my_fold], 1);
      } else {
        tp[k] = npos;
        tn[k] = bi[k];
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < KNN_K * KNN_FOLDS) a.cv_correct[(long)p * KNN_K * KNN_FOLDS + threadIdx.x] = correct[threadIdx.x];
}

int launch_tab_windows(const TabWindowsArgs& a, hipStream_t s) {
  const int rows_out = a.mode == PFN_TAB_NORM_WITH_TEST ? a.sep + 1 : a.bptt;
  const dim3 grid((unsigned)a.W, (unsigned)((rows_out + TAB_ROWS - 1) / TAB_ROWS));
  if (a.F_out % 4 == 0) tab_windows_kernel<4><<<grid, 256, 0, s>>>(a);      // x_out comes 16-byte aligned (pfn_tabular_windows checks it)
  else tab_windows_kernel<1><<<grid, 256, 0, s>>>(a);
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

int launch_auc_counts(const float* scores, const float* labels, int T, int C, int64_t* counts, hipStream_t s) {
  auc_counts_kernel<<<dim3((unsigned)C), dim3(T <= 64 ? 64 : 256), 0, s>>>(scores, labels, T, C, reinterpret_cast<long long*>(counts));
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

int launch_knn_cv(const KnnCvArgs& a, hipStream_t s) {
  static LdsAllowance allowance;
  return launch_lds(knn_cv_kernel, allowance, dim3((unsigned)a.P), dim3(256), knn_cv_lds_bytes(a.n, a.T, a.F), s, a);
}

}  // namespace
}  // namespace pfn

using namespace pfn;

extern "C" {
int pfn_tabular_windows(const float* X, const float* y, const int32_t* starts, int64_t N, int F, int F_out, int W, int bptt, int sep, float rescale, int mode,
                        float* x_out, float* y_out, void* stream) {
  if (F < 1 || F > TAB_MAX_FEATURES || F_out < F)
    return fail(PFN_ERR_UNSUPPORTED, "F %d outside 1 .. %d or F_out %d < F (a block keeps one window's per-feature statistics in LDS)", F, TAB_MAX_FEATURES, F_out);
  if (mode != PFN_TAB_NORM_WITH_TEST && mode != PFN_TAB_NORM_TRAIN_ONLY) return fail(PFN_ERR_ARGUMENT, "unknown tabular_windows mode %d", mode);
  if (N < 1 || W < 1 || sep < 1 || sep > bptt || (mode == PFN_TAB_NORM_WITH_TEST && sep == bptt) || bptt > 65536 || !(rescale > 0.f))
    return fail(PFN_ERR_ARGUMENT, "bad tabular_windows arguments (N %lld >= 1, W %d >= 1, 1 <= sep %d <%s bptt %d <= 65536, rescale %g > 0)", (long long)N, W, sep,
                mode == PFN_TAB_NORM_WITH_TEST ? "" : "=", bptt, (double)rescale);
  if (!X || !y || !starts || !x_out) return fail(PFN_ERR_ARGUMENT, "bad tabular_windows arguments (X, y, starts, x_out not NULL)");
  if ((uintptr_t)x_out % 16) return fail(PFN_ERR_ALIGNMENT, "tabular_windows: x_out must be 16-byte aligned");
  TabWindowsArgs a{};
  a.X = X; a.y = y; a.starts = starts; a.N = N; a.F = F; a.F_out = F_out; a.W = W; a.bptt = bptt; a.sep = sep; a.mode = mode; a.rescale = rescale;
  a.x_out = x_out; a.y_out = y_out;
  PFN_TRY(launch_tab_windows(a, (hipStream_t)stream));
  return PFN_OK;
}
int pfn_auc_counts(const float* scores, const float* labels, int T, int C, int64_t* counts, void* stream) {
  if (T < 1 || T > 4096) return fail(PFN_ERR_UNSUPPORTED, "auc_counts: T %d outside 1 .. 4096 (a block stages one column in LDS)", T);
  if (C < 1 || !scores || !labels || !counts) return fail(PFN_ERR_ARGUMENT, "bad auc_counts arguments (C %d >= 1, scores, labels, counts not NULL)", C);
  PFN_TRY(launch_auc_counts(scores, labels, T, C, counts, (hipStream_t)stream));
  return PFN_OK;
}
int pfn_knn_cv(const float* train, const float* labels, const float* test, const int32_t* fold, int P, int n, int T, int F, int32_t* cv_correct, int32_t* test_pos,
               int32_t* test_nbr, void* stream) {
  if (const int rc = fold_shapes("knn_cv", "one thread per query, every row in LDS", P, n, 128, T, F, 0, 0, 0, 0,
                                 train && labels && test && fold && cv_correct && test_pos && test_nbr)) return rc;
  KnnCvArgs a{};
  a.train = train; a.labels = labels; a.test = test; a.fold = fold; a.P = P; a.n = n; a.T = T; a.F = F; a.cv_correct = cv_correct; a.test_pos = test_pos; a.test_nbr = test_nbr;
  PFN_TRY(launch_knn_cv(a, (hipStream_t)stream));
  return PFN_OK;
}
}  // extern "C"
