// Class-label embedding and pixel encoder of the few-shot study (gfx950): the embedding of a (Linear, CanEmb) model on the matrix cores, forward and backward.
//   src[t, b, :] = Wx . x[t, b, :] + bx + (t < sep ? table[labels[t, b], :] : 0)          (reference transformer.py:68-74 with encoders.CanEmb(1, C, E))
// written as ONE GEMM, the narrow fused embedding's "GEMM form" (pfn_kernels.h emb_aug_width) widened to F <= 1022 features and C <= 1024 classes:
//   A_aug [S B, Kp] = [x | onehot(label) on train rows | 0]      W_aug [E, Kp] = [Wx | table^T | 0]      Kp = F + C rounded up to 64
//   forward   src = A_aug . W_aug^T + bx                          launch_gemm_nt (f32 out in [S, B, E] order: token t B + b -- pfn_stack_forward's src_sbe)
//   backward  dW_aug [E, Kp] = d(src)^T . A_aug                   launch_gemm_tn, its column sums = d(bx); then the scatter
//             dWx += dW_aug[:, :F],  dtable[c, :] += dW_aug[:, F + c],  dbx += colsum
// The kernels here are the HBM-bound ends of that: the two operand packs, the cast of d(src) (fp16: under the power-of-two loss scale of pfn_device.h, taken
// from max|d(src)|) and the gradient scatter, which multiplies the scale back out (a power of two: exact).  Plain C++ only; fp16 stores saturate by an explicit
// clamp at +-65504 and are counted.  The entry points stand below their kernels (include/pfn_hip.h states the contract).
#include <algorithm>
#include "pfn_device.h"
#include "pfn_kernels.h"

namespace pfn {

constexpr int CE_MAX_FEATURES = EMB_MAX_FEATURES, CE_MAX_CLASSES = 1024;
static inline int ce_kp(int F, int C) { return (F + C + 63) / 64 * 64; }
constexpr int CE_F32_K_CHUNK = 128;      // PFN_PREC_F32 forward: columns of K per launch (pfn_class_embed_forward)

PFN_DEV int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// one vector atomic per wave that has something to report
PFN_DEV void ce_report(int* counter, int n) {
  n = wave_sum_int(n);
  if (counter && n > 0 && (threadIdx.x & 63) == 0) atomicAdd(counter, n);
}
// f32 -> operand type; fp16 saturates at the format's largest finite value (a NaN stays a NaN) and counts
template <typename T> PFN_DEV T ce_round(float v, int& saturated) {
  if constexpr (__is_same(T, f16)) {
    if (fabsf(v) > 65504.f) { v = copysignf(65504.f, v); ++saturated; }
  }
  return (T)v;
}
template <typename T> PFN_DEV void ce_store16(T* dst, const float (&v)[16 / sizeof(T)], int& saturated) {
  constexpr int EPC = 16 / sizeof(T);
  T r[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) r[e] = ce_round<T>(v[e], saturated);
  u32x4 w;
  __builtin_memcpy(&w, r, 16);
  *reinterpret_cast<u32x4*>(dst) = w;
}

struct CePackArgs {
  const float* x; long x_st, x_sb;            // x[t, b, f] = x[t x_st + b x_sb + f]
  const long long* labels; long l_st, l_sb;   // labels[t, b] = labels[t l_st + b l_sb]
  void* a_aug;                                // [S B, Kp] T, row t B + b
  int* status;                                // nullptr, or [0] += train-row labels outside [0, C), [1] += saturated fp16 stores
  int B, S, F, C, Kp, sep;
  int x_vec;                                  // x rows may be read 16 bytes at a time
};

// A_aug rows, one 16-byte chunk per thread and step.  The one-hot columns are WRITTEN from the label (no table is read); rows t >= sep get zeros there
// whatever their label is, and so does a train row whose label is outside [0, C) -- counted once, by the chunk that holds column F.
template <typename T> __global__ __launch_bounds__(256) void class_embed_pack_kernel(CePackArgs a) {
  constexpr int EPC = 16 / sizeof(T);
  const int cpr = a.Kp / EPC;
  const long total = (long)a.B * a.S * cpr;
  T* out = reinterpret_cast<T*>(a.a_aug);
  int bad = 0, sat = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long m = i / cpr;
    const int c0 = (int)(i - m * cpr) * EPC;
    const int t = (int)(m / a.B), b = (int)(m - (long)t * a.B);
    const float* xp = a.x + (long)t * a.x_st + (long)b * a.x_sb;
    float v[EPC];
    if (c0 + EPC <= a.F) {
      if (a.x_vec) {
#pragma unroll
        for (int q = 0; q < EPC / 4; ++q) {
          const f32x4 r = *reinterpret_cast<const f32x4*>(xp + c0 + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[4 * q + e] = r[e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < EPC; ++e) v[e] = xp[c0 + e];
      }
    } else {
      const bool train = t < a.sep;
      long long lab = -1;
      if (train && c0 < a.F + a.C) {
        lab = a.labels[(long)t * a.l_st + (long)b * a.l_sb];
        if (lab < 0 || lab >= a.C) {
          if (c0 <= a.F) ++bad;      // (c0 + EPC > F here: this chunk holds column F)
          lab = -1;
        }
      }
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        const int col = c0 + e;
        v[e] = col < a.F ? xp[col] : ((long long)(col - a.F) == lab ? 1.f : 0.f);
      }
    }
    ce_store16<T>(out + m * a.Kp + c0, v, sat);
  }
  ce_report(a.status, bad);
  ce_report(a.status ? a.status + 1 : nullptr, sat);
}

// W_aug [E, Kp] = [Wx | table^T | 0] in operand precision
template <typename T> __global__ __launch_bounds__(256) void class_embed_pack_w_kernel(const float* wx, const float* table, T* w_aug, int* status, int E, int F, int C, int Kp) {
  constexpr int EPC = 16 / sizeof(T);
  const int cpr = Kp / EPC;
  const long total = (long)E * cpr;
  int sat = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int n = (int)(i / cpr), c0 = (int)(i - (long)n * cpr) * EPC;
    float v[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const int col = c0 + e;
      v[e] = col < F ? wx[(long)n * F + col] : (col < F + C ? table[(long)(col - F) * E + n] : 0.f);
    }
    ce_store16<T>(w_aug + (long)n * Kp + c0, v, sat);
  }
  ce_report(status ? status + 1 : nullptr, sat);
}

// d(src) f32 -> operand precision times 2^k (fp16; scale_amax = nullptr: 1), eight elements per thread and step
template <typename T> __global__ __launch_bounds__(256) void class_embed_cast_kernel(const float* dsrc, T* out, long n8, const float* scale_amax) {
  static_assert(sizeof(T) == 2, "the f32 mode reads d(src) where it lies");
  const float sc = loss_scale_up(scale_amax);
  int sat = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(dsrc + 8 * i), hi = *reinterpret_cast<const f32x4*>(dsrc + 8 * i + 4);
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = lo[e] * sc; v[4 + e] = hi[e] * sc; }
    ce_store16<T>(out + 8 * i, v, sat);
  }
}

// the gradients leave dW_aug: one writer per element, so a deterministic GEMM in front gives deterministic gradients
__global__ __launch_bounds__(256) void class_embed_scatter_kernel(const float* dw, const float* colsum, float* dwx, float* dbx, float* dtable, int E, int F, int C, int Kp,
                                                                  const float* scale_amax) {
  const float osc = loss_scale_down(scale_amax);
  const long n_w = dwx ? (long)E * F : 0, n_t = dtable ? (long)C * E : 0, n_b = dbx ? E : 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_w + n_t + n_b; i += (long)gridDim.x * 256) {
    if (i < n_w) {
      const long n = i / F;
      dwx[i] += dw[n * Kp + (i - n * F)] * osc;
    } else if (i < n_w + n_t) {
      const long j = i - n_w, c = j / E, n = j - c * E;
      dtable[j] += dw[n * Kp + F + c] * osc;
    } else {
      const long n = i - n_w - n_t;
      dbx[n] += colsum[n] * osc;
    }
  }
}

static int ce_grid(long items, int cap = 4096) { return (int)std::max<long>(1, std::min<long>((items + 255) / 256, cap)); }
static bool ce_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// one description of the workspace for the size query and both passes
struct CeLayout {
  int Kp;
  int64_t a_aug, w_aug, dsrc_t, dw, colsum, amax, total;
};
static CeLayout ce_layout(int B, int S, int F, int E, int C, int prec) {
  CeLayout l{};
  l.Kp = ce_kp(F, C);
  const int64_t M = (int64_t)B * S, es = prec_esize(prec);
  int64_t off = 0;
  auto carve = [&](int64_t bytes) { const int64_t at = off; off = align_up(off + bytes, 256); return at; };
  l.a_aug = carve(M * l.Kp * es);
  l.w_aug = carve((int64_t)E * l.Kp * es);
  l.dsrc_t = carve(prec_is16(prec) ? M * E * 2 : 0);
  l.dw = carve((int64_t)E * l.Kp * 4);
  l.colsum = carve((int64_t)E * 4);      // (directly behind dw's padded end: one memset clears both)
  l.amax = carve(16);
  l.total = off;
  return l;
}

// the limits every entry point checks first, before a pointer is looked at
static int ce_check_shape(const char* what, int B, int S, int F, int E, int C, int prec) {
  if (prec != PFN_PREC_BF16 && prec != PFN_PREC_F32 && prec != PFN_PREC_FP16) return fail(PFN_ERR_UNSUPPORTED, "%s: prec %d is no PFN_PREC_* value", what, prec);
  if (F < 1 || F > CE_MAX_FEATURES || C < 1 || C > CE_MAX_CLASSES || E < 8 || E % 8)
    return fail(PFN_ERR_UNSUPPORTED, "%s: F %d outside 1 .. %d, C %d outside 1 .. %d, or E %d below 8 / no multiple of 8", what, F, CE_MAX_FEATURES, C, CE_MAX_CLASSES, E);
  if (B < 0 || S < 0 || (int64_t)B * S > 0x7fffffffll) return fail(PFN_ERR_ARGUMENT, "%s: B %d, S %d (both >= 0, B S < 2^31)", what, B, S);
  return PFN_OK;
}

}  // namespace pfn

using namespace pfn;

extern "C" {

int64_t pfn_class_embed_workspace_bytes(int B, int S, int F, int E, int C, int prec) {
  if (const int rc = ce_check_shape("class_embed_workspace_bytes", B, S, F, E, C, prec)) return rc;
  return ce_layout(B, S, F, E, C, prec).total;
}

int pfn_class_embed_forward(const float* x, int64_t x_st, int64_t x_sb, const int64_t* labels, int64_t l_st, int64_t l_sb, const float* wx, const float* bx,
                            const float* table, int B, int S, int F, int E, int C, int sep, int prec, int flags, void* workspace, int64_t workspace_bytes,
                            float* src_sbe, int32_t* status, void* stream) {
  (void)flags;      // (bit 0, deterministic gradients, acts in the backward; the forward has one writer per element anyway)
  if (const int rc = ce_check_shape("class_embed_forward", B, S, F, E, C, prec)) return rc;
  if (sep < 0 || sep > S) return fail(PFN_ERR_ARGUMENT, "class_embed_forward: sep %d outside 0 .. S = %d", sep, S);
  if ((int64_t)B * S == 0) return PFN_OK;
  const CeLayout l = ce_layout(B, S, F, E, C, prec);
  if (!x || !wx || !bx || !table || !workspace || !src_sbe || (!labels && sep > 0) || workspace_bytes < l.total)
    return fail(PFN_ERR_ARGUMENT, "class_embed_forward: a NULL pointer (only status may be NULL; labels when sep = 0), or workspace_bytes %lld below %lld",
                (long long)workspace_bytes, (long long)l.total);
  if (!ce_aligned(workspace, 16) || !ce_aligned(src_sbe, 16) || !ce_aligned(bx, 16) || !ce_aligned(x, 4) || !ce_aligned(wx, 4) || !ce_aligned(table, 4) ||
      !ce_aligned(labels, 8) || !ce_aligned(status, 4))
    return fail(PFN_ERR_ALIGNMENT, "class_embed_forward: workspace, src_sbe and bx 16-byte, labels 8-byte, x, wx, table and status 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  const long M = (long)B * S;
  CePackArgs a{};
  a.x = x; a.x_st = x_st; a.x_sb = x_sb; a.labels = reinterpret_cast<const long long*>(labels); a.l_st = l_st; a.l_sb = l_sb;
  a.a_aug = ws + l.a_aug; a.status = status; a.B = B; a.S = S; a.F = F; a.C = C; a.Kp = l.Kp; a.sep = sep;
  a.x_vec = (ce_aligned(x, 16) && x_st % 4 == 0 && x_sb % 4 == 0) ? 1 : 0;
  const int epc = 16 / prec_esize(prec);
  PFN_DISPATCH_OP(prec, hipLaunchKernelGGL(class_embed_pack_kernel<T>, dim3(ce_grid(M * (l.Kp / epc))), dim3(256), 0, s, a));
  if (hipGetLastError() != hipSuccess) return fail(PFN_ERR_LAUNCH, "class_embed_forward: the A_aug pack did not launch");
  PFN_DISPATCH_OP(prec, hipLaunchKernelGGL(class_embed_pack_w_kernel<T>, dim3(ce_grid((long)E * (l.Kp / epc))), dim3(256), 0, s, wx, table,
                                           reinterpret_cast<T*>(ws + l.w_aug), status, E, F, C, l.Kp));
  if (hipGetLastError() != hipSuccess) return fail(PFN_ERR_LAUNCH, "class_embed_forward: the W_aug pack did not launch");
  GemmNT g{};
  g.A = ws + l.a_aug; g.lda = l.Kp; g.B = ws + l.w_aug; g.ldb = l.Kp; g.M = (int)M; g.N = E; g.K = l.Kp;
  g.flags = EPI_BIAS | EPI_OUT_F32; g.bias = bx; g.out_f32 = src_sbe; g.ld_out_f32 = E;
  if (prec == PFN_PREC_F32 && l.Kp > CE_F32_K_CHUNK) {
    // the parity mode: one f32 accumulator walking K = 1024 in order carries ~ sqrt(K / 2) roundings, several times what a blocked CPU sum does (measured at
    // F = 1022: 9.8e-7 of the largest output against the CPU's 2.6e-7).  Chunks of L = 128 columns added up in src leave ~ sqrt((L + K / L) / 2) of them
    for (int k0 = 0; k0 < l.Kp; k0 += CE_F32_K_CHUNK) {
      GemmNT c = g;
      c.A = reinterpret_cast<const float*>(g.A) + k0; c.B = reinterpret_cast<const float*>(g.B) + k0; c.K = std::min(CE_F32_K_CHUNK, l.Kp - k0);
      if (k0 > 0) c.flags = EPI_OUT_F32 | EPI_ACCUM;
      PFN_TRY(launch_gemm_nt(c, prec, s));
    }
    return PFN_OK;
  }
  PFN_TRY(launch_gemm_nt(g, prec, s));
  return PFN_OK;
}

int pfn_class_embed_backward(const float* dsrc_sbe, const float* wx, int B, int S, int F, int E, int C, int sep, int prec, int flags, void* workspace,
                             int64_t workspace_bytes, float* dwx, float* dbx, float* dtable, void* stream) {
  (void)wx;         // (no gradient reaches x: the weights are not read)
  if (const int rc = ce_check_shape("class_embed_backward", B, S, F, E, C, prec)) return rc;
  if (sep < 0 || sep > S) return fail(PFN_ERR_ARGUMENT, "class_embed_backward: sep %d outside 0 .. S = %d", sep, S);
  if ((int64_t)B * S == 0) return PFN_OK;
  const CeLayout l = ce_layout(B, S, F, E, C, prec);
  if (!dsrc_sbe || !workspace || workspace_bytes < l.total)
    return fail(PFN_ERR_ARGUMENT, "class_embed_backward: dsrc_sbe or workspace NULL, or workspace_bytes %lld below %lld", (long long)workspace_bytes, (long long)l.total);
  if (!ce_aligned(workspace, 16) || !ce_aligned(dsrc_sbe, 16) || !ce_aligned(dwx, 4) || !ce_aligned(dbx, 4) || !ce_aligned(dtable, 4))
    return fail(PFN_ERR_ALIGNMENT, "class_embed_backward: workspace and dsrc_sbe 16-byte, dwx, dbx and dtable 4-byte aligned");
  if (!dwx && !dbx && !dtable) return PFN_OK;
  hipStream_t s = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  const long M = (long)B * S;
  const bool deterministic = (flags & 1) != 0;
  float* amax = prec == PFN_PREC_FP16 ? reinterpret_cast<float*>(ws + l.amax) : nullptr;
  const void* dsrc_op = dsrc_sbe;
  if (prec_is16(prec)) {
    if (amax) PFN_TRY(launch_absmax(dsrc_sbe, M * E, amax, s));
    if (prec == PFN_PREC_FP16) hipLaunchKernelGGL(class_embed_cast_kernel<f16>, dim3(ce_grid(M * E / 8)), dim3(256), 0, s, dsrc_sbe, reinterpret_cast<f16*>(ws + l.dsrc_t), M * E / 8, amax);
    else hipLaunchKernelGGL(class_embed_cast_kernel<bf16>, dim3(ce_grid(M * E / 8)), dim3(256), 0, s, dsrc_sbe, reinterpret_cast<bf16*>(ws + l.dsrc_t), M * E / 8, amax);
    if (hipGetLastError() != hipSuccess) return fail(PFN_ERR_LAUNCH, "class_embed_backward: the d(src) cast did not launch");
    dsrc_op = ws + l.dsrc_t;
  }
  float* dw = reinterpret_cast<float*>(ws + l.dw);
  float* colsum = reinterpret_cast<float*>(ws + l.colsum);
  if (hipMemsetAsync(dw, 0, (size_t)(l.colsum - l.dw) + (size_t)E * 4, s) != hipSuccess) return fail(PFN_ERR_LAUNCH, "class_embed_backward: hipMemsetAsync failed");
  GemmTN g{};
  g.A = dsrc_op; g.lda = E; g.B = ws + l.a_aug; g.ldb = l.Kp; g.C = dw; g.ldc = l.Kp; g.M = (int)M; g.P = E; g.Q = l.Kp;
  g.atomic = deterministic ? 0 : 1;      // deterministic: no token splits, every element of dW_aug and of the column sums has one writer
  g.colsum = colsum;
  g.scale_amax = nullptr;                // the product stays under the loss scale; the scatter takes it out
  PFN_TRY(launch_gemm_tn(g, prec, s));
  hipLaunchKernelGGL(class_embed_scatter_kernel, dim3(ce_grid((long)E * (F + C + 1))), dim3(256), 0, s, dw, colsum, dwx, dbx, sep > 0 ? dtable : nullptr, E, F, C, l.Kp, amax);
  if (hipGetLastError() != hipSuccess) return fail(PFN_ERR_LAUNCH, "class_embed_backward: the gradient scatter did not launch");
  return PFN_OK;
}

}  // extern "C"
