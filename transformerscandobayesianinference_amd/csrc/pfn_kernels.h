// Internal (C++) launcher interface between the kernels of the transformer stack (gemm.hip, gemm_tn.hip, attention.hip, rowwise.hip) and its schedules
// (pfn_api.hip).  Every other .hip file defines its own entry points beside its kernels and needs only pfn_host.h.
// Nothing here crosses the shared-library boundary; see include/pfn_hip.h for the exported ABI.
#pragma once
#include "pfn_host.h"

namespace pfn {

// host-side dispatch of a statement over the operand type T (device code only sees the instantiations)
#define PFN_DISPATCH_OP(prec, ...)                                                          \
  do {                                                                                      \
    if ((prec) == PFN_PREC_BF16) { using T = ::pfn::bf16_t; __VA_ARGS__; }                  \
    else if ((prec) == PFN_PREC_FP16) { using T = ::pfn::f16_t; __VA_ARGS__; }              \
    else { using T = float; __VA_ARGS__; }                                                  \
  } while (0)
typedef __bf16 bf16_t;
typedef _Float16 f16_t;

// ---------------------------------------------------------------------------------------------
// Dropout masks (training with dropout > 0: TransformerEncoderLayer's four sites, reference transformer.py:17 / train.py:22).
// A mask is a pure function of (site seed, i, j) so the backward regenerates what the forward applied, in whatever register
// layout a kernel holds the elements, with no mask tensor in HBM:
//     keep(s, i, j)  <=>  mix32(s ^ i * 0x9E3779B1 ^ j * 0x85EBCA77) >= thr,      thr = p * 2^32
// (mix32: pfn_host.h).  site seed = dropout_site_seed(call seed, layer, site); the attention site mixes the
// (dataset, head) index in as well (dropout_pair_seed).  i, j = (query, key) for the attention probabilities, (token row b * S + t,
// column) for the three element-wise sites.  oracle/pfn_oracle.py restates the same integers in numpy.
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline unsigned dropout_site_seed(unsigned long long seed, int layer, int site) {
  return mix32(mix32((unsigned)seed ^ (0x9E3779B1u * (unsigned)(layer * 4 + site + 1))) ^ (unsigned)(seed >> 32));
}
__host__ __device__ inline unsigned dropout_pair_seed(unsigned site_seed, int pair) { return mix32(site_seed ^ (0xC2B2AE35u * (unsigned)(pair + 1))); }
__host__ __device__ inline unsigned dropout_threshold(float p) {
  const double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 0xffffffffu : (unsigned)t;
}
__host__ __device__ inline bool dropout_keep(unsigned s, unsigned i, unsigned j, unsigned thr) {
  return mix32(s ^ (i * 0x9E3779B1u) ^ (j * 0x85EBCA77u)) >= thr;
}

// ---- GEMM -----------------------------------------------------------------------------------
enum : int {
  EPI_BIAS = 1,      // + bias[n] (f32)
  EPI_GELU = 2,      // out = gelu(v)   (exact erf GELU, torch nn.GELU default)
  EPI_GELU_BWD = 4,  // v *= aux[m,n] (T): the GELU derivative the forward GEMM stored (EPI_GELU | EPI_OUT2_T)
  EPI_RESID = 8,     // + resid[m,n] (f32)
  EPI_OUT_F32 = 16,  // store f32
  EPI_OUT_T = 32,    // store operand type T
  EPI_OUT2_T = 64,   // second T output: with EPI_GELU the GELU DERIVATIVE at the pre-activation, else the value before the activation
  EPI_ACCUM = 128,   // out_f32 += v
  EPI_RESID_T = 256, // + aux[m,n] (T): residual taken from an operand-precision tensor (not with EPI_GELU_BWD)
  // (LDS-DMA 256 / 128 x 256 kernels only; gemm_nt_rowdot_fused tells the caller beforehand)  rowdot[b, head, i] += sum over the tile's columns of
  // out_t[m, n] * aux[m, n], m = b * rd_S + i, head = n / rd_D -- the attention backward's delta = rowsum(dO . O) taken while d(ctx) leaves the GEMM that
  // produces it (aux = the forward's context rows), with f32 atomics (two 64-column waves per head of 128: two addends, order-free; the caller zeroes rowdot);
  // the wave that owns a head's first columns also writes lse2 = lse * log2(e) behind it (what attn_delta_kernel did)
  EPI_ROWDOT = 512,
  // out[m, n] -= rowshift[(m / rs_S) * rs_ld + (n - rs_n0)] for rs_n0 <= n < rs_n1: a per-DATASET shift of a column range, applied in f32 before the value is
  // rounded to operand precision -- the key centring of the q|k|v projection (launch_key_shift below; pfn_api.hip).  rs_n0, rs_n1 multiples of 64.
  EPI_ROWSHIFT = 1024,
};

struct GemmNT {
  const void* A; long lda;  // [M,K] T
  const void* B; long ldb;  // [N,K] T
  int M, N, K;
  int flags;
  const float* bias;
  const void* aux; long ld_aux;
  const float* resid; long ld_resid;
  float* out_f32; long ld_out_f32;
  void* out_t; long ld_out_t;
  void* out2_t; long ld_out2;
  int vec_ok;  // filled by the launcher
  int wide_t;  // filled by the launcher: operand-precision outputs may be stored 16 bytes at a time
  // EPI_ROWDOT: rowdot [B, H, S] f32 (+ lse2 [B, H, S] behind it at rd_lse2_off), lse [B, H, S]; rows m = b * rd_S + i, heads of rd_D columns
  float* rowdot; const float* rd_lse; long rd_lse2_off; int rd_S, rd_H, rd_D;
  // EPI_ROWSHIFT: rowshift [M / rs_S, rs_ld] f32
  const float* rowshift; long rs_ld; int rs_S, rs_n0, rs_n1;
};
// Key centring (round 6).  softmax_j(q_i . k_j) does not change when ONE vector c is subtracted from every key of a (dataset, head): q_i . (k_j - c) = q_i . k_j - q_i . c,
// a constant along j (the self key of a test row is shifted like the others).  In a trained PFN the keys of a dataset share a large common component (measured on
// tests/golden/trained_config1.pt: |k| rms 6.6, |k - mean_j k| rms 0.73) and the 16-bit rounding of k is relative to |k|, not to the part that matters: storing
// k' = k - c with c ~ the dataset's mean key makes the attention 9 x less sensitive to the operand rounding of K (profiles/r06_operand_format_simulation.json: bf16
// forward 5e-2 -> 2e-2, fp16 7e-3 -> 2.5e-3 on that checkpoint).  The backward needs nothing: sum_j dS_ij = 0, so dK' = dK and d(c) = 0 (the reference's gradient).
// c = W_k xbar with xbar the mean of a strided SAMPLE of the dataset's TRAIN rows of the layer input (any c is exact; this one removes the common part to ~ 1 / sqrt(samples);
// train rows only, so that no test row reaches another row's output even at rounding level):
//   kshift[b, n] = sum_e w_k[n, e] * mean_{t in sample} x[b, t, e]        x [B, S, E] T,  w_k [E, E] T (rows = the K block of in_proj_weight),  kshift [B, E] f32
//   sep / sep_of: the eval position (sep_of [B] on the device for a ragged batch, else nullptr); a dataset without train rows gets a zero shift
int launch_key_shift(const void* x_t, const void* w_k_t, float* kshift, int B, int S, int E, int sep, const int* sep_of, int precision, hipStream_t s);
int launch_gemm_nt(const GemmNT& g, int precision, hipStream_t stream);
bool gemm_nt_rowdot_fused(const GemmNT& g, int precision);   // true: launch_gemm_nt(g) will run a kernel that implements EPI_ROWDOT (else the caller keeps attn_delta_kernel)
// kernel selection knob (tests / profiling): 0 automatic, 1 only the 128x128 kernel, 2 the 256x256 kernel whenever legal
void set_gemm_nt_big_mode(int mode);
void set_gemm_ln_rows64(int on);

struct GemmTN {
  const void* A; long lda;  // [M,P] T
  const void* B; long ldb;  // [M,Q] T
  float* C; long ldc;       // [P,Q] f32
  int M, P, Q;
  int atomic;               // 1: C += (split over M, f32 atomics); 0: C = (single split)
  int m_chunk;              // filled by the launcher
  float* colsum;            // optional [P]: += column sums of A (bias gradient), atomically
  int max_splits;           // 0 = automatic; else an upper bound on the token-axis splits (small C: fewer atomic partial sums)
  const float* scale_amax;  // fp16 backward: C and colsum receive the product times 2^-k (nullptr = 1)
};
int launch_gemm_tn(GemmTN g, int precision, hipStream_t stream);

// Grouped weight-gradient GEMMs (bf16): C_i[P_i,Q_i] (+)= A_i[M,P_i]^T . B_i[M,Q_i] for every problem of the
// group in ONE launch of 256x256 tiles (gemm_tn_big_kernel).  splits: 0 = automatic (1 when the group has
// enough tiles: no atomics, deterministic), > 1 = split the token axis with f32 atomics.
constexpr int TN_GROUP_MAX = 26;
struct TnProblem {
  const void* A; const void* B; float* C; float* colsum;  // colsum: optional [P] += column sums of A
  long lda, ldb, ldc;
  int P, Q;
  int Pv;   // rows of C (and entries of colsum) that exist: 0 = all P; < P when A's last columns are zero padding (P still a multiple of 256)
};
struct GemmTNGroup {
  TnProblem p[TN_GROUP_MAX];
  int tile_start[TN_GROUP_MAX + 1];  // filled by the launcher
  int n, M, splits, m_chunk;
  int debug_mask;                    // filled by the launcher: all ones.  Profiling only (pfn_set_tuning key 1 = wrap rows): a wrap that is a power of two >= the 64-token
                                     // stage gives wrap - 1, and the STAGE row inside a token split wraps there (the operand bases return to the split's first row: cache-resident
                                     // operands, wrong products); any other value leaves the wrap off
  const float* scale_amax;           // fp16 backward: every C and colsum of the group receives its product times 2^-k (nullptr = 1)
};
void set_gemm_tn_debug_wrap(int rows);         // PFN_TUNE_GEMM_TN_WRAP (see GemmTNGroup::debug_mask): powers of two >= 64 only, everything else = off
void set_gemm_tn_group_waves(int waves);       // PFN_TUNE_WGRAD_WAVES: 8 = gemm_tn_big_kernel (eight waves of 128 x 64), 4 = gemm_tn_wide_kernel (four of 128 x 128)
// GEMM + bias + residual + LayerNorm in one kernel (gemm_nt_ln_kernel): one workgroup owns 128 full rows of the
// N = emsize columns, so the row statistics are taken straight from the accumulators:
//     v = A . B^T + bias + r,   y = v (f32, kept for the LayerNorm backward),   x_t = (T) ((v - mean) rstd gamma + beta)
// The residual r is either a plain f32 tensor (resid) or the PREVIOUS LayerNorm's output recomputed on the fly from
// its pre-LN sums and statistics (r = (ry - rmean) rrstd rgamma + rbeta): the f32 LayerNorm output is never stored.
struct GemmLN {
  const void* A; long lda;      // [M,K] bf16
  const void* B; long ldb;      // [N,K] bf16
  int M, N, K;
  const float* bias;            // [N]
  const float* resid;           // [M,N] f32, or nullptr to use the recomputed form below
  const void* ry; const float* rmean; const float* rrstd; const float* rgamma; const float* rbeta;      // ry: f32, or operand precision when y16
  const float* gamma; const float* beta; float eps;
  void* y; float* mean; float* rstd; void* x_t;    // outputs (y: f32, or operand precision when y16)
  float* x_f32;                                    // optional: the LayerNorm output in f32 as well (last layer -> decoder)
  int y16;                                         // fp16 only: y is written, and ry read, in operand precision (half the bytes of this HBM-bound epilogue's two f32 streams)
};
bool gemm_ln_supported(const GemmLN& g);
int launch_gemm_ln(const GemmLN& g, int precision, hipStream_t stream);      // precision: one of the 16-bit formats

// A data-gradient GEMM with the backward of the LayerNorm whose OUTPUT gradient it produces fused in (gemm_nt_lnbwd_kernel):
//   v = A . B^T + aux;  dx_t = LayerNorm backward of v through (y, mean, rstd, gamma);  dgamma += sum_rows v xhat;  dbeta += sum_rows v
struct GemmLNB {
  const void* A; long lda;      // [M,K] bf16
  const void* B; long ldb;      // [N,K] bf16
  int M, N, K;
  const void* aux;              // [M,N] bf16 (row pitch N): the residual-branch gradient added to the product
  const void* y; const float* mean; const float* rstd; const float* gamma;    // the LayerNorm's input [M,N] (f32, or operand precision when y16), row statistics [M], weight [N]
  void* dx_t;                   // [M,N] bf16: gradient w.r.t. the LayerNorm input
  float* dgamma; float* dbeta;  // [N] f32, accumulated with atomics
  const float* scale_amax;      // fp16 backward: dgamma / dbeta leave times 2^-k (dx_t stays in the scaled chain); nullptr = 1
  int y16;                      // y as GemmLN::y16 stored it
};
bool gemm_lnbwd_supported(const GemmLNB& g);
int launch_gemm_lnbwd(const GemmLNB& g, int precision, hipStream_t stream);

bool gemm_tn_group_supported(const TnProblem& p);
int launch_gemm_tn_group(GemmTNGroup g, int precision, hipStream_t stream);

// ---- attention (attention.hip) ---------------------------------------------------------------
// qkv: [B, S, 3E] T (q | k | v, heads contiguous inside each E), ctx: [B, S, E] T,
// lse: [B, H, S] f32 (natural-log LSE of the scaled scores over the allowed keys).
// Allowed keys for query i: j < sep, plus j == i when i >= sep (reference transformer.py:34-41).
struct AttnArgs {
  const void* qkv; void* ctx; float* lse;
  int B, S, E, H, sep;
  // ragged batch (round 5): per-dataset eval positions [B] on the device; then `sep` is their maximum (grid of the key-block pass, dS^T scratch dims) and
  // every workgroup reads its own dataset's position.  nullptr = every dataset at `sep`.
  const int* sep_of;
  int q_from_sep;      // ragged batch with the top layer on the test rows: dataset b skips the queries below sep_of[b] / 256 * 256 (q_begin then = the smallest of them: the grids)
  // The backward's fields and those of a predict pass share their bytes: no kernel reads both, and every other kernel's argument block keeps its layout.
  union {
    struct {      // backward
      const void* dctx; void* dqkv; float* delta;  // delta: [B,H,S] f32 scratch
      void* ds;   // dS^T scratch [B, H, ds_rows, ds_ld] T: written by the key-block pass, read by the query-block pass (attn_bwd_ds_bytes)
      int ds_rows, ds_ld;  // filled by the launcher
      int parts;  // backward launches to run, bit mask over ATTN_BWD_*; 0 = all (profiling entry point pfn_op_attention_bwd_parts)
      int zero_delta;  // the query-block pass (the last reader's successor) leaves delta[b, head, its queries] = 0: the next layer's GEMM epilogue ADDS into it (EPI_ROWDOT)
    };
    struct {      // PREDICT AGAINST A K / V CACHE (launch_attn_fwd_cache; pfn_stack_predict): qkv holds the S = n test rows [B, n, 3E] -- the queries and their own (self)
                  // keys and values -- and `sep` keys per dataset come from the context: K of key j at kv + b * kv_sb + j * kv_ld, its V E elements behind it
      const void* kv; long kv_ld, kv_sb;
      float* part_o;      // more than one split: [nsplit, B, n, E] f32 unnormalised outputs ...
      float* part_ml;     // ... and [nsplit, B, n, H] (running max in log2 units, row sum) pairs; attn_merge_kernel writes ctx from them
      int split_keys;     // filled by the launcher: keys per split (whole tiles); split z = blockIdx.z streams keys [z * split_keys, min(sep, (z + 1) * split_keys))
                          // (ragged context: sep_of above gives every dataset its own key count <= sep; splits beyond it write nothing and the merge skips them)
    };
  };
  int pingpong;  // filled by the launcher (PFN_TUNE_ATTN_PINGPONG): bit 0 forward, bit 1 key-block pass
  // forward with the Q PROJECTION FUSED IN (north_star's "QKV projection + attention as one kernel", the half that can exist: K and V are shared by every query block
  // of a head and stay a GEMM).  xq != nullptr (16-bit operands, head dim <= 128, E % 128 == 0): the workgroup forms its 256 queries' head slice q = x W_q[h]^T + b_q[h]
  // on the matrix cores in the prologue -- W_q[h] through LDS in 128-column chunks, x rows straight from global -- instead of reading them from qkv;
  // q_store != 0 also writes them to qkv's Q columns (training: the backward reads them there).
  const void* xq;      // [B, S, E] T: the layer input (operand copy)
  const void* wq;      // [E, E] T: the Q block of in_proj_weight (rows h * D .. of head h)
  const float* bq;     // [E] f32: the Q block of in_proj_bias
  int q_store;
  // Queries below q_begin are skipped: their context rows / dQ rows are not written and they add nothing to dK and dV (the top encoder
  // layer, whose train rows feed nothing: pfn_api.hip).  The launcher rounds it down to a multiple of 256 (whole query blocks / tiles of every
  // kernel); the caller hands in dctx rows that are ZERO in [that multiple, its own first live row).
  int q_begin;
  // dropout on the attention probabilities (training with dropout > 0): P' = P * keep / (1 - p), keep = dropout_keep(pair seed, query, key)
  float p_drop;            // 0 = off (the kernels without the mask arithmetic run)
  unsigned drop_seed;      // site seed of this layer's attention (dropout_site_seed(call seed, layer, 0)); the kernels mix (dataset, head) in
};
// splits of the key range [0, sep) that launch_attn_fwd_cache runs for n test rows of B datasets (a function of the grid size: few query blocks -> more splits);
// sep < 0: the largest count any sep can give (what a workspace must hold)
int attn_cache_splits(int B, int n, int E, int H, int sep, int precision);
int launch_attn_fwd_cache(const AttnArgs& a, int precision, hipStream_t stream);
void set_attn_cache_split_cap(int splits);      // PFN_TUNE_ATTN_CACHE_SPLITS: 0 = the rule, k > 0 = at most k splits
// Backward of a predict pass's attention w.r.t. the test rows' q | k | v (pfn_stack_predict_backward): the cached keys and values are constants, so nothing
// flows into the context.  S = n test rows per dataset, `sep` cached keys; the splits of the key range follow attn_cache_splits (as the forward's).
struct AttnCacheBwdArgs {
  const void* qkv;        // [B, n, 3E] T: the test rows' q | k | v (forward)
  const void* ctx;        // [B, n, E] T: the attention output O (forward)
  const float* lse;       // [B, H, n] f32: its log-sum-exp (natural units; launch_attn_fwd_cache with AttnArgs::lse)
  const void* dctx;       // [B, n, E] T: dO
  void* dqkv;             // [B, n, 3E] T: out
  const void* kv; long kv_ld, kv_sb;      // the context's K | V rows of this layer (AttnArgs' predict fields)
  float* part_dq;         // more than one split: [nsplit, B, n, E] f32 partial dQ (unscaled), summed in split order by the merge kernel
  int B, S, E, H, sep;
  int split_keys;         // filled by the launcher
  const int* sep_of;      // ragged context: per-dataset key counts [B] on the device (clamped to [0, sep] by the kernels); nullptr = every dataset at `sep`
};
// a ragged context's per-dataset train-row counts clamped to [0, hi] (dst [B] int32 on the device): what the condition pass hands the training-path kernels
int launch_clamp_sep_of(const int* src, int* dst, int B, int hi, hipStream_t stream);
int launch_attn_bwd_cache(const AttnCacheBwdArgs& a, int precision, hipStream_t stream);
void set_attn_pingpong(int mask);
enum : int { ATTN_BWD_DELTA = 1, ATTN_BWD_KV = 2, ATTN_BWD_DQ = 4 };
int64_t attn_bwd_ds_bytes(int B, int S, int H, int precision);   // size of AttnArgs::ds for any sep <= S
int launch_attn_fwd(const AttnArgs& a, int precision, hipStream_t stream);
bool attn_fwd_can_fuse_q(int E, int H, int precision);      // shapes for which AttnArgs::xq is implemented (16-bit operands, head dim <= 128, E % 128 == 0, no dropout)
int launch_attn_bwd(const AttnArgs& a, int precision, hipStream_t stream);

// ---- row-wise / element-wise kernels (rowwise.hip) --------------------------------------------
int launch_cast_params(const float* src, void* dst_t, long n, int precision, hipStream_t s);
constexpr int TRANSPOSE_GROUP_MAX = 64;
struct TransposeGroup {     // by value in the kernel arguments: offsets in elements from one source / one destination base
  int n = 0, blocks = 0;
  long src_off[TRANSPOSE_GROUP_MAX], dst_off[TRANSPOSE_GROUP_MAX];
  int rows[TRANSPOSE_GROUP_MAX], cols[TRANSPOSE_GROUP_MAX], ld_dst[TRANSPOSE_GROUP_MAX], first_block[TRANSPOSE_GROUP_MAX];
};
void transpose_group_add(TransposeGroup& g, long src_off, long dst_off, int rows, int cols, int ld_dst);
int launch_transpose_cast_group(const float* src, void* dst, const TransposeGroup& g, int precision, hipStream_t s);
int launch_transpose_cast(const float* src, void* dst_t, int rows, int cols, long ld_dst, int precision, hipStream_t s);
// dst[r, 0:C] = (T) src[r, 0:C], dst[r, C:ld_dst] = 0
int launch_cast_rows(const float* src, long ld_src, void* dst_t, long ld_dst, long R, int C, int precision, hipStream_t s, const float* scale_amax = nullptr);
// ---- loss scale of the fp16 backward (pfn_device.h loss_scale_up / loss_scale_down): `scale_amax` arguments below point at ONE device float holding
// max|incoming gradient| (launch_absmax), from which every kernel derives the same power of two; nullptr = no scaling (bf16 / f32) ----
int launch_absmax(const float* x, long n, float* amax, hipStream_t s);      // amax[0] = max |x[i]| (x 4-byte aligned: a head in front of the first 16-byte boundary is read by scalar loads)
int set_loss_scale_target(int log2_target);      // PFN_TUNE_LOSS_SCALE_TARGET
int launch_scale_copy(const float* src, float* dst, long n, const float* scale_amax, hipStream_t s);    // dst = src * 2^k

// x:[T,B,nf] (strides given in elements), y:[T,B]; out f32 + T in [B,S,E]
struct EmbedArgs {
  const float* x; long x_st, x_sb;  // x[t,b,f] = x[t*x_st + b*x_sb + f]
  const float* y; long y_st, y_sb;
  const float* wx; const float* bx;  // [E,nf], [E]
  const float* wy; const float* by;  // [E,1],  [E]
  float* out_f32; void* out_t;
  void* xaug_t;   // optional [B*S, xaug_ld] T: the token's features, masked y, train flag, zero padding -- the B operand of the backward's GEMM
  int xaug_ld;    // columns of xaug_t: emb_aug_width(nf)
  const float* xaug_amax;   // optional [xaug_ld]: max|.| of every column of xaug_t (launch_embed_colmax); column f is then stored times 2^-xaug_col_exp(f)
  int S, B, nf, E, sep;
  const int* sep_of;   // ragged batch: per-dataset eval positions [B] on the device (then `sep` is unused); nullptr = every dataset at `sep`
};
// the widest encoder: embed_fwd_kernel stages 16 tokens x (nf + 2) f32 in at most 64 KB of LDS (check_desc; include/pfn_hip.h num_features)
constexpr int EMB_MAX_FEATURES = 1022;
// columns of xaug_t / of the [E, aug] gradient accumulator: num_features + 2 rounded up to 32, 64 or 128 (the GEMM form of the embedding backward; 0 = wider
// encoders keep the register kernel).  Round 6: 64 and 128 added -- BASELINE configs[3] has 60 features and spent 9 % of its kernel time in embed_bwd_wide_kernel
__host__ __device__ inline int emb_aug_width(int nf) { return nf + 2 <= 32 ? 32 : nf + 2 <= 64 ? 64 : nf + 2 <= 128 ? 128 : 0; }
int launch_embed_fwd(const EmbedArgs& a, int precision, hipStream_t s);
// fp16 xaug_t: amax[f] = max|column f| over the batch for the features and the masked y (a.xaug_ld floats, zeroed here; the train flag column and the padding stay 0).
// Each column is stored in xaug_t times a power of two that brings its maximum into [1, 2): feature scales far from 1 neither round to fp16 subnormals nor
// saturate, and embed_grad_scatter multiplies the same power back out exactly.  The logits never see it (the forward reads x in f32)
int launch_embed_colmax(const EmbedArgs& a, float* amax, hipStream_t s);
__device__ inline int xaug_col_exp(const float* amax, int f) {
  if (!amax) return 0;
  const float m = amax[f];
  if (!(m > 0.f) || !(m <= 3.402823466e38f)) return 0;     // (an all-zero column, or a NaN / inf in it: unscaled)
  const int e = ilogbf(m);
  return e < -126 ? -126 : e;
}
// backward: dsrc [B,S,E] f32 -> dwx, dbx, dwy, dby (accumulated, f32)
struct EmbedBwdArgs {
  const float* dsrc; const float* x; long x_st, x_sb; const float* y; long y_st, y_sb;
  float* dwx; float* dbx; float* dwy; float* dby;
  int S, B, nf, E, sep;
  const int* sep_of;    // ragged batch: per-dataset eval positions [B] (nullptr = every dataset at `sep`)
  int single_block;     // 1: every workgroup walks every token (one writer per gradient element: PFN_SCHED_DETERMINISTIC)
  const float* scale_amax;   // fp16 backward: dsrc carries the loss scale, the gradients leave without it (nullptr = none)
};
int launch_embed_bwd(const EmbedBwdArgs& a, hipStream_t s);
// the GEMM form: acc[E, aug] = d(src)^T . xaug (launch_gemm_tn), aug = emb_aug_width(nf) -> dwx += acc[:, :nf], dwy += acc[:, nf], dby += acc[:, nf + 1]
// (xaug_amax: the column scales of xaug_t, multiplied back out; nullptr = none)
int launch_embed_grad_scatter(const float* acc, float* dwx, float* dwy, float* dby, int E, int nf, const float* xaug_amax, hipStream_t s);
// input gradients of the fused embedding: dx[t, b, :] = d(src)[b S + t] . W_enc ([E] x [E, nf]) and, for t < sep, dy[t, b] = d(src)[b S + t] . w_y (0 for t >= sep)
struct EmbedInGradArgs {
  const void* dsrc; int dsrc_prec;       // [B S, E] rows b S + t: f32 (PFN_PREC_F32) or operand precision
  const float* wx; const float* wy;      // encoder.weight [E, nf], y_encoder.weight [E]
  float* dx; long dx_st, dx_sb;          // [S, B, nf] (strides in elements)
  float* dy; long dy_st, dy_sb;          // nullptr: no y gradient
  int S, B, nf, E, sep;
  const float* scale_amax;               // fp16 backward: d(src) carries the loss scale, dx / dy leave without it (nullptr = none)
};
int launch_embed_input_grad(const EmbedInGradArgs& a, hipStream_t s);

// src given in the reference layout [S,B,E] f32 (custom encoders): copy into [B,S,E] f32 + T
int launch_sbe_to_bse(const float* src, float* out_f32, void* out_t, int S, int B, int E, int precision, hipStream_t s);
int launch_bse_to_sbe(const float* src_bse, float* dst_sbe, int S, int B, int E, hipStream_t s, const float* scale_amax = nullptr);      // (* 2^-k)

// y = LN(x) * gamma + beta over E; writes f32 and T copies, mean/rstd per row
int launch_layernorm_fwd(const void* x, const float* gamma, const float* beta, float* y_f32, void* y_t,
                         float* mean, float* rstd, long rows, int E, float eps, int precision, hipStream_t s, int x_is_t = 0);      // x_is_t: x in operand precision
// dx = LN'(dy) (dy f32, or T when dy_is_t); dx written f32 + T; dgamma/dbeta accumulated with atomics; optional dbias_extra
// accumulates colsum(dx) (the bias gradient of the linear that produced x's pre-LN sum).
int launch_layernorm_bwd(const void* dy, int dy_is_t, const void* x, const float* gamma, const float* mean, const float* rstd,
                         float* dx_f32, void* dx_t, float* dgamma, float* dbeta, float* dbias_extra,
                         long rows, int E, int precision, hipStream_t s, float* partials = nullptr, const float* scale_amax = nullptr, int x_is_t = 0);      // x_is_t: x in operand precision (GemmLN::y16);      // scale_amax: dgamma / dbeta / dbias_extra leave times 2^-k
// `partials` (PFN_SCHED_DETERMINISTIC): scratch of LNB_MAX_BLOCKS * 3 * E floats -- every workgroup leaves its column sums there and a second tiny launch adds
// them to dgamma / dbeta / dbias_extra in block order (one writer per element, a fixed summation order) instead of the f32 atomics
constexpr int LNB_MAX_BLOCKS = 512;
// out[n] += sum_m a[m,n]
int launch_colsum(const void* a_t, long lda, long rows, int cols, float* out, int precision, hipStream_t s);

// gather test rows: dst[(s-sep)*B + b, :] = src[b, s, :]  (f32 in, T out)  and its transpose
// ---- element-wise dropout (training with dropout > 0 only; masks: pfn_device.h dropout_keep with i = row, j = column) ----
// y[r, c] = resid[r, c] + keep * y[r, c] / (1 - p)            (dropout1 / dropout2 of TransformerEncoderLayer, in place on the f32 sum)
int launch_dropout_add(float* y, const float* resid, long rows, int cols, unsigned site_seed, float p, hipStream_t s);
// dst[r, c] = keep * src[r, c] / (1 - p) in operand precision; src == dst allowed; a second pair shares the mask (h and gelu'(hpre))
int launch_dropout_scale(const void* src, void* dst, const void* src2, void* dst2, long rows, int cols, unsigned site_seed, float p, int precision, hipStream_t s);
int launch_gather_test_rows(const float* src_bse, void* dst_t, int S, int B, int E, int sep, int precision, hipStream_t s);
// ragged batch (per-dataset eval positions sep_of[B], compact rows dataset-major: row_off[b] + (s - sep_of[b]), row_off[B] = total):
// dst[row_off[b] + s - sep_of[b], :] = (T) src[b, s, :] for s >= sep_of[b]   /   dst[b, s, :] = s >= sep_of[b] ? (T) src[row_off[b] + s - sep_of[b], :] : 0
// the top layer's row moves for a ragged batch (compact rows dataset-major): dst[row_off[b] + s - sep_of[b]] = src[b, s] (s >= sep_of[b]);
// dst[b, s] = s >= sep_of[b] ? src[row_off[b] + s - sep_of[b]] : 0 for s >= zero_from(b) = zero_from_block ? sep_of[b] / 256 * 256 : 0; base[b, s, 0 : width] = 0 for s < sep_of[b] / 256 * 256
int launch_gather_rows_ragged(const void* src_bs, void* dst, int S, int B, long row_bytes, const int* sep_of, const long* row_off, hipStream_t s);
int launch_scatter_rows_ragged(const void* src, void* dst_bs, int S, int B, long row_bytes, const int* sep_of, const long* row_off, int zero_from_block, hipStream_t s);
int launch_zero_row_prefix_ragged(void* base, int S, int B, const int* sep_of, long row_bytes, long width_bytes, hipStream_t s);
int launch_gather_test_rows_ragged(const float* src_bse, void* dst_t, int S, int B, int E, const int* sep_of, const long* row_off, int precision, hipStream_t s);
int launch_scatter_test_rows_ragged(const float* src, void* dst_bse_t, int S, int B, int E, const int* sep_of, const long* row_off, int precision, hipStream_t s);
// dst[b, s, :] = (s >= sep) ? src[(s-sep)*B + b, :] : 0
int launch_scatter_test_rows(const float* src, void* dst_bse_t, int S, int B, int E, int sep, int precision, hipStream_t s);
// the same row moves for any operand, as bytes (the top encoder layer runs on the test rows only, pfn_api.hip): compact order [S - sep, B]
int launch_gather_rows(const void* src_bs, void* dst_tb, int S, int B, long row_bytes, int sep, hipStream_t s);
// rows >= sep take the compact rows, rows in [zero_from, sep) zeros, rows below zero_from are not touched
int launch_scatter_rows(const void* src_tb, void* dst_bs, int S, int B, long row_bytes, int sep, int zero_from, hipStream_t s);
// base[b, s, 0 : width_bytes] = 0 for s < nrows
int launch_zero_row_prefix(void* base, int S, int B, int nrows, long row_bytes, long width_bytes, hipStream_t s);

}  // namespace pfn
