/*
 * pfn_hip.h -- C ABI of libpfn_hip.so, the MI355X (gfx950) implementation of the PFN training
 * hot path of automl/TransformersCanDoBayesianInference.
 *
 * The reference is pure Python and has no FFI of its own; the drop-in
 * boundary is its Python module surface.  Every entry point below names the reference code it
 * replaces (paths relative to the reference checkout).  A binding needs nothing but dlopen /
 * ctypes.CDLL: plain pointers, sizes, and a HIP stream handle passed as void*.
 *
 * Contract (all entry points):
 *   - every pointer is DEVICE memory owned by the caller unless stated otherwise; the library
 *     never allocates or frees device memory and never synchronises the device;
 *   - work is enqueued asynchronously on `stream` (a hipStream_t; NULL = the legacy default stream);
 *   - return value: PFN_OK (0) or a negative PFN_ERR_* code; pfn_last_error_string() gives detail;
 *     no C++ exception crosses the boundary;
 *   - re-entrant for distinct streams.  Everything that decides what a call computes or how its workspace is laid out travels IN the call
 *     (pfn_model_desc incl. its `schedule` bits, shapes, pointers).  The only process-wide mutable state is (a) the per-thread error
 *     string, (b) the TEST / PROFILING hooks pfn_set_tuning and pfn_profile_* below -- kernel-selection and instrumentation switches that
 *     never change a result beyond rounding order or a buffer layout; they are not synchronised and are meant to be set while no call is
 *     in flight (tests, bench.py --tune); production callers never touch them.
 *
 * Internal activation layout is batch-major [B, S, E] (one synthetic dataset = one contiguous
 * block); the reference layout [S, B, ...] is converted at the boundary kernels.
 */
#ifndef PFN_HIP_H
#define PFN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFN_ABI_VERSION 10

enum {
  PFN_OK = 0,
  PFN_ERR_UNSUPPORTED = -1, /* shape / option outside what the kernels implement */
  PFN_ERR_ALIGNMENT = -2,   /* pointer or leading dimension not 16-byte aligned */
  PFN_ERR_LAUNCH = -3,      /* hipGetLastError() after a launch */
  PFN_ERR_ARGUMENT = -4,    /* NULL pointer, negative size, workspace too small ... */
};

enum { PFN_PREC_BF16 = 0, /* bf16 MFMA operands, f32 accumulate / residual / statistics */
       PFN_PREC_F32 = 1,  /* exact-f32 MFMA (v_mfma_f32_32x32x2_f32): parity / debugging mode */
       PFN_PREC_FP16 = 2  /* ABI 8: fp16 MFMA operands (v_mfma_f32_32x32x16_f16: the same rate and bytes as bf16, 11-bit significand -- the format whose
                           * TRAINING forward meets the reference's outputs to 1e-3, profiles/r06_operand_format_simulation.json); f32 accumulate / residual /
                           * statistics as in bf16.  The backward runs under a power-of-two loss scale chosen on the device from max|dlogits| and taken out again where
                           * the gradients are written (csrc/pfn_device.h LossScale): `grads` holds unscaled f32 gradients, as in the other modes. */ };

/* Architecture of TransformerModel (transformer.py:14-26) with the default Linear encoders
 * (encoders.py:8), NoPositionalEncoding (positional_encodings.py:12-18) and the default
 * decoder Linear-GELU-Linear (transformer.py:23). */
typedef struct pfn_model_desc {
  int32_t num_features; /* x-encoder input width (train.py:33); 1 .. 1022: the embedding stages 16 tokens x (num_features + 2) f32 in 64 KB of LDS -- wider is PFN_ERR_UNSUPPORTED */
  int32_t emsize;       /* ninp */
  int32_t nhead;
  int32_t nhid;         /* FFN width and decoder hidden width (transformer.py:17,23) */
  int32_t nlayers;
  int32_t n_out;        /* decoder output width (criterion.num_bars for bar losses, train.py:39) */
  int32_t precision;    /* PFN_PREC_* */
  float ln_eps;         /* 1e-5 (torch LayerNorm default) */
  float dropout;        /* TransformerEncoderLayer's dropout probability (transformer.py:17; train.py:22 default 0.2).  0: no dropout
                         * buffers are carved.  > 0: pfn_stack_forward_dropout / pfn_stack_backward_split(use_dropout = 1) apply it at the
                         * layer's four sites (attention probabilities, after out_proj, after the FFN activation, after linear2);
                         * pfn_stack_forward is the inference pass (model.eval()) and applies none. */
  int32_t schedule;     /* PFN_SCHED_* bits, 0 = the measured defaults.  The schedule is part of the descriptor because it decides the row
                         * layout of some workspace buffers: a forward and the backward that reads its workspace must see the same bits, and
                         * they do when both are given the same descriptor (ABI 6; it was process-global state before). */
} pfn_model_desc;
enum { PFN_SCHED_TOP_LAYER_ALL_ROWS = 1, /* run the TOP encoder layer on every row like the others.  Default (bit clear): everything behind its K / V
                                          * projection runs on the test rows only -- the reference returns output[single_eval_pos:] (transformer.py:91),
                                          * so that layer's train rows feed nothing (not with live dropout, not when sep < S / 4) */
       PFN_SCHED_FUSE_LN_WIDE = 2,       /* emsize 1024: LayerNorm-fused GEMMs on 64-row x 1024-column tiles (correct, measured slower: default off) */
       PFN_SCHED_SEPARATE_LNBWD = 4,     /* LayerNorm backward as its own kernels instead of inside the data-gradient GEMMs that feed it */
       PFN_SCHED_NO_KEY_CENTERING = 16,  /* KEY CENTRING (ABI 8): the keys of every dataset are centred before they are rounded to 16 bits: k' = k - W_k xbar with xbar a sample mean
                                          * of the dataset's TRAIN rows of the layer input.  softmax_j(q_i . k_j) is invariant to one vector subtracted from every key, so outputs and
                                          * gradients are the reference's (transformer.py:84) while the rounding of K stops being relative to the keys' common component (nine
                                          * times their spread on a trained model).  Default: ON with PFN_PREC_FP16 -- this bit turns it off -- and OFF with PFN_PREC_BF16 (the
                                          * arithmetic of rounds 1-5) -- PFN_SCHED_KEY_CENTERING turns it on.  Costs one small kernel + a shifted GEMM epilogue per layer: 0.5 % of the step. */
       PFN_SCHED_KEY_CENTERING = 64,
       PFN_SCHED_F32_RESIDUAL = 128,     /* PFN_PREC_FP16 keeps the pre-LayerNorm sums (the residual the next block adds, the LayerNorm backward's input) in f32 as bf16 does.
                                          * Default (bit clear, fp16, no dropout, emsize 128 / 256 / 512): they are stored in fp16 -- the LayerNorm-fused GEMMs are bound by their
                                          * epilogue's HBM streams and this halves the two f32 ones; LayerNorm itself, its statistics and the operand copy still come from f32 registers.
                                          * Other widths (the LayerNorm as its own kernel): the GEMM ahead of it adds the residual from the operand-precision copy and stores an fp16 sum */
       PFN_SCHED_FUSE_Q_PROJECTION = 32, /* the Q projection runs INSIDE the attention forward kernel (north_star: "QKV projection + scaled-dot-product attention + softmax ... as one
                                          * fused kernel"): a workgroup forms its 256 queries' head slice x W_q[h]^T + b_q[h] on the matrix cores in its prologue, the GEMM in
                                          * front projects k | v only (shared by every query block of a head: they stay a GEMM).  Same Q bits as the GEMM's; 16-bit operands,
                                          * head dim <= 128, emsize % 128 == 0, no live dropout -- otherwise ignored.  Built and measured in round 6 (ABI 8); default off:
                                          * profiles/r06_fused_q_projection.txt */
       PFN_SCHED_DETERMINISTIC = 8       /* bit-reproducible gradients (the reference's CPU loop is deterministic, train.py:58-110): every gradient element has
                                          * exactly ONE writer per launch and launches are stream-ordered -- weight-gradient GEMMs without token splits, LayerNorm
                                          * gamma / beta / bias gradients through per-workgroup partials summed in a fixed order (implies SEPARATE_LNBWD), the
                                          * embedding gradient from one workgroup per column block.  The caller runs ONE backward at a time into a gradient buffer
                                          * (no concurrent micro-batch streams).  Slower (weight gradients under-fill the chip); default off. */ };
/* schedule bits a binding should put into new descriptors: 0 unless a test / profiling run changed the defaults through pfn_set_tuning
 * (PFN_TUNE_FUSE_LNBWD, PFN_TUNE_FUSE_LN_WIDE, PFN_TUNE_TOP_LAYER_TEST_ROWS) */
int pfn_default_schedule(void);

int pfn_abi_version(void);
const char* pfn_last_error_string(void);
/* TEST / PROFILING ONLY: process-wide kernel-selection knobs (results are identical up to rounding order; not synchronised -- set them
 * while no call is in flight).  Keys 2, 5, 6, 12 and 13 do not act on calls directly: they change what pfn_default_schedule() hands to NEW
 * descriptors (pfn_model_desc::schedule), so a forward / backward pair can never disagree about them.
 * PFN_TUNE_GEMM_NT_KERNEL: 0 automatic (default), 1 always the 128x128 register-staged
 * kernel, 2 the 256x256 LDS-DMA kernel whenever the shape is legal for it, 3 the 128x256 one.
 * PFN_TUNE_FUSE_LNBWD: 1 (default) the stack backward runs LayerNorm backward inside the data-gradient GEMMs that feed it
 * (pfn_op_gemm_lnbwd), 0 as separate kernels.  (Key 3, the persistent NT GEMM of round 5, is gone from the product library: csrc/experiments/.)
 * Retired numbers (3, 10, 11) are refused as unknown keys and are not given to a new key. */
enum { PFN_TUNE_GEMM_NT_KERNEL = 0,
       PFN_TUNE_GEMM_TN_WRAP = 1, /* profiling only: > 0 makes the grouped TN kernel re-read its first `value` token rows (wrong results, cache-resident operands) */
       PFN_TUNE_FUSE_LNBWD = 2,
       PFN_TUNE_ATTN_PINGPONG = 4, /* bit 0: attention forward, bit 1: backward key-block pass -- the two waves of a SIMD run half a tile apart (default: see attention.hip) */
       PFN_TUNE_FUSE_LN_WIDE = 5,  /* 1: emsize 1024 runs the LayerNorm-fused GEMMs on 64-row x 1024-column tiles (gemm_nt_ln_wide / lnbwd_wide); 0 (default): the
                                    * 256 x 256 GEMM + LayerNorm kernels -- measured faster at that width */
       PFN_TUNE_GP_PLANES = 8,     /* 1 (default): the GP sampler's rank-256 trailing update reads pre-split fp16 planes (hi, lo on a power-of-two scale) by LDS-DMA; 0: it splits the f32 panel into three bf16 terms per tile (rounds 2-3) */
       PFN_TUNE_FUSE_DELTA = 9,    /* 1 (default): on the full-sequence layers of the bf16 stack the attention backward's delta = rowsum(dO . O) is taken in the epilogue of the GEMM that
                                    * produces dO (f32 atomics into a zeroed scratch: two addends per element at head dim 128); 0: a pass of its own over dO and O (attn_delta_kernel) */
       PFN_TUNE_GEMM_LN_ROWS = 7,  /* 1: the LayerNorm-fused GEMMs at emsize 512 run on 64-row tiles, two workgroups per CU (gemm.hip g_ln_rows64); 0 (default): 128-row tiles */
       PFN_TUNE_WGRAD_WAVES = 14,       /* waves per 256 x 256 tile of the grouped weight-gradient launch: 8 (128 x 64 each) or 4 (128 x 128 each, the whole register file per wave) */
       PFN_TUNE_LOSS_SCALE_TARGET = 15, /* PFN_PREC_FP16 backward: log2 of the value max|dlogits| is scaled to (power-of-two loss scale chosen on the device per call; default 2,
                                         * range -8 .. 12).  16 - target binades of headroom for what the chain adds; overflowing elements saturate at +-65504 */
       PFN_TUNE_RESIDUAL16 = 16,        /* 0: new descriptors carry PFN_SCHED_F32_RESIDUAL; 1 (default): they do not */
       PFN_TUNE_FUSE_Q_PROJECTION = 12, /* 1: new descriptors carry PFN_SCHED_FUSE_Q_PROJECTION (default 0) */
       PFN_TUNE_KEY_CENTERING = 13,     /* 1: new descriptors carry PFN_SCHED_KEY_CENTERING, 0: PFN_SCHED_NO_KEY_CENTERING, -1 (default): neither (centred with fp16, not with bf16) */
       PFN_TUNE_ATTN_CACHE_SPLITS = 17, /* > 0: at most that many key-range splits in the attention of pfn_stack_predict (1 = one pass over the keys, no merge); 0 (default): the
                                         * grid-size rule (csrc/attention.hip attn_cache_splits).  tools/bench_predict.py prices the split with it */
       PFN_TUNE_TOP_LAYER_TEST_ROWS = 6 /* 1 (default): the top encoder layer runs everything behind its K / V projection on the test rows only -- the reference
                                    * returns output[single_eval_pos:] (transformer.py:91), so that layer's train rows feed nothing; 0: every layer on every row */ };
int pfn_set_tuning(int key, int value);
/* TEST / PROFILING ONLY: in-step kernel timing.  pfn_profile_enable(1) makes the stack entry points (and pfn_op_attention_*) bracket every
 * launch of the kernel classes below with a pair of HIP events ON THE LAUNCH STREAM; pfn_profile_read(slot, &ms, &n) waits for the pairs
 * recorded for that class so far, returns their summed duration and count and forgets them.  bench.py uses it to report how long the
 * dominant kernel runs INSIDE the step (two micro-batch streams and the prior sampler share the chip), next to its duration on an idle chip.
 * Slots with +1 = the same kernel launched for the top encoder layer's test rows only. */
enum { PFN_PROF_ATTN_FWD = 0, PFN_PROF_ATTN_BWD_DELTA = 2, PFN_PROF_ATTN_BWD_KV = 4, PFN_PROF_ATTN_BWD_DQ = 6, PFN_PROF_GEMM_QKV = 8,
       PFN_PROF_GEMM_OUT_LN = 10, PFN_PROF_GEMM_LIN1 = 12, PFN_PROF_GEMM_LIN2_LN = 14, PFN_PROF_GEMM_DHPRE = 16, PFN_PROF_GEMM_DY1 = 18,
       PFN_PROF_GEMM_DCTX = 20, PFN_PROF_GEMM_DX = 22, PFN_PROF_WGRAD = 24, PFN_PROF_SLOTS = 26 };
int pfn_profile_enable(int on);
int pfn_profile_read(int slot, double* total_ms, int64_t* launches);

/* ---- parameter packing ------------------------------------------------------------------------
 * All parameters live in ONE flat f32 buffer (and one flat f32 gradient buffer) in state-dict
 * order: encoder.{weight,bias}, y_encoder.{weight,bias}, then per layer
 * self_attn.in_proj_{weight,bias}, self_attn.out_proj.{weight,bias}, linear1.{weight,bias},
 * linear2.{weight,bias}, norm1.{weight,bias}, norm2.{weight,bias}, then decoder.0.{weight,bias},
 * decoder.2.{weight,bias} (SURVEY.md 8(b) key list).  Each tensor starts at a multiple of 64
 * elements.  pfn_param_layout fills offsets[i] (elements) for tensor i; returns the tensor count
 * (4 + 12*nlayers + 4) or a negative error.  offsets may be NULL to query the count. */
int pfn_param_layout(const pfn_model_desc* d, int64_t* offsets, int64_t* numels, int max_tensors);
int64_t pfn_param_count(const pfn_model_desc* d);
/* operand-precision shadow of the weights (+ transposed copies for the data-gradient GEMMs) */
int64_t pfn_shadow_bytes(const pfn_model_desc* d);
int pfn_prepare_params(const pfn_model_desc* d, const float* params, void* shadow, void* stream);

/* ---- encoder stack: replaces TransformerModel.forward (transformer.py:55-91) -------------------
 * x: [T,B,F] f32 with element strides (x_st, x_sb, 1); y: [T,B] f32 with strides (y_st, y_sb).
 * sep = single_eval_pos, already normalised to [0,T].  Attention mask semantics of
 * generate_D_q_matrix (transformer.py:34-41): query i may attend key j iff j < sep or j == i.
 * logits: [(T-sep)*B, n_out] f32, row (t-sep)*B + b  (== output[single_eval_pos:] of the reference).
 * workspace: pfn_workspace_bytes() bytes; holds the activations pfn_stack_backward needs.
 * src_sbe: optional [T,B,E] f32 pre-embedded input (custom encoders / positional encodings run
 * in PyTorch); when non-NULL x/y are ignored and pfn_stack_backward returns d(src) in dsrc_sbe. */
int64_t pfn_workspace_bytes(const pfn_model_desc* d, int B, int S);
/* Rows the TOP encoder layer runs on behind its K / V projection for this call shape: (S - sep) * B when the stack drops that layer's train rows
 * (they feed nothing: the reference returns output[single_eval_pos:], transformer.py:91 -- the default; not with PFN_SCHED_TOP_LAYER_ALL_ROWS, not with live
 * dropout, not when sep < S / 4), else B * S.  Same results either way; bench.py counts FLOPs and launches with it. */
int64_t pfn_top_layer_rows(const pfn_model_desc* d, int B, int S, int sep, int use_dropout);
int pfn_stack_forward(const pfn_model_desc* d, const float* params, const void* shadow,
                      const float* x, int64_t x_st, int64_t x_sb,
                      const float* y, int64_t y_st, int64_t y_sb,
                      const float* src_sbe,
                      int B, int S, int sep,
                      void* workspace, int64_t workspace_bytes,
                      float* logits, void* stream);
/* The training forward with dropout (desc.dropout > 0).  Masks are counter-based functions of (dropout_seed, layer, site, element)
 * -- csrc/pfn_device.h `dropout_keep`; the backward regenerates them from the same seed, nothing is stored.  torch's own Philox
 * stream cannot be reproduced, so parity is against the oracle evaluating the SAME masks (oracle/pfn_oracle.py dropout_masks). */
int pfn_stack_forward_dropout(const pfn_model_desc* d, const float* params, const void* shadow,
                              const float* x, int64_t x_st, int64_t x_sb,
                              const float* y, int64_t y_st, int64_t y_sb,
                              const float* src_sbe,
                              int B, int S, int sep,
                              void* workspace, int64_t workspace_bytes,
                              float* logits, void* stream, uint64_t dropout_seed);
/* replaces loss.backward() through the model (train.py:93).  dlogits: [(T-sep)*B, n_out] f32.
 * grads: flat f32 buffer in pfn_param_layout order; gradients are ACCUMULATED into it
 * (train.py:92-97 sums micro-batch gradients). */
int pfn_stack_backward(const pfn_model_desc* d, const float* params, const void* shadow,
                       const float* x, int64_t x_st, int64_t x_sb,
                       const float* y, int64_t y_st, int64_t y_sb,
                       int B, int S, int sep,
                       void* workspace, int64_t workspace_bytes,
                       const float* dlogits, float* grads, float* dsrc_sbe, void* stream);
/* The same backward for data-parallel runs (no counterpart in the reference, which is single-process: train.py:29): the weight
 * gradients of the TOP `first_group_layers` encoder layers are launched as their own group as soon as the data-gradient chain has
 * passed those layers, and `on_first_group(user)` is called on the host right after that launch has been enqueued on `stream` --
 * every gradient of the parameters from layer (nlayers - first_group_layers) to the end of the flat buffer (those layers and the
 * decoder) is then complete in stream order, so the caller can record an event there and start the all-reduce of that part of the
 * buffer while the lower layers' backward still runs.  first_group_layers <= 0 or >= nlayers, or a NULL callback: exactly
 * pfn_stack_backward. */
typedef void (*pfn_host_callback)(void* user);
int pfn_stack_backward_split(const pfn_model_desc* d, const float* params, const void* shadow,
                             const float* x, int64_t x_st, int64_t x_sb,
                             const float* y, int64_t y_st, int64_t y_sb,
                             int B, int S, int sep,
                             void* workspace, int64_t workspace_bytes,
                             const float* dlogits, float* grads, float* dsrc_sbe, void* stream,
                             int first_group_layers, pfn_host_callback on_first_group, void* user,
                             int use_dropout, uint64_t dropout_seed);   /* use_dropout: the forward was pfn_stack_forward_dropout(dropout_seed) */

/* ---- RAGGED BATCH (ABI 7): the micro-batches of one optimizer step as ONE launch set.  The reference runs the k batches of an optimizer step one after the
 * other, each with its own single_eval_pos (train.py:66-97; the notebooks train at batch_size 4 x aggregate_k_gradients 25); a batch of 4 datasets fills a
 * fraction of the chip.  Here the datasets of several batches are stacked along B and every dataset carries its own eval position:
 *   sep_of  [B]     int32, device: eval position of dataset b (0 <= sep_of[b] <= S);  sep_min / sep_max = min / max over b (host values)
 *   row_off [B + 1] int64, device: first compact test row of dataset b; row_off[B] = test_rows = sum_b (S - sep_of[b])
 * Compact test rows (logits / dlogits [test_rows, n_out]) are DATASET-MAJOR: row_off[b] + (t - sep_of[b]) -- not the (t - sep) * B + b of the uniform entry
 * points (a micro-batch's rows are one contiguous slice [b][t]).  Fused embedding only (x / y given, no src_sbe); the top encoder layer runs on the test rows
 * only when every dataset leaves room for it (4 sep_min >= S), on every row otherwise.
 * Same workspace (pfn_workspace_bytes(d, B, S)); gradients are accumulated into `grads` as in pfn_stack_backward; first_group_layers / on_first_group as in
 * pfn_stack_backward_split.  The caller forms each micro-batch's loss from its slice, so the summed gradient equals the reference's sequential accumulation. */
int pfn_stack_forward_ragged(const pfn_model_desc* d, const float* params, const void* shadow,
                             const float* x, int64_t x_st, int64_t x_sb,
                             const float* y, int64_t y_st, int64_t y_sb,
                             int B, int S, const int32_t* sep_of, const int64_t* row_off, int sep_min, int sep_max, int64_t test_rows,
                             void* workspace, int64_t workspace_bytes, float* logits, void* stream,
                             int use_dropout, uint64_t dropout_seed);
int pfn_stack_backward_ragged(const pfn_model_desc* d, const float* params, const void* shadow,
                              const float* x, int64_t x_st, int64_t x_sb,
                              const float* y, int64_t y_st, int64_t y_sb,
                              int B, int S, const int32_t* sep_of, const int64_t* row_off, int sep_min, int sep_max, int64_t test_rows,
                              void* workspace, int64_t workspace_bytes,
                              const float* dlogits, float* grads, void* stream,
                              int first_group_layers, pfn_host_callback on_first_group, void* user,
                              int use_dropout, uint64_t dropout_seed);

/* ---- CONDITION ONCE, PREDICT MANY (ABI 9).  What a user does with a trained PFN: hold one training set fixed and ask for the posterior predictive at many test
 * points (reference presentation/heatmap_bardistribution.py, tabular.py, mcmc_svi_transformer_on_bayesian.py eval_transformer, BarDistribution.ei).  Under the mask
 * of generate_D_q_matrix (transformer.py:34-41) a train row attends to keys [0, sep) only and a test row to those plus itself, so the train rows' keys and values in
 * every layer do not depend on any test row, and test rows do not depend on each other.  pfn_stack_condition runs the train rows once and keeps every layer's
 * K | V in a CONTEXT buffer; pfn_stack_predict then runs any number of test rows against it, in as many calls and chunks as the caller likes:
 *   pfn_stack_predict(context of (x_train, y_train), x_test)  ==  pfn_stack_forward(cat(x_train, x_test), cat(y_train, anything), sep)  row for row
 * up to rounding order (no dropout: the inference pass).  Fused embedding only (x / y given; positional encodings and SeqBN tie a row's value to the sequence).
 *   x, y (condition): [sep, B, F] / [sep, B] f32 with element strides (x_st, x_sb, 1) / (y_st, y_sb); sep >= 0.  x (predict): [n, B, F] with strides (x_st, x_sb, 1).
 *   CONTEXT: pfn_context_bytes(d, B, sep) bytes, per layer [B, sep, 2E] K | V rows in operand precision (K centred when the descriptor centres keys,
 *     PFN_SCHED_NO_KEY_CENTERING) followed, when it does, by the [B, E] f32 key shift of that layer; every block 256-byte aligned.  sep = 0: 0 bytes, context may
 *     be NULL (each test row attends only to itself).  The context belongs to the descriptor, the parameters and the B, F, sep it was made with: a caller
 *     that changes any of them conditions again.
 *   workspace (condition): pfn_workspace_bytes(d, B, sep) -- the train rows' forward; free again when the call has run.
 *   workspace (predict): pfn_predict_workspace_bytes(d, B, n): the test rows of one layer at a time -- independent of nlayers and sep.
 *   logits (predict): [n * B, n_out] f32, row t * B + b (the forward's (t - sep) * B + b with t counted from the first test row); n_out == 0 (custom decoder):
 *     [n * B, emsize] f32, the encoder's test rows.
 * Wrong sizes, a NULL context with sep > 0, or a context smaller than pfn_context_bytes return PFN_ERR_ARGUMENT before anything is launched. */
int64_t pfn_context_bytes(const pfn_model_desc* d, int B, int sep);
int pfn_stack_condition(const pfn_model_desc* d, const float* params, const void* shadow,
                        const float* x, int64_t x_st, int64_t x_sb,
                        const float* y, int64_t y_st, int64_t y_sb,
                        int B, int sep,
                        void* workspace, int64_t workspace_bytes,
                        void* context, int64_t context_bytes, void* stream);
int64_t pfn_predict_workspace_bytes(const pfn_model_desc* d, int B, int n);
int pfn_stack_predict(const pfn_model_desc* d, const float* params, const void* shadow,
                      const void* context, int64_t context_bytes, int sep,
                      const float* x, int64_t x_st, int64_t x_sb,
                      int B, int n,
                      void* workspace, int64_t workspace_bytes, float* logits, void* stream);

/* ---- INPUT GRADIENTS (ABI 10): d(output)/d(x) for Bayesian optimisation (reference acquisition_functions.py; botorch's optimize_acqf climbs grad_x of the
 * acquisition value) and for sensitivity analyses.
 * Predict: pfn_stack_predict_saved is pfn_stack_predict (same arguments, same kernels and fusion decisions, bit-identical logits) on a workspace of
 *   pfn_predict_grad_workspace_bytes(d, B, n) bytes that keeps every layer's test-row activations (q|k|v, ctx, lse, the pre-LayerNorm sums and their statistics,
 *   the GELU derivatives, the layer outputs) plus the backward's scratch: linear in nlayers, independent of sep.  pfn_stack_predict_backward then turns
 *   dlogits [n * B, n_out] (row t * B + b; [n * B, emsize] when n_out == 0) into dx = d(x_test) [n, B, F] f32 with element strides (dx_st, dx_sb, 1).  The train
 *   rows behind the context are constants: no gradient reaches the context or any parameter, and no parameter gradient is written.  fp16 descriptors run the
 *   chain under the training backward's loss scale (from max |dlogits|); dx leaves unscaled.  The workspace must be the one the saved predict call wrote, for
 *   the same descriptor, parameters, context, sep, B and n.
 * Full forward: pfn_stack_input_grads, after pfn_stack_backward / pfn_stack_backward_split on the same workspace (fused embedding, not ragged): dx [S, B, F] for
 *   every row and, when dy is not NULL, dy [S, B] for the train rows -- rows t >= sep of dy are 0 (the reference reads y[:sep] only, transformer.py:73).
 * Wrong sizes, NULL pointers, or a context smaller than pfn_context_bytes return PFN_ERR_ARGUMENT before anything is launched. */
int64_t pfn_predict_grad_workspace_bytes(const pfn_model_desc* d, int B, int n);
int pfn_stack_predict_saved(const pfn_model_desc* d, const float* params, const void* shadow,
                            const void* context, int64_t context_bytes, int sep,
                            const float* x, int64_t x_st, int64_t x_sb,
                            int B, int n,
                            void* workspace, int64_t workspace_bytes, float* logits, void* stream);
int pfn_stack_predict_backward(const pfn_model_desc* d, const float* params, const void* shadow,
                               const void* context, int64_t context_bytes, int sep, int B, int n,
                               void* workspace, int64_t workspace_bytes, const float* dlogits,
                               float* dx, int64_t dx_st, int64_t dx_sb, void* stream);
int pfn_stack_input_grads(const pfn_model_desc* d, const float* params, int B, int S, int sep,
                          const void* workspace, int64_t workspace_bytes,
                          float* dx, int64_t dx_st, int64_t dx_sb, float* dy, int64_t dy_st, int64_t dy_sb, void* stream);

/* ---- CONDITION AND PREDICT WITH A DIFFERENT TRAINING-SET SIZE PER DATASET (ABI 10, additive: a binding detects these four by symbol).  Tabular tasks of different
 * sizes, Bayesian-optimisation runs at different iteration counts, or one dataset at many train sizes (a learning curve) as ONE batch.  The four calls mirror
 * pfn_stack_condition / pfn_stack_predict / pfn_stack_predict_saved / pfn_stack_predict_backward with `sep` replaced by sep_max and sep_of:
 *   sep_of: [B] int32 in DEVICE memory, dataset b's train-row count len_b; sep_max >= every len_b is the row count of the padded x / y arrays of the condition call
 *     and the context's rows per dataset.
 *   SEMANTICS: for every dataset b, row t of column b of the ragged predict equals
 *       pfn_stack_forward(cat(x_b[:len_b], x_test_b), cat(y_b[:len_b], anything), sep = len_b)   run alone on that dataset, up to rounding order.
 *   PADDING RULE: rows t >= len_b of the padded x / y (any finite values) reach NO output, not even at rounding level.  Padding with real rows would not do: a padded
 *     train row is a key every query sees.  The condition pass treats these rows as test rows of the ragged forward (embedded without y, attending to [0, len_b)
 *     plus themselves, outside the key-shift sample); their K | V land in the context and are never read.  It runs B * sep_max rows.
 *   len_b = 0 is allowed inside a batch with sep_max > 0: that dataset's test rows attend to themselves only (zero key shift).
 *   CLAMPING: the values behind sep_of cannot be checked on the host without a synchronise.  Every kernel that reads them clamps them to [0, sep_max] (the condition
 *     pass works on a clamped copy), so no value can carry a read outside the context; a value outside the range gives the clamped dataset's result.
 *   CONTEXT and WORKSPACES keep the uniform sizes and layout at sep_max: pfn_context_bytes(d, B, sep_max) (dataset stride sep_max rows; the per-layer [B, E] key shift
 *     where keys are centred), pfn_workspace_bytes(d, B, sep_max), pfn_predict_workspace_bytes / pfn_predict_grad_workspace_bytes(d, B, n).  A context made by
 *     pfn_stack_condition_ragged is read with the SAME sep_max and sep_of.  With every len_b == sep_max the calls run the uniform calls' arithmetic bit for bit.
 *   The attention's key-range splits (one launch geometry per call) are sized for sep_max; a split beyond a dataset's last key does no work.
 * NULL sep_of, B < 1, sep_max < 0, n < 0, a NULL context with sep_max > 0, a context or workspace that is too small return PFN_ERR_ARGUMENT before anything is
 * launched.  sep_max == 0: nothing to condition, as pfn_stack_condition at sep = 0. */
int pfn_stack_condition_ragged(const pfn_model_desc* d, const float* params, const void* shadow,
                               const float* x, int64_t x_st, int64_t x_sb,
                               const float* y, int64_t y_st, int64_t y_sb,
                               int B, int sep_max, const int32_t* sep_of,
                               void* workspace, int64_t workspace_bytes,
                               void* context, int64_t context_bytes, void* stream);
int pfn_stack_predict_ragged(const pfn_model_desc* d, const float* params, const void* shadow,
                             const void* context, int64_t context_bytes, int sep_max, const int32_t* sep_of,
                             const float* x, int64_t x_st, int64_t x_sb,
                             int B, int n,
                             void* workspace, int64_t workspace_bytes, float* logits, void* stream);
int pfn_stack_predict_saved_ragged(const pfn_model_desc* d, const float* params, const void* shadow,
                                   const void* context, int64_t context_bytes, int sep_max, const int32_t* sep_of,
                                   const float* x, int64_t x_st, int64_t x_sb,
                                   int B, int n,
                                   void* workspace, int64_t workspace_bytes, float* logits, void* stream);
int pfn_stack_predict_backward_ragged(const pfn_model_desc* d, const float* params, const void* shadow,
                                      const void* context, int64_t context_bytes, int sep_max, const int32_t* sep_of, int B, int n,
                                      void* workspace, int64_t workspace_bytes, const float* dlogits,
                                      float* dx, int64_t dx_st, int64_t dx_sb, void* stream);

/* ---- bar distribution: replaces BarDistribution / FullSupportBarDistribution.forward and .mean
 * (bar_distribution.py:19-38, 83-117).  logits [R, nbars] f32 (row stride ld), y [R], borders
 * [nbars+1] sorted.  nll [R].  lse [R] and bucket [R] are saved for the backward. */
int pfn_bar_nll_forward(const float* logits, int64_t ld, const float* y, const float* borders,
                        int64_t R, int nbars, int full_support,
                        float* nll, float* lse, int32_t* bucket, void* stream);
/* dlogits[r,:] = gout[r] * (softmax(logits[r,:]) - onehot(bucket[r])) */
int pfn_bar_nll_backward(const float* logits, int64_t ld, const float* lse, const int32_t* bucket,
                         const float* gout, int64_t R, int nbars, float* dlogits, void* stream);
int pfn_bar_mean(const float* logits, int64_t ld, const float* borders, int64_t R, int nbars,
                 int full_support, float* mean, void* stream);
/* its gradient (ABI 10): dlogits[r, j] = gout[r] * p_j * (c_j - mean[r]), c_j the bucket means pfn_bar_mean uses, mean[r] what it returned; row stride ld */
int pfn_bar_mean_backward(const float* logits, int64_t ld, const float* borders, int64_t R, int nbars, int full_support,
                          const float* mean, const float* gout, float* dlogits, void* stream);

/* ---- posterior summaries and draws (ABI 10, additive: a binding detects them by symbol).  pfn_bar_stats generalises
 * BarDistribution.quantile / mode / ei (bar_distribution.py:40-80) and adds variance, CDF and an inverse CDF at any level; one pass
 * over each logits row computes K <= PFN_BAR_STATS_MAX of them, no [R, nbars] intermediate.  The definitions (conditional bucket CDF
 * with the half-normal tails of the full-support class, variance, gradients) are in the header of this section of csrc/bar.hip.
 *   kinds: HOST array of K PFN_BAR_STAT_* values.
 *   args: DEVICE, one float per statistic -- y for CDF, the level u for ICDF, best_f for EI_MAX / EI_MIN, ignored for MEAN / VARIANCE / MODE.
 *     arg_ld == 0: K values shared by all rows; otherwise [R, arg_ld] with arg_ld >= K (a best_f per dataset, a target per row).
 *   MODE (bar_distribution.py:64-67): midpoint of the bucket with the largest logit, lowest index on ties, plain midpoint in the tails; zero gradient.
 *   EI_MAX / EI_MIN (bar_distribution.py:69-80): the reference formula for both classes -- the outer buckets count as [b_0, b_1] and [b_{n-1}, b_n].
 *   ICDF (generalises bar_distribution.py:40-62): linear inside a bucket, the half-normal tails inverted for full support; u <= 0 gives b_0 / -inf, u >= 1 b_n / +inf.
 *   out [R, K] f32.  The arguments are not differentiated.
 * pfn_bar_stats_backward: dlogits[r, :] (row stride ld) = sum_k gout[r, k] d out[r, k] / d logits[r, :], one read of the row and one write; `out` is what
 *   the forward returned for the same arguments.
 * pfn_bar_sample: out[s, r] = ICDF_r(u(seed, r, s)), s < n_samples, with
 *     a = mix32(lo32(seed) ^ lo32(r) * 0x9E3779B1), b = mix32(a ^ hi32(seed) ^ hi32(r) * 0x85EBCA77), h = mix32(b ^ s * 0xC2B2AE35), u = ((h >> 9) + 0.5) * 2^-23
 *   (mix32: h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16; products modulo 2^32): a function of (seed, row, draw) only,
 *   bit-identical to the ICDF statistic at the same u.  No cap on nbars.
 * PFN_ERR_ARGUMENT before anything is launched: NULL pointers, K outside 1 .. 16, an unknown kind, nbars < 1 (< 2 with full_support), ld < nbars,
 *   0 < arg_ld < K, R < 0, n_samples < 0.  R == 0 or n_samples == 0: PFN_OK, nothing launched. */
#define PFN_BAR_STATS_MAX 16
#define PFN_BAR_STAT_MEAN 0
#define PFN_BAR_STAT_VARIANCE 1
#define PFN_BAR_STAT_MODE 2
#define PFN_BAR_STAT_CDF 3
#define PFN_BAR_STAT_ICDF 4
#define PFN_BAR_STAT_EI_MAX 5
#define PFN_BAR_STAT_EI_MIN 6
int pfn_bar_stats(const float* logits, int64_t ld, const float* borders, int64_t R, int nbars, int full_support,
                  const int32_t* kinds, int K, const float* args, int64_t arg_ld, float* out, void* stream);
int pfn_bar_stats_backward(const float* logits, int64_t ld, const float* borders, int64_t R, int nbars, int full_support,
                           const int32_t* kinds, int K, const float* args, int64_t arg_ld, const float* out, const float* gout,
                           float* dlogits, void* stream);
int pfn_bar_sample(const float* logits, int64_t ld, const float* borders, int64_t R, int nbars, int full_support,
                   int n_samples, uint64_t seed, float* out, void* stream);

/* ---- optimizer: replaces clip_grad_norm_(params, 1.) + Adam.step() + zero_grad()
 * (train.py:55,95-97).  One fused pass over the flat buffers; the clip coefficient is computed on
 * the device (no host sync).  grad_scale multiplies g first (1/world for DP averaging).
 * scratch: >= 8192 bytes, zeroed once by the caller; scratch[0] (f32) receives the global gradient norm before clipping.
 * A non-finite norm (inf / NaN anywhere in g) SKIPS the step: params and moments are left as they are, g is still cleared when zero_grad != 0, and
 * scratch[1025] (f32) counts the skipped steps -- GradScaler's found_inf behaviour; the reference's loop would write NaN into every parameter.
 * zero_grad != 0 clears g after the update. */
int pfn_clip_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                       float lr, float beta1, float beta2, float eps, float max_norm,
                       float grad_scale, int step, int zero_grad, float* scratch, void* stream);

/* ---- GP prior sampler: replaces priors.fast_gp.get_batch (priors/fast_gp.py:35-58) and the
 * sampling half of priors.fast_gp_mix.get_batch (priors/fast_gp_mix.py:85-99).
 * y_b ~ N(0, outputscale_b * k(x_b, x_b; lengthscale_b) + noise_b * I) by Gram -> Cholesky -> L z.
 * x [B,S,nf] f32: filled with U[0,1) from the counter-based generator when gen_x != 0, else input.
 * z [B,S] f32 base normals: generated when gen_z != 0 (and written back), else input.
 * lengthscale [B,nf], outputscale [B], noise [B].  kernel: 0 = RBF, 1 / 2 / 3 = Matern nu = 2.5 / 1.5 / 0.5 (gpytorch MaternKernel's three closed forms).
 * K_ws: workspace of pfn_gp_workspace_bytes(B, S) bytes: the [B,S,S] f32 matrix, factored in place (SCRATCH: with the plane scratch attached only the
 * 256 x 256 diagonal blocks of the factor are left in it -- the panels below them are consumed from the planes and never stored), followed by the scratch of
 * the trailing update (TWO sets -- the solved panels of an even and an odd outer block, the delayed rank-512 update -- of two scaled fp16 planes each: + 23 % at S = 2000, + 39 % at 1000, + 50 % at 512; always size with pfn_gp_workspace_bytes).  K_ws_bytes (ABI 7): the size the caller allocated --
 * below B*S*S*4 the call returns PFN_ERR_ARGUMENT; between that and pfn_gp_workspace_bytes(B, S) the trailing update runs without the plane scratch
 * (same arithmetic, slower), so a caller sized for an older ABI cannot be written past.  info [B]: 0 or (index+1) of the first non-positive pivot. */
int64_t pfn_gp_workspace_bytes(int B, int S);
int pfn_gp_prior_sample(float* x, float* z, float* y, float* K_ws, int64_t K_ws_bytes,
                        const float* lengthscale, const float* outputscale, const float* noise,
                        int B, int S, int nf, int kernel, int gen_x, int gen_z,
                        uint64_t seed, uint64_t offset, int32_t* info, void* stream);

/* ---- Exact-GP sequential predictions: replaces priors.fast_gp.evaluate (priors/fast_gp.py:88-120), which refits a
 * gpytorch ExactGP on points 0..t-1 and predicts point t for every t (one Cholesky per t).  Here ONE factorisation of
 * the full covariance gives all of them (gp_prior.hip): for every dataset b and position t, the posterior at x[b,t]
 * given (x[b,:t], y[b,:t]) under the GP with the given hyper-parameters:
 *   mean[b,t], var[b,t] (predictive, observation noise included), nll[b,t] = -log N(y[b,t]; mean, var).
 * Position 0 is the prior.  x [B,S,nf], y [B,S]; K_ws / K_ws_bytes as in pfn_gp_prior_sample; resid_ws / w_ws [B,S] scratch; nll / mean / var may be
 * null.  S % 4 == 0.  info as in pfn_gp_prior_sample. */
int pfn_gp_posterior(const float* x, const float* y, float* K_ws, int64_t K_ws_bytes, float* resid_ws, float* w_ws,
                     const float* lengthscale, const float* outputscale, const float* noise,
                     int B, int S, int nf, int kernel, float* nll, float* mean, float* var,
                     int32_t* info, void* stream);

/* ---- GP hyper-parameter fit (ABI 10, additive: a binding detects these three by symbol): the MAP-II baseline of the mixture-of-GPs prior, reference
 * priors/fast_gp_mix.py:156-169 (`get_fitted_model`: botorch fit_gpytorch_model on gpytorch's ExactMarginalLogLikelihood).  Problem p uses the first
 * n = n_of[p] rows of x[p] [S,nf] and y[p] [S]; its parameters are theta[p] [nf+3] = (log lengthscale_d, log outputscale, log(noise - noise_floor), constant
 * mean c) and the objective is
 *   J = -(1/n) [ log N(y_:n; c 1, K) + sum_d lg(l_d; a_l, b_l) + lg(os; a_o, b_o) + lg(noise; a_n, b_n) ],   K = os k(x, x; l) + noise I,
 *   lg(v; a, b) = a log b - lgamma(a) + (a - 1) log v - b v         (Gamma log densities on the natural values, no Jacobian term, as gpytorch),
 * prior [8] = (a_l, b_l, a_o, b_o, a_n, b_n, noise_floor, 0) on the device.  kernel as in pfn_gp_prior_sample.
 * pfn_gp_mll_grad: value [P] = J, grad [P,nf+3] = dJ/dtheta (null: value only).  flags bit 0: c is held fixed, grad[c] = 0.  A non-positive pivot gives
 *   info[p] = pivot + 1, value[p] = +inf, grad[p,:] = 0; the other problems are unaffected.  The result for problem p is a deterministic function of
 *   (x[p], y[p], n_of[p], theta[p]): no atomics, independent of P and of the other problems of the call.
 * pfn_gp_fit_predict: factorises by itself; for every test point x_test[p,j] the posterior under theta[p]: mean = c + (L^-1 k*) . (L^-1 (y - c)),
 *   var = os + noise - |L^-1 k*|^2 (observation noise included).
 * Both: caller-owned buffers, stream-ordered, no allocation, no device synchronisation.  S % 4 == 0, nf <= 126, P <= 65535.  n_of null = all S rows, else
 * read on the device and clamped to [1, S]; rows >= n_of[p] of x / y are never read.  ws: pfn_gp_fit_workspace_bytes(P, S) bytes (two [P,Sp,Sp] f32
 * matrices, Sp = S rounded up to 64: the factor / K^-1 and L^-1, plus vectors and per-tile partial sums); smaller returns PFN_ERR_ARGUMENT.  info [P] is
 * written by the call (0 = ok). */
int64_t pfn_gp_fit_workspace_bytes(int P, int S);
int pfn_gp_mll_grad(const float* x, const float* y, const int32_t* n_of, const float* theta, const float* prior,
                    int P, int S, int nf, int kernel, int flags, void* ws, int64_t ws_bytes,
                    float* value, float* grad, int32_t* info, void* stream);
int pfn_gp_fit_predict(const float* x, const float* y, const int32_t* n_of, const float* theta, const float* prior,
                       int P, int S, int nf, int kernel, const float* x_test, int m, void* ws, int64_t ws_bytes,
                       float* mean, float* var, int32_t* info, void* stream);

/* ---- batched NUTS (ABI 10, additive; csrc/gp_mcmc.hip): the No-U-Turn sampler as a state machine that advances C independent chains by exactly ONE
 * evaluation of the potential per call.  The caller owns the target: it evaluates value [C] and grad [C, ld] at trial [C, ld] (e.g. with pfn_gp_mll_grad) and
 * calls advance, which finishes the pending leapfrog of every chain, does the leaf's bookkeeping (multinomial NUTS, iterative tree with per-leaf progressive
 * sampling inside a subtree and biased progressive sampling between subtrees, diagonal mass, divergence at an energy error above 1000), ends / begins
 * transitions as needed and writes the next trial point.  The potential is U_c = scale[c] value[c] - sum_k shift[k] theta_ck with gradient scale[c] grad - shift
 * (scale [C], shift [D] nullable: 1 and 0); only columns < D of the rows of trial / grad (row stride ld >= D) are ever touched.  A non-finite value, or
 * info[c] != 0 (info nullable), makes the leaf divergent.  1 <= D <= 128, 1 <= max_tree_depth <= 10, num_samples >= 1, num_warmup >= 0; else PFN_ERR_ARGUMENT.
 *   init: lays out the workspace, copies theta0 [C, ld] to trial (the first advance consumes the potential AT the start point), zeroes *done_count.
 *         chain_ids [C] int64 (NULL: 0 .. C-1) select the chain's Philox stream: chain c's whole history is a function of (seed, chain_ids[c], its own inputs).
 *         inv_mass0 [C, D] (NULL: ones).  window_ends: HOST array of n_windows <= PFN_NUTS_MAX_WINDOWS increasing transition counts at which a slow
 *         (mass) adaptation window ends, the first window starting at transition window_start; every end lies below num_warmup (dual averaging restarts
 *         at a window end); used with PFN_NUTS_ADAPT_MASS.  During the num_warmup
 *         transitions the step size follows dual averaging (gamma .05, t0 10, kappa .75, mu = log(10 step_size)) towards target_accept; afterwards it is
 *         the averaged one.
 *   advance: outputs per finished transition t of chain c: stats [C, W+N, 8] = (step size used, mean accept probability, tree depth, leapfrogs, diverging,
 *         potential of the kept point, 0, 0); the kept point into samples [C, N, D] (t >= W) or, with PFN_NUTS_KEEP_WARMUP and warm != NULL, warm [C, W, D].
 *         A chain that has finished W+N transitions adds 1 to *done_count, rests at its last sample in trial and is never written again.
 *         W = num_warmup and N = num_samples size these buffers and must be the values given to init.  The kernel compares (C, D, max_tree_depth, W, N)
 *         with what init recorded in the workspace; on a mismatch it touches NOTHING -- no output, no trial point, no done_count -- while the call, which
 *         cannot read device memory without synchronising, still returns PFN_OK: a caller that passes other sizes than it initialised sees no progress.
 * Workspace: pfn_nuts_workspace_bytes(C, D, max_tree_depth) bytes (negative on bad arguments); the current inverse mass [C, D] f32 sits at byte offset
 * PFN_NUTS_INV_MASS_OFFSET.  Stream-ordered; nothing is allocated and nothing synchronises. */
#define PFN_NUTS_ADAPT_MASS 1
#define PFN_NUTS_KEEP_WARMUP 2
#define PFN_NUTS_MAX_WINDOWS 16
#define PFN_NUTS_INV_MASS_OFFSET 256
int64_t pfn_nuts_workspace_bytes(int C, int D, int max_tree_depth);
int pfn_nuts_init(void* ws, int64_t ws_bytes, int C, int D, int64_t ld, int max_tree_depth, int num_warmup, int num_samples, int flags,
                  const int32_t* window_ends, int n_windows, int window_start, float step_size, float target_accept, uint64_t seed,
                  const int64_t* chain_ids, const float* theta0, const float* inv_mass0, float* trial, int32_t* done_count, void* stream);
int pfn_nuts_advance(void* ws, int64_t ws_bytes, int C, int D, int64_t ld, int max_tree_depth, int num_warmup, int num_samples,
                     const float* value, const float* grad, const int32_t* info, const float* scale, const float* shift, float* trial,
                     float* samples, float* stats, float* warm, int32_t* done_count, void* stream);

/* ---- BNN posterior target (ABI 10, additive; csrc/bnn_mcmc.hip): the potential of the two-layer Bayesian neural network of the reference's BNN study
 * (mcmc_svi_transformer_on_bayesian.py:28-67, `BayesianModel`) and its gradient for C = P K chains in one launch -- the `fun` of pfn_nuts_advance's caller --
 * and the chains' class-1 probabilities at test points.  Model: h = W1 x + b1, a = act(h), o = W2 a + b2; activation 0 = identity (the reference's
 * nn.Sequential(fc1, fc2) has no non-linearity), 1 = tanh; every weight and bias ~ N(0, 1); y_i ~ Categorical(softmax(o_i)).  A chain's parameters are
 * theta = (W1 [H,F] row-major, b1 [H], W2 [2,H], b2 [2]), D = H (F + 3) + 2 numbers in a row of stride ld >= D; chain c belongs to problem c / K.
 * pfn_bnn_logp_grad: x [P,S,F], y [P,S] f32 (class = y > 0.5); problem p uses its first n = clamp(n_of[p], 0, S) rows (n_of [P] int32 on the device; NULL:
 *   all S; n = 0 gives the prior), rows >= n are never read.  value [C] = |theta|^2 / 2 + (D / 2) log 2 pi - sum_{i<n} log softmax(o_i)[y_i], the potential
 *   itself (pfn_nuts_advance takes it with scale = NULL); grad [C, ld] receives its gradient in the first D columns, columns >= D are never written; grad
 *   NULL: value only.  The log-softmax is softplus of the signed logit difference: logits of any finite size give finite values.  A non-finite theta gives a
 *   non-finite value (a divergent leaf for pfn_nuts_advance).
 * pfn_bnn_predict: x_test [P,m,F], theta [C, ld] -> prob1 [C, m] = softmax(o)[1].  m = 0 returns at once.
 * Both: caller-owned buffers, stream-ordered, no allocation, no device synchronisation, no atomics; the result for chain c is a deterministic function of
 * its own problem's data and its own theta, bit for bit -- independent of P, K and of the chain's position in the call.  1 <= F <= 16, 1 <= H <= 64 and
 * activation in {0, 1}, else PFN_ERR_UNSUPPORTED; P >= 1, K >= 1, S >= 1, m >= 0, ld >= D and non-NULL buffers, else PFN_ERR_ARGUMENT; the shapes are
 * checked first, before any pointer is looked at and before any HIP call. */
int pfn_bnn_logp_grad(const float* x, const float* y, const int32_t* n_of, const float* theta, int64_t ld,
                      int P, int K, int S, int F, int H, int activation,
                      float* value, float* grad, void* stream);
int pfn_bnn_predict(const float* x_test, const float* theta, int64_t ld, int P, int K, int m, int F, int H, int activation,
                    float* prob1, void* stream);

/* ---- SVI on the BNN (ABI 10, additive; csrc/bnn_svi.hip): the mean-field Gaussian guide of the reference's `eval_svi` (mcmc_svi_transformer_on_bayesian.py:211-246:
 * pyro's AutoDiagonalNormal + Trace_ELBO(num_particles) + Adam) for P problems, num_steps steps in ONE launch, one block per problem.
 * Guide: q(theta) = N(loc, diag(scale^2)), scale = softplus(u); theta_k = loc + scale eps_k for particles k < K = num_particles.  Per step
 *   L = mean_k [ U(theta_k) - sum_i (log scale_i + eps_ki^2 / 2) - (D / 2) log 2 pi ]      (what pyro's svi.step returns; U: the potential of pfn_bnn_logp_grad,
 *   prior included, same theta layout, activation and n_of), g_loc = mean_k grad U(theta_k), g_scale = mean_k grad U(theta_k) * eps_k - 1 / scale,
 *   g_u = g_scale sigmoid(u), then torch.optim.Adam without weight decay on loc and u: m <- beta1 m + (1 - beta1) g, v <- beta2 v + (1 - beta2) g^2,
 *   p <- p - lr (m / (1 - beta1^t)) / (sqrt(v / (1 - beta2^t)) + eps), t = absolute step index + 1 (beta^t in f64).
 * state [P, 6, ld] f32, ld >= D, caller-owned: rows loc, u, m_loc, v_loc, m_u, v_u; columns >= D are never read or written.  The launch runs steps
 *   step0 .. step0 + num_steps - 1; loss [P, num_steps] (or NULL) receives L of every step, evaluated before the step's update.
 * Noise: eps of (problem id q, absolute step t, particle k, coordinate i) is component i & 3 of normal4(philox4x32_10(idx = ((t K + k) << 10) | (i >> 2),
 *   stream = q, key = seed)) (Box-Muller on the block's four words); q = problem_ids[p] (int64 [P] on the device), or p when NULL.  It depends on
 *   (seed, q, t, k, i) alone -- not on P, on the block shape or on how the steps are split over launches.
 * A problem's result is a bitwise function of its own rows, state, q, seed and (H, F, K): the same alone and in a batch, and steps(0, a + b) equals
 *   steps(0, a) followed by steps(a, b).  Rows >= n of x / y are never read.  A problem whose state is or becomes non-finite stays alone in that.
 * Stream-ordered, no allocation, no host synchronisation, no atomics.  1 <= F <= 16, 1 <= H <= 64, activation in {0, 1}, else PFN_ERR_UNSUPPORTED;
 *   P >= 1, S >= 1, num_particles >= 1, 0 <= step0 <= 2^40, num_steps >= 0, (step0 + num_steps + 1) num_particles < 2^53, ld >= D, lr >= 0, beta1 / beta2 in [0, 1),
 *   eps >= 0 and non-NULL x, y, state, else PFN_ERR_ARGUMENT; the shapes are checked first, before any pointer is looked at and before any HIP call.
 *   num_steps = 0 returns at once. */
int pfn_bnn_svi_steps(const float* x, const float* y, const int32_t* n_of, float* state, int64_t ld, int P, int S, int F, int H, int activation,
                      int num_particles, int64_t step0, int num_steps, float lr, float beta1, float beta2, float eps, uint64_t seed,
                      const int64_t* problem_ids, float* loss, void* stream);

/* ---- SVGD on the BNN (ABI 10, additive; csrc/bnn_svgd.hip): Stein variational gradient descent, the reference's `eval_svi(..., svgd=True)`
 * (mcmc_svi_transformer_on_bayesian.py:211-246: pyro's SVGD(model, RBFSteinKernel(), adam, num_particles)) for P problems, num_steps steps in ONE launch, one
 * block per problem.  N = num_particles points x_n in R^D per problem; U is the potential of pfn_bnn_logp_grad (prior included, same theta layout,
 * activation and n_of).  One step:
 *   g_n = grad U(x_n);
 *   h_d = bandwidth_factor * median_{i<j} (x_id - x_jd)^2 / log(N + 1) per coordinate d (RBFSteinKernel, "univariate"): torch.median's median of the
 *     N (N - 1) / 2 pairs, the lower of the two middle values when their count is even -- exactly one of the pairwise values, the f32 square of the selected
 *     k-th smallest f32 |x_id - x_jd|; h is a constant of the step; h_d = 0 (coincident particles) makes that problem non-finite, as the formula does;
 *   k_d(n,m) = exp(-(x_nd - x_md)^2 / h_d),  s_nd = (1/N) sum_m [ k_d(n,m) g_md + k_d(n,m) 2 (x_md - x_nd) / h_d ]  (summed over m in index order);
 *   torch.optim.Adam without weight decay on every x_nd with gradient s_nd: m <- beta1 m + (1 - beta1) s, v <- beta2 v + (1 - beta2) s^2,
 *     x <- x - lr (m / (1 - beta1^t)) / (sqrt(v / (1 - beta2^t)) + eps), t = absolute step index + 1 (beta^t in f64).  No randomness inside a step.
 * state [P, 3, N, ld] f32, ld >= D, caller-owned: N rows of particles, N rows of m, N rows of v per problem; updated in place; columns >= D are never read
 *   or written.  The launch runs steps step0 .. step0 + num_steps - 1.  potential [P, num_steps] (or NULL): the mean over particles of U(x_n) before the
 *   step's update.  bandwidth [P, ld] (or NULL): h of the last step run, first D columns.
 * workspace: pfn_bnn_svgd_workspace_bytes(P, num_particles, F, H) bytes (negative on bad arguments; 0 when particles, gradients and moments stay in LDS
 *   for the whole launch, and workspace may then be NULL); otherwise it carries the particles' gradients between the phases of a step.
 * A problem's result is a bitwise function of its own rows, its own state and (H, F, N): the same alone and in a batch, and steps(0, a + b) equals
 *   steps(0, a) followed by steps(a, b).  Rows >= n of x / y are never read.  A problem whose state is or becomes non-finite stays alone in that.
 * Stream-ordered, no allocation, no host synchronisation, no atomics.  1 <= F <= 16, 1 <= H <= 64, activation in {0, 1} and
 *   2 <= num_particles <= PFN_BNN_SVGD_MAX_PARTICLES, else PFN_ERR_UNSUPPORTED; P >= 1, S >= 1, step0 >= 0, num_steps >= 0, ld >= D, lr >= 0 and finite,
 *   beta1 / beta2 in [0, 1), eps >= 0, bandwidth_factor > 0, non-NULL x, y, state and a workspace of at least the stated bytes, else PFN_ERR_ARGUMENT; the
 *   limits are checked first, before any pointer is looked at and before any HIP call.  num_steps = 0 returns at once. */
#define PFN_BNN_SVGD_MAX_PARTICLES 64
int64_t pfn_bnn_svgd_workspace_bytes(int P, int num_particles, int F, int H);
int pfn_bnn_svgd_steps(const float* x, const float* y, const int32_t* n_of, float* state, int64_t ld, int P, int S, int F, int H, int activation,
                       int num_particles, int64_t step0, int num_steps, float lr, float beta1, float beta2, float eps, float bandwidth_factor,
                       void* workspace, int64_t workspace_bytes, float* potential, float* bandwidth, void* stream);

/* ---- Tabular study (ABI 10, additive; csrc/tabular.hip): the evaluation protocol of the reference's tabular.py:160-370 on the device.  f32 data, int32
 * indices, caller-owned buffers, stream-ordered, no allocation, no workspace, no host synchronisation; every result is a bitwise function of its own
 * window / column / problem, wherever it sits in the call.  The shapes are checked first, before any pointer is looked at and before any HIP call.
 *
 * pfn_tabular_windows: X [N,F] the table, y [N], starts [W] int32 ON THE DEVICE (the first row of each window; a window with start < 0 or start + bptt > N
 *   is never read and comes out as NaN), T = bptt - sep.
 *   mode PFN_TAB_NORM_WITH_TEST (evaluate_position:288-296, the PFN arm): x_out [sep+1, W T, F_out], y_out [sep, W T]; column w T + t holds the sep train
 *     rows of window w followed by its test row t; every feature is normalised by the mean and the unbiased std (+ 1e-6) of those sep + 1 values, then
 *     divided by `rescale`.  1 <= sep < bptt.
 *   mode PFN_TAB_NORM_TRAIN_ONLY (batch_pred:315-317, the baselines): x_out [bptt, W, F_out], y_out [bptt, W]; the statistics of the sep train rows are
 *     applied to all bptt rows; `rescale` is not used.  1 <= sep <= bptt.
 *   Columns F .. F_out - 1 are zeros (the reference's extend_features).  y_out may be NULL.  The train rows' mean m0 (a sum, then a centred correction) and
 *   their second moment about m0 are formed once per (window, feature) in f64 and never as a sum of squares of raw values; WITH_TEST folds the one test value in
 *   by the one-step Welford update.  A feature whose values (sep + 1, respectively sep) are all bit-equal is written as exactly 0 -- the padding columns, and
 *   constant columns too, where the reference writes (x - mean) / 1e-6 noise.
 *   1 <= F <= 1024, F <= F_out: else PFN_ERR_UNSUPPORTED; N, W >= 1, the sep ranges above, rescale > 0, a known mode, non-NULL X, y, starts, x_out, x_out
 *   16-byte aligned: else PFN_ERR_ARGUMENT / PFN_ERR_ALIGNMENT.
 *
 * pfn_auc_counts: scores [T,C], labels [T,C] (positive = label > 0.5) -> counts [C,4] int64 = (P positives, Nn negatives, gt = pairs (pos, neg) with
 *   s_pos > s_neg, eq = pairs with s_pos == s_neg).  AUC = (2 gt + eq) / (2 P Nn), formed by the caller in f64; a NaN score wins and ties nothing.
 *   1 <= T <= 4096 else PFN_ERR_UNSUPPORTED; C >= 1 and non-NULL buffers else PFN_ERR_ARGUMENT.
 *
 * pfn_knn_cv: P problems; train [P,n,F], labels [P,n] (class = label > 0.5), test [P,T,F], fold [P,n] int32 in 0 .. 4 (the CV test fold of each train row;
 *   a value outside takes no part in cv_correct).  Squared Euclidean distances in f32, an fma chain in ascending feature order; neighbours ordered by
 *   (d^2, train index), the lower index first at equal distance.  cv_correct [P,5,5] int32: [p][k-1][f] = rows of fold f whose class the majority of their k
 *   nearest train rows OUTSIDE fold f predicts (a split vote at even k predicts class 0); a row with fewer than k such neighbours counts as wrong.
 *   test_pos [P,T,5]: positives among the k nearest of all n train rows; test_nbr [P,T,5]: those neighbours' indices (-1 where n < k).
 *   4 <= n <= 128, 1 <= T <= 128, 1 <= F <= 128 else PFN_ERR_UNSUPPORTED; P >= 1 and non-NULL buffers else PFN_ERR_ARGUMENT. */
#define PFN_TAB_NORM_WITH_TEST 0
#define PFN_TAB_NORM_TRAIN_ONLY 1
int pfn_tabular_windows(const float* X, const float* y, const int32_t* starts, int64_t N, int F, int F_out, int W, int bptt, int sep, float rescale, int mode,
                        float* x_out, float* y_out, void* stream);
int pfn_auc_counts(const float* scores, const float* labels, int T, int C, int64_t* counts, void* stream);
int pfn_knn_cv(const float* train, const float* labels, const float* test, const int32_t* fold, int P, int n, int T, int F,
               int32_t* cv_correct, int32_t* test_pos, int32_t* test_nbr, void* stream);

/* ---- Logistic regression with its grid search (ABI 10, additive; csrc/logistic.hip): the reference's logistic_metric (tabular.py:325-346) as a batch of
 * independent convex fits.  f32 data, caller-owned buffers, stream-ordered, no allocation, no workspace, no host synchronisation, no global atomics.
 *
 * pfn_logistic_cv: P problems; train [P,n,F], labels [P,n] (class = label > 0.5, y~ = +1 / -1), test [P,T,F], fold [P,n] int32 (the CV test fold of each
 *   train row), NC candidates: cand_C [NC] f32 and cand_kind [NC] int32 = penalty code (PFN_LOGIT_NONE / L1 / L2) | PFN_LOGIT_FIT_INTERCEPT.  All on the device.
 *   One block per fit (problem p, candidate c, slot s): slot s < n_splits trains on the rows with fold[p,i] != s, slot s = n_splits on all rows (the refit),
 *   slots beyond are unused (status PFN_LOGIT_UNUSED, zeros).  A fit is a bitwise function of its own problem and candidate, wherever it sits in the call.
 *   Objective (scikit-learn's): C sum_i softplus(-y~_i z_i) + r(w), z = x w + b; r = 1/2 |w|^2 (l2), |w|_1 (l1), 0 (none: C is ignored, 1 is used); the
 *   intercept is never penalised; the start is w = 0.  Solver: proximal Newton -- H = C X^T D X (+ I on the penalised coordinates for l2) plus a damping of
 *   2^-16 trace(H) / d on the diagonal, the direction by Cholesky (l2, none) or by cyclic coordinate descent with soft-thresholding on the quadratic model (l1,
 *   at most 50 sweeps), Armijo backtracking (1e-4, at most 30 halvings) on the true objective's difference, at most 48 iterations.
 *   It stops with status PFN_LOGIT_CONVERGED when KKT_inf <= 64 2^-23 C max_j sum_i m_i |x_ij| (KKT: the minimum-norm subgradient; m_i = 1 on the fit's
 *   training rows; j over the features and, with an intercept, the column of ones), PFN_LOGIT_STALLED when backtracking finds no decrease, PFN_LOGIT_CAPPED at
 *   the iteration cap (e.g. 'none' on separable rows, which has no finite optimum), PFN_LOGIT_NONFINITE when a NaN reached the residual.  A fit whose training
 *   rows hold one class is not run: PFN_LOGIT_ONE_CLASS, zero coefficients, a zero count, NaN decision values.  A feature that is zero on all training rows of
 *   a fit has a coefficient of exactly 0 under every penalty.
 *   cv_correct [P,NC,5] int32: held-out rows of fold s with (z > 0) == class (z == 0 predicts class 0); test_z [P,NC,T]: the refit's decision values;
 *   status [P,NC,6,2] int32 = (exit reason, iterations); coef [P,NC,6,F+1] (may be NULL): the F weights, then the intercept (0 without one).
 *   4 <= n <= 128, 1 <= T <= 128, 1 <= F <= 128, 1 <= NC <= 64 else PFN_ERR_UNSUPPORTED; P >= 1, 2 <= n_splits <= 5 and non-NULL buffers else
 *   PFN_ERR_ARGUMENT; all of it before any launch. */
#define PFN_LOGIT_NONE 0
#define PFN_LOGIT_L1 1
#define PFN_LOGIT_L2 2
#define PFN_LOGIT_FIT_INTERCEPT 4
#define PFN_LOGIT_FOLDS 5
#define PFN_LOGIT_SLOTS 6
#define PFN_LOGIT_MAX_CANDIDATES 64
#define PFN_LOGIT_UNUSED 0
#define PFN_LOGIT_CONVERGED 1
#define PFN_LOGIT_STALLED 2
#define PFN_LOGIT_CAPPED 3
#define PFN_LOGIT_ONE_CLASS 4
#define PFN_LOGIT_NONFINITE 5
int pfn_logistic_cv(const float* train, const float* labels, const float* test, const int32_t* fold, const float* cand_C, const int32_t* cand_kind, int P, int n,
                    int T, int F, int NC, int n_splits, int32_t* cv_correct, float* test_z, int32_t* status, float* coef, void* stream);

/* ---- GP classifier with its grid search (ABI 10, additive; csrc/gpc.hip): the reference's gp_metric (tabular.py:480-503), i.e. scikit-learn's binary
 * GaussianProcessClassifier under the kernel c * RBF(l), as a batch of independent Laplace fits.  f32 data and arithmetic, caller-owned buffers, stream-ordered, no
 * allocation, no workspace, no host synchronisation, no global atomics.  The optimiser over theta is the caller's.
 *
 * Both calls: P problems; theta [P,NC,6,2] = (log c, log l) of every fit; train [P,n,F], labels [P,n] (class = label > 0.5), fold [P,n] int32 (the CV test fold
 *   of each train row).  One block per fit (problem p, candidate c, slot s): slot s < n_splits trains on the rows with fold[p,i] != s (compacted: held-out rows
 *   are not in K), slot s = n_splits on all rows (the refit), slots beyond are unused (status PFN_GPC_UNUSED).  A result is a bitwise function of its own
 *   (problem, theta, slot), wherever it sits in the call.
 *   Model: K = c exp(-d^2 / 2 l^2), no jitter.  Posterior mode by GPML algorithm 3.1 from f = 0 on every call (no warm start): pi = sigma(f), W = pi (1 - pi),
 *   B = I + W^1/2 K W^1/2 = L L^T, b = W f + (y - pi), a = b - W^1/2 B^-1 W^1/2 K b, f = K a, Z = -1/2 a.f - sum softplus(-(2y - 1) f) - sum log L_ii; as in
 *   scikit-learn, pi, W and L are those of the last iteration, one step behind f.  Newton stops PFN_GPC_CONVERGED two iterations after the first whose change
 *   of Z -- summed from the rows' term differences, not a difference of two totals -- is below 2^-20 max(1, |Z|) (scikit-learn: below 1e-10, in f64; the two
 *   further iterations bring the one-step-behind pi to f32's floor), or PFN_GPC_CAPPED after PFN_GPC_MAX_NEWTON = 100 iterations (scikit-learn's max_iter_predict).
 *   A non-positive pivot of B (PFN_GPC_NONPOSITIVE) or a non-finite Z or gradient (PFN_GPC_NONFINITE) fails that fit only.  A fit whose training rows hold one
 *   class is not run: PFN_GPC_ONE_CLASS.
 *   status [P,NC,6,2] int32 = (exit reason, Newton iterations).
 * pfn_gpc_lml_grad: value [P,NC,6] = -Z, grad [P,NC,6,2] = -dZ/dtheta by GPML algorithm 5.1 (K_0 = K, K_1 = K * d^2 / l^2), with tr(R K) = n - tr(B^-1) and
 *   s_2 = -1/2 (1 - diag(B^-1)) (1 - 2 pi) taken through B^-1 = L^-T L^-1 (the same numbers; they do not cancel in f32 where K is near rank one).  A failed fit
 *   gives +inf and a zero gradient, a one-class fit NaN and a zero gradient, an unused slot zeros.
 * pfn_gpc_predict: finds the mode at theta once more; test [P,T,F].  A decision value f* = k*^T (y - pi) is written as a pair (m, e) with f* = m exp(-e): e the
 *   smallest exponent argument d^2 / 2 l^2 over the fit's training rows, m = sum_i c exp(e - d_i^2 / 2 l^2) (y_i - pi_i) -- the sign of f* survives where exp
 *   underflows in f32; the caller forms f* in f64.  Slot s < n_splits writes cv_f [P,NC,n,2] at its held-out rows (fold == s) only; a row in no fold is never
 *   written.  The refit slot writes test_f [P,NC,T,2] and test_var [P,NC,T] = max(c - |L^-1 W^1/2 k*|^2, 0).  A failed or one-class fit writes NaN there.
 *   4 <= n <= PFN_GPC_MAX_N = 112 (three n x n matrices in 160 KB of LDS), 1 <= T <= 128, 1 <= F <= 128, 1 <= NC <= 64 else PFN_ERR_UNSUPPORTED; P >= 1,
 *   2 <= n_splits <= 5 and non-NULL buffers else PFN_ERR_ARGUMENT; all of it before any launch. */
#define PFN_GPC_FOLDS 5
#define PFN_GPC_SLOTS 6
#define PFN_GPC_MAX_CANDIDATES 64
#define PFN_GPC_MAX_N 112
#define PFN_GPC_MAX_NEWTON 100
#define PFN_GPC_UNUSED 0
#define PFN_GPC_CONVERGED 1
#define PFN_GPC_CAPPED 2
#define PFN_GPC_ONE_CLASS 3
#define PFN_GPC_NONPOSITIVE 4
#define PFN_GPC_NONFINITE 5
int pfn_gpc_lml_grad(const float* theta, const float* train, const float* labels, const int32_t* fold, int P, int n, int F, int NC, int n_splits, float* value,
                     float* grad, int32_t* status, void* stream);
int pfn_gpc_predict(const float* theta, const float* train, const float* labels, const float* test, const int32_t* fold, int P, int n, int T, int F, int NC,
                    int n_splits, float* cv_f, float* test_f, float* test_var, int32_t* status, void* stream);

/* ---- BNN classifier with its grid search (ABI 10, additive; csrc/bnn_cv.hip): the reference's bayes_net_metric (tabular.py:372-478) as a batch of independent
 * SVI fits -- the model, the guide and the step of pfn_bnn_svi_steps at activation = 0 with ONE particle -- followed by their predictive.  f32 data, caller-owned
 * buffers, stream-ordered, no allocation, no workspace, no host synchronisation, no atomics.
 *
 * pfn_bnn_cv: P problems; train [P,n,F], labels [P,n] (class y = label > 0.5), test [P,T,F], fold [P,n] int32 (the CV test fold of each train row), all on the
 *   device; NC candidates (width H_c, learning rate lr_c): cand_H [NC] int32 and cand_lr [NC] f32 are HOST arrays, read before the call returns.  One block per fit
 *   (problem p, candidate c, slot s): slot s < n_splits trains on the rows with fold[p,i] != s, slot s = n_splits on all rows (the refit), slots beyond are unused
 *   (status PFN_BNN_CV_UNUSED, nothing else written).  A row whose fold value is outside 0 .. n_splits - 1 trains every slot and is held out by none.  A training
 *   part that holds one class is fitted like any other.
 * Model: theta = (W1 [H,F] row-major, b1 [H], W2 [2,H], b2 [2]), D = H (F + 3) + 2; o = W2 (W1 x + b1) + b2;
 *   U(theta) = |theta|^2 / 2 + (D / 2) log 2 pi - sum_i m_i log softmax(o_i)[y_i], m_i = 1 on the slot's training rows (a row with m_i = 0 is not read by the
 *   steps: a NaN there stays there).  Guide q = N(loc, diag(scale^2)), scale = softplus(u); per step theta = loc + scale eps,
 *   L = U(theta) - sum_i (log scale_i + eps_i^2 / 2) - (D / 2) log 2 pi, g_loc = grad U(theta), g_scale = grad U(theta) * eps - 1 / scale, g_u = g_scale sigmoid(u), then
 *   torch.optim.Adam without weight decay on loc and u exactly as stated for pfn_bnn_svi_steps (beta^t in f64, t = absolute step index + 1) with lr = lr_c.
 *   The sums over rows, features and hidden units are accumulated in f64 and rounded once to f32; everything else is f32.
 * state [P,NC,6 slots,6 rows,ld] f32, caller-owned; rows loc, u, m_loc, v_loc, m_u, v_u; ld >= the largest candidate's D; columns >= that candidate's own D, and the
 *   unused slots, are never read or written.  The launch runs steps step0 .. step0 + num_steps - 1; loss [P,NC,6,num_steps] (or NULL) receives L of every step,
 *   evaluated before the step's update.
 * Predictive: after the steps, skipped when num_pred_samples = S = 0; draws theta_k = loc + scale eps_k, k < S, prob_k(x) = sigmoid(o_1 - o_0).  Slot s < n_splits
 *   writes cv_prob [P,NC,n] at its held-out rows (fold == s) only -- a row in no fold is never written --, the refit slot writes test_prob [P,NC,T]: the mean over
 *   the draws, added in draw order in f64 and rounded once.  cv_draw / test_draw (same shapes, NULL to skip) are the reference's estimator, the mean over the draws
 *   of a Bernoulli observation obs_k = (u_k < prob_k).
 * Noise: q = (problem_ids[p], int64 [P] on the device, or p when NULL) * 8 + slot; it does not depend on the candidate, so the candidates of a problem share their
 *   random numbers.  With B(idx) = philox4x32_10(idx, stream = q, key = seed):
 *     eps of coordinate i at absolute step t  = component i & 3 of normal4(B((t << 12) | (i >> 2)))
 *     eps of coordinate i in predictive draw k = component i & 3 of normal4(B(((2^41 + k) << 12) | (i >> 2)))
 *     u of row r in predictive draw k          = (word r & 3 of B(((2^42 + k) << 12) | (r >> 2)) >> 8) * 2^-24;  r = i for train row i, n + j for test row j
 *   (normal4: Box-Muller on the block's four words, as for pfn_bnn_svi_steps).  D <= 8386 uses the blocks 0 .. 2096 of 4096; the three domains are disjoint.
 * A fit is a bitwise function of its own problem, candidate (H, lr), slot, q and seed, wherever it sits in the call and however the candidates are grouped into
 *   calls; steps(0, a + b) equals steps(0, a) followed by steps(a, b); the predictive in a call of its own (num_steps = 0) equals the predictive at the end of a
 *   stepping call.  A fit whose state is or becomes non-finite stays alone in that.  status [P,NC,6] int32: PFN_BNN_CV_UNUSED, PFN_BNN_CV_DONE, or
 *   PFN_BNN_CV_NONFINITE where loc or u left the finite numbers during the call (or, in a predictive-only call, were not finite).
 * 4 <= n <= 128, 1 <= T <= 128, 1 <= F <= 128, 1 <= NC <= PFN_BNN_CV_MAX_CANDIDATES, every 1 <= cand_H <= 64, else PFN_ERR_UNSUPPORTED (a NULL cand_H is an
 *   argument error); P >= 1, 2 <= n_splits <= 5, ld >= max D, 0 <= step0 <= 2^40, num_steps >= 0, 0 <= num_pred_samples <= 2^20, every lr finite and >= 0, beta1 /
 *   beta2 in [0, 1), eps >= 0, non-NULL train, labels, test, fold, cand_H, cand_lr, state, status, and non-NULL cv_prob and test_prob when num_pred_samples > 0,
 *   else PFN_ERR_ARGUMENT; the limits are checked first, all of it before any device pointer is read and before any HIP call.  num_steps = 0 with
 *   num_pred_samples = 0 returns at once. */
#define PFN_BNN_CV_FOLDS 5
#define PFN_BNN_CV_SLOTS 6
#define PFN_BNN_CV_MAX_CANDIDATES 64
#define PFN_BNN_CV_UNUSED 0
#define PFN_BNN_CV_DONE 1
#define PFN_BNN_CV_NONFINITE 2
int pfn_bnn_cv(const float* train, const float* labels, const float* test, const int32_t* fold, const int32_t* cand_H, const float* cand_lr, int P, int n, int T,
               int F, int NC, int n_splits, float* state, int64_t ld, int64_t step0, int num_steps, float beta1, float beta2, float eps, int num_pred_samples,
               uint64_t seed, const int64_t* problem_ids, float* loss, float* cv_prob, float* test_prob, float* cv_draw, float* test_draw, int32_t* status,
               void* stream);

/* ---- Gradient-boosted trees with their grid search (ABI 10, additive; csrc/xgb_cv.hip): the reference's xgb_metric (tabular.py:599-626) as a batch of
 * independent fits of the exact greedy algorithm on logistic loss.  f32 data, caller-owned buffers, stream-ordered, no allocation, no host synchronisation, no
 * atomics.  No boosting library is carried or compared against: this text is the specification.
 *
 * pfn_xgb_cv: P problems; train [P,n,F], labels [P,n] (class y = label > 0.5), test [P,T,F], fold [P,n] int32 (the CV test fold of each train row), all on the
 *   device; NC candidates as HOST arrays read before the call returns: cand_depth int32, cand_lr f32 (eta), cand_mcw, cand_subsample, cand_colsample f64, cand_ids
 *   int32 or NULL (0 .. NC-1).  Two launches: the sort orders, then one block per fit (problem p, candidate c, slot s): slot s < n_splits trains on the rows with
 *   fold[p,i] != s, slot s = n_splits on all rows (the refit), slots beyond are unused (status PFN_XGB_CV_UNUSED, nothing else written).  A row whose fold value
 *   is outside 0 .. n_splits - 1 trains every slot and is held out by none.
 * order [P,F,n] uint8, caller-owned workspace: the first launch writes the stable argsort of every column over all n rows, key (value, row index).
 * A fit: every margin starts at 0.  Round t = 0 .. num_rounds - 1:
 *   p = sigmoid(margin), g = p - y, h = p (1 - p) in f32, then gi = rint(g 2^23), hi = rint(h 2^23) as int32; every sum of them is an integer sum.
 *   Row sample: train row i of the slot is in iff its word < floor(subsample 2^32).  Column sample: the k = max(1, floor(colsample F)) features of smallest
 *   (word, feature index).  With B(idx) = philox4x32_10(idx, stream = ((problem_ids[p] or p) * 64 + (cand_ids[c] or c)) * 8 + s, key = seed):
 *     word of row i     = component i & 3 of B((t << 6) | (i >> 2))                 (i: the row's index among the n rows of the window)
 *     word of feature f = component f & 3 of B(2^32 | (t << 6) | (f >> 2))
 *   The tree grows level by level to cand_depth.  A node's candidates: for every sampled feature, between two consecutive DISTINCT values a < b in the feature's
 *   sorted order of the node's sampled rows.  With the integer sums of the two sides scaled by 2^-23 (int -> f32 conversion, then the product), lambda = 1:
 *     legal iff HLi >= mcwi and HRi >= mcwi,  mcwi = rint(min_child_weight 2^23)  (formed in f64 on the host, compared as integers)
 *     gain = (GL^2 / (HL + 1) + GR^2 / (HR + 1)) - G^2 / (H + 1) in f32, every operation rounded once
 *   The node splits on the legal candidate of largest gain if that gain > 1e-6; among bit-equal gains the lowest feature index, then the lowest position wins.
 *   Threshold thr = 0.5f (a + b) in f32, and b where that equals a; a row goes left iff x < thr.  Leaf value -eta G / (H + 1) = eta * -(G / (H + 1)) over the
 *   leaf's sampled rows (0 with none).  Every train row (sampled or not, held out or not) and, in the refit slot, every test row takes margin += leaf value.
 * Outputs: slot s < n_splits writes the final margins of its held-out rows (fold == s) into cv_margin [P,NC,n] -- a row in no fold is never written --, the refit
 *   slot those of the test rows into test_margin [P,NC,T].  status [P,NC,6] int32: PFN_XGB_CV_UNUSED, PFN_XGB_CV_DONE, or PFN_XGB_CV_NONFINITE where a value the
 *   fit read or a final margin is not finite (NaN is refused, not treated as missing: such a fit's numbers mean nothing).
 *   tree_feature / tree_threshold [P,NC,6,num_rounds,3] and tree_leaf [P,NC,6,num_rounds,4] (all three or all NULL): per round the root and its left and right
 *   child (feature, or -1 where the node does not split, then threshold 0), and the leaf values by code 2 (right of the root) + (right of the child); a node
 *   that does not split keeps its rows at the code of its left side.  The unused slots are never written.
 * A fit is a bitwise function of its own problem, candidate parameters, slot, ids and seed, wherever it sits in the call and however problems and candidates
 *   are grouped into calls.
 * 4 <= n <= 128, 1 <= T <= 128, 1 <= F <= 128, 1 <= NC <= PFN_XGB_CV_MAX_CANDIDATES, 0 <= num_rounds <= PFN_XGB_CV_MAX_ROUNDS, every 1 <= cand_depth <=
 *   PFN_XGB_CV_MAX_DEPTH, subsample and colsample in (0, 1], min_child_weight >= 0, learning rate > 0, else PFN_ERR_UNSUPPORTED; P >= 1, 2 <= n_splits <= 5,
 *   non-NULL train, labels, test, fold, the five candidate arrays, order, cv_margin, test_margin, status, the tree buffers all or none, every candidate number
 *   finite, 0 <= cand_ids < 64, else PFN_ERR_ARGUMENT; the limits are checked first, all of it before any device pointer is read and before any HIP call. */
#define PFN_XGB_CV_FOLDS 5
#define PFN_XGB_CV_SLOTS 6
#define PFN_XGB_CV_MAX_CANDIDATES 64
#define PFN_XGB_CV_MAX_DEPTH 2
#define PFN_XGB_CV_MAX_ROUNDS 4096
#define PFN_XGB_CV_UNUSED 0
#define PFN_XGB_CV_DONE 1
#define PFN_XGB_CV_NONFINITE 2
int pfn_xgb_cv(const float* train, const float* labels, const float* test, const int32_t* fold, const int32_t* cand_depth, const float* cand_lr,
               const double* cand_mcw, const double* cand_subsample, const double* cand_colsample, const int32_t* cand_ids, int P, int n, int T, int F, int NC,
               int n_splits, int num_rounds, uint64_t seed, const int64_t* problem_ids, uint8_t* order, float* cv_margin, float* test_margin, int32_t* status,
               int32_t* tree_feature, float* tree_threshold, float* tree_leaf, void* stream);

/* ---- Oblivious boosted trees with their grid search (ABI 10, additive; csrc/catboost_cv.hip): the reference's catboost_metric (tabular.py:556-596) as a batch
 * of independent fits of symmetric (oblivious) trees on logistic loss.  f32 data, caller-owned buffers, stream-ordered, no allocation, no host synchronisation,
 * no atomics.  No boosting library is carried or compared against: this text is the specification (INTEGRATION.md lists what it restates from memory).
 *
 * pfn_catboost_cv: P problems; train [P,n,F], labels [P,n] (class y = label > 0.5), test [P,T,F], fold [P,n] int32, all on the device; NC candidates as HOST
 *   arrays read before the call returns: cand_depth int32, cand_lr f32, cand_l2 f32, cand_ids int32 or NULL (0 .. NC-1); checkpoints: a HOST array of
 *   1 <= NK <= 8 ascending tree counts >= 1, the last equal to num_rounds.  Two launches: the sort orders, then one block per fit (problem p, candidate c,
 *   slot s): slot 0, the search fit, learns on the rows with fold != 0; slot 1, the refit, learns on all rows.
 * order [P,F,n] uint8, caller-owned workspace: the first launch writes the stable argsort of every column over all n rows, key (value, row index).
 * A fit, m its number of learn rows: every margin starts at 0; no row or column sampling.  sig(z) = (z >= 0 ? 1 : e) / (1 + e) with e = exp(-|z|).  Every f32
 *   operation below is rounded once (no fused multiply-add).
 * Borders: for every feature, between two consecutive distinct values a < b of the fit's learn rows in the column's sorted order: thr = 0.5f (a + b) in f32,
 *   and a where that equals b; a row's bit is 1 iff x > thr.  The border's position j is the sorted position (over all n rows) of the last learn row that holds a.
 * Tree t = 0 .. num_rounds - 1: p = sig(margin), g = y - p in f32, gi = rint(g 2^23) as int32 over the learn rows; every per-leaf sum of gi and every count is
 *   an integer sum.  S2 = sum gi^2 (an integer).  The tree grows level by level, d = 0 .. depth - 1; one (feature, border) splits all leaves of a level and the
 *   row's leaf code gains bit d.  A candidate is every (feature, border) not already used in this tree; with none left the tree ends at the levels it has.
 *   Score of a candidate: over the leaves of the level so far in ascending code, those without learn rows left out, the two children low (bit 0) and high (bit
 *   1) with integer sums Gi and counts c:  G = (float)Gi * 2^-23, avg = c > 0 ? G / ((float)c + l2) : 0, and four running f32 sums from 0,
 *     num_lo += avg G, den_lo += (avg avg) c over the low children, num_hi, den_hi over the high ones (an empty child adds nothing);
 *     num = num_lo + num_hi, den = den_lo + den_hi, score = den > 0 ? num / sqrt(den) : 0.
 *   Noise: sigma_t = sqrt(((float)S2 * 2^-46) / (float)m) * (L / (1 + L)), L = exp(log((float)m) - (float)t * lr), in f32.  With B(idx) = philox4x32_10(idx,
 *     stream = ((problem_ids[p] or p) * 64 + (cand_ids[c] or c)) * 8 + s, key = seed) and (w0, w1) the first two words of B((t << 17) | (d << 14) | (f << 7) | j):
 *     u1 = ((w0 >> 9) + 0.5) 2^-23, u2 = (w1 >> 8) 2^-24 (both exact in f32), z = sqrt(-2 log u1) * cos(pi * (2 u2)).  The compared value is score + sigma_t * z;
 *     the largest wins, among bit-equal values the lowest feature, then the lowest position.
 *   Leaf values, over the leaves that hold learn rows (any other leaf has value 0): v = 0, obj = objective(v), then at most 10 Newton iterations:
 *     per learn row z = margin + v_leaf, r = y ? sig(-z) : -sig(z) (that is y - sig(z), without the cancellation), h = sig(z) sig(-z); ri = rint(r 2^40),
 *     hi = rint(h 2^40) as int64 (2^40, not 2^23: a saturated leaf's h is a few units of 2^-23, and a step would stand on their rounding); per leaf the integer
 *     sums R, H:  den = (float)H * 2^-40 + l2,  step = den > 0 ? ((float)R * 2^-40) / den : 0.
 *     Backtracking ("AnyImprovement"): for scale = 1, 1/2, .., 2^-10:  try_leaf = v_leaf + scale * step_leaf;  the first scale with objective(try) <= obj is
 *     taken (v = try, obj = objective(try)); with none the iteration loop ends with v as it was.
 *     objective(v) = (float)(sum over the learn rows of rint(loss 2^40) as int64) * 2^-40 + (0.5f * l2) * pen,  loss = max(y ? -z : z, 0) + log1p(exp(-|z|)) at
 *     z = margin + v_leaf,  pen = the f32 sum of v_leaf^2 from 0 over the leaves with learn rows in ascending code.
 *   Then every row of the window (learn or held out) and, in the refit slot, every test row takes margin += lr * v_leaf (its leaf by its own bits).
 * Outputs: after tree checkpoints[k] - 1, slot 0 writes the margins of the rows with fold == 0 into hold_margin [P,NC,NK,n] (the other rows are never written),
 *   slot 1 those of the test rows into test_margin [P,NC,NK,T].  status [P,NC,2] int32: PFN_CATBOOST_CV_DONE; PFN_CATBOOST_CV_NONFINITE where a value of the
 *   window's rows (or, in slot 1, the test rows) is not finite -- NaN is refused, not treated as missing -- or a final margin is not; PFN_CATBOOST_CV_ONE_CLASS
 *   where the learn rows hold one class (the library raises there).  A fit that is NONFINITE by its inputs or ONE_CLASS writes nothing but its status.
 *   tree_feature int32 / tree_threshold f32 [P,NC,2,num_rounds,7] and tree_leaf [P,NC,2,num_rounds,128] (all three or all NULL): per tree and level the chosen
 *   feature and threshold (-1 and 0 for a level the tree does not have), and lr * v by leaf code (0 for a leaf without learn rows).
 * Nothing in a fit depends on the trees after it: the margins at checkpoint k are those of a launch with num_rounds = checkpoints[k].  A fit is a bitwise
 *   function of its own problem, candidate parameters, slot, ids and seed, wherever it sits in the call and however problems and candidates are grouped.
 * 4 <= n <= 128, 1 <= T <= 128, 1 <= F <= 128, 1 <= NC <= PFN_CATBOOST_CV_MAX_CANDIDATES, 1 <= num_rounds <= PFN_CATBOOST_CV_MAX_ROUNDS, every 1 <= cand_depth
 *   <= PFN_CATBOOST_CV_MAX_DEPTH, else PFN_ERR_UNSUPPORTED; P >= 1, non-NULL train, labels, test, fold, the three candidate arrays, checkpoints, order,
 *   hold_margin, test_margin, status, the tree buffers all or none, 1 <= NK <= 8 with the checkpoints as above, every l2 >= 0 and finite, every learning rate
 *   > 0 and finite, 0 <= cand_ids < 64, else PFN_ERR_ARGUMENT; the limits are checked first, all of it before any device pointer is read and before any HIP
 *   call. */
#define PFN_CATBOOST_CV_SLOTS 2
#define PFN_CATBOOST_CV_MAX_CANDIDATES 64
#define PFN_CATBOOST_CV_MAX_DEPTH 7
#define PFN_CATBOOST_CV_MAX_LEAVES 128
#define PFN_CATBOOST_CV_MAX_ROUNDS 1024
#define PFN_CATBOOST_CV_MAX_CHECKPOINTS 8
#define PFN_CATBOOST_CV_DONE 1
#define PFN_CATBOOST_CV_NONFINITE 2
#define PFN_CATBOOST_CV_ONE_CLASS 3
int pfn_catboost_cv(const float* train, const float* labels, const float* test, const int32_t* fold, const int32_t* cand_depth, const float* cand_lr,
                    const float* cand_l2, const int32_t* cand_ids, const int32_t* checkpoints, int P, int n, int T, int F, int NC, int NK, int num_rounds,
                    uint64_t seed, const int64_t* problem_ids, uint8_t* order, float* hold_margin, float* test_margin, int32_t* status, int32_t* tree_feature,
                    float* tree_threshold, float* tree_leaf, void* stream);

/* ---- BNN prior sampler: replaces the per-dataset module forwards of priors.mlp.get_batch (priors/mlp.py:116-124
 * network, :150-157 forward of the non-causal branch, :195-197 Python loop over datasets).  For dataset b with model
 * m = model_of[b]:  h_0 = causes W_0^T + b_0;  h_l = act(h_{l-1}) W_l^T + b_l + noise_std[m] * eps_l  (1 <= l < L_m);
 * y[b,t] = h_{L-1}[t, 0].
 * weights [num_models][Lmax][HP][HP] f32: layer l stored TRANSPOSED ([in][out]) and zero padded to HP (a multiple of 4,
 * <= 152); biases [num_models][Lmax][HP]; dims [num_models][3] = (num_causes, hidden, num_layers); noise_std [num_models].
 * causes [B][T][HP]: filled with N(0,1) in the first num_causes columns when gen_causes != 0 (the x of the dataset),
 * else taken as input.  noise: NULL (generated, Philox) or [B][Lmax-1][T][HP] standard normals.
 * hidden: NULL, or [B][Lmax-1][T][HP] receiving the outputs (noise included) of layers 1 .. L-1 -- the node pool from which the
 * causal variant (priors/mlp.py:158-166, `outputs[2:]`) picks its features and target.
 * activation: 0 identity, 1 relu, 2 tanh, 3 sigmoid. */
int pfn_mlp_prior_forward(const float* weights, const float* biases, const int32_t* model_of, const int32_t* dims,
                          const float* noise_std, float* causes, const float* noise, float* y, float* hidden,
                          int B, int T, int HP, int Lmax, int activation, int gen_causes,
                          uint64_t seed, uint64_t offset, void* stream);

/* ---- Stroke prior of the few-shot study (ABI 10, additive): replaces the Pillow drawing loop of priors.stroke.get_batch (priors/stroke.py:9-63, :95-110).
 * An image is up to PFN_STROKE_MAX_STROKES straight strokes of one width on a size x size 8-bit canvas, exactly the pixels Pillow's ImageDraw.line lights
 * (csrc/stroke_prior.hip states the rule), each lit pixel holding a noise byte in 200 .. 254, blurred as Pillow's GaussianBlur(0.2) blurs it; the output is
 * byte / 255 in f32, correctly rounded, and with normalize != 0 (x - mean) / (std + 1e-6) per image, std the unbiased one.  A stroke with a coordinate beyond
 * +-PFN_STROKE_COORD_LIMIT is not drawn.  Stream-ordered, no allocation, no host synchronisation, no atomics.
 * pfn_stroke_render: N images from explicit parameters.  segs [N,8,4] int32 = (x0, y0, x1, y1), 16-byte aligned; n_strokes [N], width [N] int32 -- DEVICE
 *   arrays, so the call cannot refuse their values: the kernel clamps them to 0 .. 8 and 0 .. PFN_STROKE_MAX_WIDTH (hipops.stroke_render checks them first).
 *   noise [N,size^2] uint8 or NULL: then pixel x of row y of image n takes word x % 4 of the Philox4x32-10 block at counter (n * 64 + y) * 16 + x / 4,
 *   stream word offset * 8 + 4, key seed, as 200 + mulhi(u32, 55).  x: image n at x + n * image_stride floats (image_stride >= size^2, so a caller can write
 *   into a larger layout); raw / img [N,size^2] uint8 or NULL: the image before / after the blur.
 *   8 <= size <= 64 else PFN_ERR_UNSUPPORTED; N >= 0, image_stride >= size^2, non-NULL segs, n_strokes, width, x, segs 16-byte and the others 4-byte aligned else
 *   PFN_ERR_ARGUMENT; all of it before any launch.  N == 0: PFN_OK, nothing launched.
 * pfn_stroke_prior_sample: the prior.  Dataset b (global index d = first_dataset + b, so dataset b of a batch equals a call with B = 1, first_dataset = b) has
 *   num_classes classes; image (b, t) is one of class labels[b,t] and lands in x [T,B,size^2].  Counter-based randomness: Philox4x32-10, counter = a global
 *   index, stream word = offset * 8 + purpose, key = seed; an integer in [lo, hi] is lo + mulhi(u32, hi - lo + 1), whose bias is below (hi - lo + 1) 2^-32.
 *   Class (d, c): stroke count in [strokes_lo, strokes_hi] from counter d * num_classes + c (purpose 0).  Stroke s of it, pass p < PFN_STROKE_MAX_PASSES = 256:
 *   the block at counter ((d * 16 + c) * 8 + s) * 256 + p (purpose 1) gives (length, start x, start y, angle); length in [len_lo, len_hi] and the start in
 *   [start_lo, start_hi]^2 are taken anew when p % 3 == 0, the angle theta = u32 * 2 pi / 2^32 on every pass; the pass is accepted iff both coordinates of
 *   start + length (cos theta, sin theta) lie in [0, size - 1] (f64).  On the cap the last draw stays and status[b] counts it.
 *   Image g = d * T + t: the block at counter g (purpose 2) gives (width in [width_lo, width_hi], offset x, offset y in [-max_offset, max_offset]); word pair
 *   s % 2 of the block at counter g * 4 + s / 2 (purpose 3) the jitter of stroke s in [-max_target_offset, max_target_offset]^2; p0 = start + offset,
 *   p1 = rint(p0 + (length (cos theta, sin theta) + jitter)) in f64, every step rounded; the noise as pfn_stroke_render with n = g.
 *   Returned beside x: cls_n [B,C], cls_len [B,C,8], cls_start [B,C,8,2] int32, cls_dir [B,C,8] f64 (theta), segs [B,T,8,4], width [B,T] int32 (all required),
 *   raw / img [B,T,size^2] uint8 or NULL, status [B] int32.
 *   8 <= size <= 64, 1 <= num_classes <= PFN_STROKE_MAX_CLASSES, strokes_hi <= 8, width_hi <= PFN_STROKE_MAX_WIDTH, len_hi, start_hi, max_offset,
 *   max_target_offset <= 1024 else PFN_ERR_UNSUPPORTED; B, T >= 1, B * T < 2^31, 0 <= lo <= hi for every range, max_offset, max_target_offset >= 0, non-NULL
 *   and aligned buffers (segs 16 bytes, cls_dir 8, the others 4) else PFN_ERR_ARGUMENT; all of it before any launch. */
#define PFN_STROKE_MAX_STROKES 8
#define PFN_STROKE_MAX_CLASSES 16
#define PFN_STROKE_MAX_WIDTH 64
#define PFN_STROKE_MAX_PASSES 256
#define PFN_STROKE_COORD_LIMIT 4096
int pfn_stroke_render(const int32_t* segs, const int32_t* n_strokes, const int32_t* width, const uint8_t* noise, int64_t N, int size, int normalize,
                      int64_t image_stride, uint64_t seed, uint64_t offset, float* x, uint8_t* raw, uint8_t* img, void* stream);
int pfn_stroke_prior_sample(const int32_t* labels, int B, int T, int num_classes, int size, int normalize, int strokes_lo, int strokes_hi, int len_lo, int len_hi,
                            int start_lo, int start_hi, int width_lo, int width_hi, int max_offset, int max_target_offset, uint64_t seed, uint64_t offset,
                            uint64_t first_dataset, float* x, int32_t* cls_n, int32_t* cls_len, int32_t* cls_start, double* cls_dir, int32_t* segs, int32_t* width,
                            uint8_t* raw, uint8_t* img, int32_t* status, void* stream);

/* ---- Omniglot episode loader of the few-shot study (ABI 10, additive; csrc/episode.hip): replaces the per-image loop of priors/omniglot.py:13-35 and the
 * numpy loops of datasets/omniglotNshot.py:31-77, :172-230 over an IMAGE BANK on the device, bank [n_classes, n_img, size, size]: f32 (table == NULL) or uint8
 * with a 256-entry f32 table (a pixel's value is table[byte]); the background is the value 0.0f in both.  Stream-ordered, no allocation, no host
 * synchronisation, no atomics.  Every output image is: source image src = class * n_img + image; rotated by k quarter turns exactly as np.rot90(a, k,
 * axes=(-2, -1)); the bounding box (c0, c1, r0, r1) of the pixels != 0 of the rotated image; a shift tx in [-c0, size-1-c1], ty in [-r0, size-1-r1];
 * out[y][x] = rot[y - ty][x - tx] where that lies inside the image, else 0.0f.  The output value is the source value bit for bit.  An image without content has
 * bbox (0, -1, 0, -1), gets tx = ty = 0 and is counted in status (the reference raises an IndexError there).
 * Randomness: Philox4x32-10, counter = a global index, stream word = offset * 8 + purpose, key = seed; an integer in [lo, hi] is lo + mulhi(u32, hi - lo + 1),
 * whose bias is below (hi - lo + 1) 2^-32.  Word m of a run is component m % 4 of the block at base + m / 4.
 * pfn_episode_gather: N images from explicit parameters.  src [N], rot [N] (NULL: none) int32 -- DEVICE arrays, so the call cannot refuse their values: the
 *   kernel clamps them to 0 .. n_classes n_img - 1 and 0 .. 3 (hipops.episode_gather checks them first).  shift_in [N,2] = (tx, ty) or NULL; given shifts are
 *   applied as they are (clamped to +-size: content may leave the frame).  With shift_in == NULL and translate != 0 image n draws (tx, ty) from words .x, .y of
 *   the block at counter first_image + n, purpose 5; with translate == 0 the shift is (0, 0).  Image n is written at x + n * image_stride floats (image_stride >=
 *   size^2; floats between images are left untouched).  Returned: bbox [N,4] = (c0, c1, r0, r1), shift [N,2] as used; status [1] or NULL: images without content.
 * pfn_episode_sample: the loader's draw for B datasets of T = n_way k_shot + 1 positions: x [T,B,size^2] f32, labels [B,T], targets [B,T] (-100 except at the
 *   last position) and, for tests and replay, classes [B,n_way] (bank class of label j), rotations [B,n_way], src [B,T], shift [B,T,2], bbox [B,T,4],
 *   status [B] (images without content), all int32.  Every draw is a function of (seed, offset, d = first_dataset + b): dataset b of a batch equals a call with
 *   B = 1, first_dataset = b; image (b, t) is pfn_episode_gather's image n with first_image + n = d T + t.
 *   A k-subset of n is drawn by the rank rule: draw j takes r = mulhi(word j, n - j), the rank of the pick among the values not yet taken (walking the taken
 *   values in ascending order, r += 1 for each one <= r): every ordered selection has probability prod_j 1 / (n - j), each factor within (n - j) 2^-32.  A
 *   permutation of n is Fisher-Yates: for i = n-1 .. 1 swap(a[i], a[mulhi(word n-1-i, i+1)]).
 *   mode PFN_EPISODE_STANDARD (OmniglotNShot.load_data_cache, datasets/omniglotNshot.py:184-212): classes = the n_way-subset of the pool [pool_lo, pool_hi)
 *     (purpose 0, base 4 d; :190); label j = position in the selection (:192); class j takes the k_shot-subset of n_img (purpose 1, base 16 (16 d + j)) and the
 *     query class one more draw of that run (:194 draws k_shot + 1 for every class; only one query is used); rotation of class j = mulhi(word j, 4) (purpose 3,
 *     base 4 d), applied to support and query alike (:196-202); the support positions are one permutation of the class-major list (purpose 4, base 256 d;
 *     :207-209); the query class is mulhi(.x, n_way) of the block at counter d, purpose 2 (:210-212 permutes n_way queries of which priors/omniglot.py:61 keeps
 *     the first).  The reference's cache of ten batches (:184) only amortises its loop: draws here are fresh on every call.
 *   mode PFN_EPISODE_JONAS (OmniglotNShotJonas.next, :38-75): the alphabet is mulhi(.y, n_alphabets) of the block at counter d, purpose 2 (:38); the classes are
 *     alphabet_offsets[alphabet] + a permutation of range(n_way) (purpose 0) -- the FIRST n_way classes of the alphabet, as the reference permutes range(n_way)
 *     (:43); train != 0: images as in standard mode (:49-51); train == 0: the support is a permutation of images 0 .. k_shot-1 (purpose 1, k_shot - 1 words) and
 *     the query class's query k_shot + mulhi(word k_shot-1, n_img - k_shot) (:53-54); no rotation; the support stays class-major and unshuffled (:68); the query
 *     class as above (:72-75).  alphabet_offsets [n_alphabets + 1] int32 is a DEVICE array: the caller guarantees offsets[a] + n_way <= offsets[a+1] <= n_classes
 *     (hipops checks it on the host when the bank is built; the kernel clamps a class to the bank).
 *   PFN_ERR_UNSUPPORTED: size outside 8 .. 64, n_img outside 1 .. 64, n_way outside 1 .. 16, an unknown mode.  PFN_ERR_ARGUMENT: k_shot outside 1 .. n_img-1,
 *   a pool outside [0, n_classes) or with fewer than n_way classes, B < 0, N < 0, B T or N or n_classes n_img >= 2^31, image_stride < size^2, jonas mode without
 *   offsets, a NULL or misaligned buffer (4 bytes; the uint8 bank 1).  All of it before any launch; B == 0 or N == 0: PFN_OK, nothing launched. */
#define PFN_EPISODE_MIN_SIZE 8
#define PFN_EPISODE_MAX_SIZE 64
#define PFN_EPISODE_MAX_WAY 16
#define PFN_EPISODE_MAX_IMAGES 64
#define PFN_EPISODE_STANDARD 0
#define PFN_EPISODE_JONAS 1
int pfn_episode_gather(const void* bank, const float* table, int n_classes, int n_img, int size, const int32_t* src, const int32_t* rot, const int32_t* shift_in,
                       int64_t N, int translate, int64_t image_stride, uint64_t seed, uint64_t offset, uint64_t first_image, float* x, int32_t* bbox, int32_t* shift,
                       int32_t* status, void* stream);
int pfn_episode_sample(const void* bank, const float* table, int n_classes, int n_img, int size, int B, int n_way, int k_shot, int mode, int train, int translate,
                       int pool_lo, int pool_hi, const int32_t* alphabet_offsets, int n_alphabets, uint64_t seed, uint64_t offset, uint64_t first_dataset, float* x,
                       int32_t* labels, int32_t* targets, int32_t* classes, int32_t* rotations, int32_t* src, int32_t* shift, int32_t* bbox, int32_t* status,
                       void* stream);

/* ---- Class-label embedding of the few-shot study (ABI 10, additive; csrc/class_embed.hip): the embedding of a model whose x-encoder is nn.Linear and whose
 * y-encoder is encoders.CanEmb(1, C, E) -- an nn.Embedding over class labels -- forward and backward on the matrix cores (reference transformer.py:68-74):
 *     src[t, b, :] = Wx . x[t, b, :] + bx + (t < sep ? table[labels[t, b], :] : 0)
 * as ONE GEMM of A_aug [S B, Kp] = [x | onehot(label) on train rows | 0] against W_aug [E, Kp] = [Wx | table^T | 0], Kp = F + C rounded up to a multiple of 64,
 * the bias in the epilogue; the backward is the transposed GEMM dW_aug = d(src)^T . A_aug and a scatter of its columns.  x [S, B, F] f32 with strides x_st,
 * x_sb in elements (features contiguous), labels [S, B] int64 with strides l_st, l_sb; wx [E, F], bx [E], table [C, E] f32; src_sbe [S, B, E] f32 contiguous
 * (token t B + b): the src_sbe operand of pfn_stack_forward.  prec: a PFN_PREC_* value, the operand type both GEMMs run in.
 *   pfn_class_embed_workspace_bytes: what `workspace` must hold for this call shape (negative: an error code).
 *   pfn_class_embed_forward: writes src_sbe and leaves A_aug in the workspace.  status: NULL, or two int32 the kernels ADD to (the caller zeroes them):
 *     [0] train-row labels outside [0, C) -- such a row gets no class row (it equals the x-embedding) and gives the table no gradient, where torch's device
 *     assert would abort the process; [1] values of x, wx or table beyond +-65504 under PFN_PREC_FP16: they are stored as +-65504, as everywhere in the fp16
 *     path, and the caller is responsible for scaling inputs that large.  Labels of rows t >= sep are never read into the result.
 *   pfn_class_embed_backward: reads the A_aug the forward left (same call shape, same workspace, as for the stack's backward) and ACCUMULATES dwx [E, F] +=,
 *     dbx [E] +=, dtable [C, E] += (any of them NULL: skipped).  wx is accepted for a later input gradient and not read: no gradient reaches x.  Under
 *     PFN_PREC_FP16 d(src) is cast under a power-of-two scale taken on the device from max|d(src)| and the scatter multiplies it back out, exactly.
 *     flags bit 0: deterministic -- the weight-gradient GEMM runs without token splits, every gradient element has one writer, two runs are bit-equal.
 *     sep == 0: dtable is not touched.
 * Limits, checked before anything is launched: 1 <= F <= 1022, 1 <= C <= 1024, E >= 8 and E % 8 == 0, a PFN_PREC_* prec else PFN_ERR_UNSUPPORTED; B, S >= 0,
 * B S < 2^31, 0 <= sep <= S, non-NULL pointers, a workspace of at least the stated size else PFN_ERR_ARGUMENT; workspace, src_sbe, dsrc_sbe and bx 16-byte,
 * labels 8-byte, every other pointer 4-byte aligned else PFN_ERR_ALIGNMENT.  Every shape inside the limits runs in every precision (small or odd ones on the
 * 128 x 128 register-staged GEMMs).  B S == 0: PFN_OK, nothing launched.  Stream-ordered, no allocation, no host synchronisation. */
int64_t pfn_class_embed_workspace_bytes(int B, int S, int F, int E, int C, int prec);
int pfn_class_embed_forward(const float* x, int64_t x_st, int64_t x_sb, const int64_t* labels, int64_t l_st, int64_t l_sb, const float* wx, const float* bx,
                            const float* table, int B, int S, int F, int E, int C, int sep, int prec, int flags, void* workspace, int64_t workspace_bytes,
                            float* src_sbe, int32_t* status, void* stream);
int pfn_class_embed_backward(const float* dsrc_sbe, const float* wx, int B, int S, int F, int E, int C, int sep, int prec, int flags, void* workspace,
                             int64_t workspace_bytes, float* dwx, float* dbx, float* dtable, void* stream);

/* ---- single-op entry points (unit tests / profiling of individual kernels) --------------------
 * prec selects operand element type T: PFN_PREC_BF16 / PFN_PREC_FP16 (2 bytes) or PFN_PREC_F32; the LDS-DMA kernels (grouped weight gradients,
 * LayerNorm-fused GEMMs) take the two 16-bit formats only. */
int pfn_op_gemm_nt(const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K,
                   int flags, const float* bias, const void* aux, int64_t ld_aux,
                   const float* resid, int64_t ld_resid, float* out_f32, int64_t ld_out_f32,
                   void* out_t, int64_t ld_out_t, void* out2_t, int64_t ld_out2, int prec, void* stream);
int pfn_op_gemm_tn(const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc,
                   int M, int P, int Q, int atomic, int prec, void* stream);
/* grouped weight-gradient GEMMs (16-bit operands only): for i < n, C[i][P[i],Q[i]] += A[i][M,P[i]]^T . B[i][M,Q[i]] and, when
 * colsum && colsum[i], colsum[i][P[i]] += column sums of A[i]; one launch of 256x256 tiles.  The pointer / size
 * tables are HOST arrays.  splits: 0 automatic, 1 no split (deterministic, no atomics), > 1 token-axis splits.
 * P[i] and Q[i] must be multiples of 256 (PFN_ERR_UNSUPPORTED otherwise). */
int pfn_op_gemm_tn_group(int n, const void* const* A, const int64_t* lda, const void* const* B, const int64_t* ldb,
                         float* const* C, const int64_t* ldc, const int32_t* P, const int32_t* Q,
                         float* const* colsum, int M, int splits, int prec, void* stream);
/* fused linear + bias + residual + LayerNorm (16-bit operands, N in {128, 256, 512}, K % 32 == 0):
 *   v = A[M,K] . B[N,K]^T + bias + r;  y = v (f32);  mean / rstd of v per row;  x_t = bf16((v - mean) rstd gamma + beta)
 * r = resid[M,N] (f32) when resid != NULL, else the previous LayerNorm's output recomputed as
 * (ry - rmean) rrstd rgamma + rbeta.  Replaces `x = norm(x + dropout(sublayer(x)))` of torch's TransformerEncoderLayer
 * (nn/modules/transformer.py:952-957) for the out_proj and linear2 sublayers.
 * prec | PFN_OP_SUMS_16BIT (PFN_PREC_FP16 only): y is WRITTEN, and ry READ, in operand precision (the pointers then address fp16 rows) -- what the stack does for
 * fp16 models unless PFN_SCHED_F32_RESIDUAL is set; pfn_op_gemm_lnbwd takes the same flag for its y. */
#define PFN_OP_SUMS_16BIT 256
int pfn_op_gemm_ln(const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K, const float* bias,
                   const float* resid, const float* ry, const float* rmean, const float* rrstd,
                   const float* rgamma, const float* rbeta, const float* gamma, const float* beta, float eps,
                   float* y, float* mean, float* rstd, void* x_t, int prec, void* stream);
/* data-gradient GEMM + residual-branch gradient + the backward of the LayerNorm whose output gradient the sum is (16-bit
 * operands, N in {128, 256, 512}, K % 32 == 0):
 *   v = A[M,K] . B[N,K]^T + aux[M,N];   xhat = (y - mean) rstd;
 *   dx_t = bf16(rstd (gamma v - mean_n(gamma v) - xhat mean_n(gamma v xhat)));   dgamma += sum_m v xhat;   dbeta += sum_m v
 * i.e. autograd of `norm(x + sublayer(x))` (torch nn/modules/transformer.py:952-957) w.r.t. the norm's input, taking the
 * place of pfn_op_gemm_nt(EPI_RESID_T | EPI_OUT_T) followed by pfn_op_layernorm_bwd.  dgamma / dbeta accumulate atomically. */
int pfn_op_gemm_lnbwd(const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K, const void* aux,
                      const float* y, const float* mean, const float* rstd, const float* gamma,
                      void* dx_t, float* dgamma, float* dbeta, int prec, void* stream);
int pfn_op_attention_fwd(const void* qkv, void* ctx, float* lse, int B, int S, int E, int H, int sep,
                         int prec, void* stream);
/* Attention backward = three launches: delta = rowsum(dO * O); the key-block pass (dK, dV and dS^T into ds_ws); the
 * query-block pass (dQ from ds_ws, plus the self-key terms of the test rows).  ds_ws: pfn_op_attention_bwd_ws_bytes(B, S, H,
 * prec) bytes of scratch; delta_ws: 2 * B * H * S floats (the first launch leaves [delta | lse in log2 units] there).  parts: 0 = all, else a bit mask (1 delta, 2 key-block pass, 4 query-block pass) that lets bench.py
 * time every launch on its own; a partial run leaves the outputs of the skipped launches untouched.
 * sep == 0 (no train rows, no dropout): one launch instead, under the query-block bit -- dV = dO, dQ = dK = 0 exactly.  delta_ws is then NOT written (parts = 1
 * alone launches nothing): without keys no launch reads it. */
int64_t pfn_op_attention_bwd_ws_bytes(int B, int S, int H, int prec);
int pfn_op_attention_bwd(const void* qkv, const void* ctx, const float* lse, const void* dctx,
                         void* dqkv, float* delta_ws, void* ds_ws, int B, int S, int E, int H, int sep,
                         int prec, int parts, void* stream);
/* The same two with the queries below q_begin skipped (q_begin is rounded DOWN to a multiple of 256 = whole query blocks of every kernel): their
 * ctx / lse rows are not written; in the backward they add nothing to dK / dV and their dQ rows are zeros.  dctx must be zero in
 * [q_begin rounded down, first row that carries a gradient).  This is how the stack runs its TOP layer, whose train rows feed nothing
 * (the reference returns output[single_eval_pos:], transformer.py:91): q_begin = sep. */
int pfn_op_attention_fwd_from(const void* qkv, void* ctx, float* lse, int B, int S, int E, int H, int sep, int q_begin,
                              int prec, void* stream);
int pfn_op_attention_bwd_from(const void* qkv, const void* ctx, const float* lse, const void* dctx,
                              void* dqkv, float* delta_ws, void* ds_ws, int B, int S, int E, int H, int sep, int q_begin,
                              int prec, int parts, void* stream);
/* TEST ONLY: pfn_op_attention_fwd / pfn_op_attention_bwd with dropout on the attention probabilities, P' = P keep / (1 - p_drop), the way a training step with
 * dropout > 0 runs them.  drop_seed is the SITE seed of the layer's attention (what the stack derives from its call seed and the layer); the kernels mix the
 * (dataset, head) index b * H + h in themselves and regenerate keep(seed, query, key) from indices in every pass.  p_drop == 0 is exactly the pair above;
 * p_drop outside [0, 1) is PFN_ERR_ARGUMENT.  (ABI 10, additive: detect by symbol.) */
int pfn_op_attention_fwd_dropout(const void* qkv, void* ctx, float* lse, int B, int S, int E, int H, int sep,
                                 int prec, float p_drop, uint32_t drop_seed, void* stream);
int pfn_op_attention_bwd_dropout(const void* qkv, const void* ctx, const float* lse, const void* dctx,
                                 void* dqkv, float* delta_ws, void* ds_ws, int B, int S, int E, int H, int sep,
                                 int prec, int parts, float p_drop, uint32_t drop_seed, void* stream);
/* Rows of [B, S] token order <-> the decoder's compact test-row order [(S - sep), B] (row bytes a multiple of 4); the scatter
 * writes zeros into rows [zero_from, sep) and leaves rows below zero_from alone. */
int pfn_op_gather_rows(const void* src_bs, void* dst_tb, int B, int S, int64_t row_bytes, int sep, void* stream);
int pfn_op_scatter_rows(const void* src_tb, void* dst_bs, int B, int S, int64_t row_bytes, int sep, int zero_from, void* stream);
int pfn_op_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y_f32, void* y_t,
                         float* mean, float* rstd, int64_t rows, int E, float eps, int prec, void* stream);
/* dy: f32 when dy_is_t == 0, operand precision (prec) otherwise -- the form the backward schedule feeds it;
 * dx_f32 / dx_t may each be null. */
int pfn_op_layernorm_bwd(const void* dy, int dy_is_t, const float* x, const float* gamma, const float* mean,
                         const float* rstd, float* dx_f32, void* dx_t, float* dgamma, float* dbeta,
                         float* dbias_extra, int64_t rows, int E, int prec, void* stream);
int pfn_op_cast(const float* src, void* dst, int64_t n, int prec, void* stream);
/* The packed q|k|v projection of one encoder layer as the stack runs it (torch multi_head_attention_forward's in_proj: reference transformer.py:84):
 *   qkv[b, t, :] = x[b, t, :] . w_in^T + b_in,   x [B, S, E] T,  w_in [3E, E] T,  b_in [3E] f32,  qkv [B, S, 3E] T
 * and, when center != 0 (16-bit operands, E % 64 == 0), with the keys of every dataset centred before they are rounded (ABI 8, PFN_SCHED_NO_KEY_CENTERING clear):
 *   k'[b, t, :] = k[b, t, :] - W_k . xbar[b],   xbar[b] = mean of <= 64 evenly spaced rows t' = i * (sep_b / ns) (i < ns = min(64, sep_b)) of x[b, 0 : sep_b, :]
 * (sep_b = sep_of[b] when sep_of != NULL -- a device array -- else sep).  kshift_ws: B * E floats of scratch (receives W_k . xbar). */
int pfn_op_qkv_projection(const void* x_t, const void* w_in_t, const float* b_in, void* qkv_t, float* kshift_ws,
                          int B, int S, int E, int sep, const int32_t* sep_of, int center, int prec, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PFN_HIP_H */
