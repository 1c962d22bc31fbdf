// Weight-gradient GEMMs of the PFN encoder stack (gfx950): C[P,Q] (+)= A[M,P]^T . B[M,Q], contraction over the (long) token axis.
//   gemm_tn_kernel      : one product, 128 x 128 tiles, token splits with f32 atomics (templated over every operand type; the decoder / embedding shapes, f32 mode)
//   gemm_tn_big_kernel  : the GROUPED launch of all 4 L weight (and fused bias) gradients on 256 x 256 tiles (16-bit operands)
// Replaces autograd's dW = dY^T X of every nn.Linear of the stack (reference train.py:93; torch nn/modules/transformer.py:952-982).
#include <type_traits>
#include "pfn_device.h"
#include "pfn_kernels.h"

namespace pfn {

// (as in gemm.hip) XCD-aware, bijective remap of the linear workgroup id
PFN_DEV int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}
typedef __attribute__((address_space(1))) const void gvoid_t;
typedef __attribute__((address_space(3))) void lvoid_t;

// ---------------------------------------------------------------------------------------------
// C[P,Q] (+)= A[M,P]^T . B[M,Q]     contraction over the (long) token axis, split across
// workgroups in z; partial tiles are added with hardware f32 atomics.
// ---------------------------------------------------------------------------------------------
constexpr int TN_BMK = 32;  // token rows per LDS tile

template <typename T>
__global__ __launch_bounds__(256, 2) void gemm_tn_kernel(GemmTN g) {
  constexpr int RB = 128 * sizeof(T);  // 128 columns per tile row
  constexpr int TILE = TN_BMK * RB;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  LdsPtr smem = lds_cast(smem_raw);
  auto tileA = [&](int buf) { return smem + buf * 2 * TILE; };
  auto tileB = [&](int buf) { return smem + buf * 2 * TILE + TILE; };

  const int p0 = blockIdx.y * 128, q0 = blockIdx.x * 128;
  const int colsA = min(128, g.P - p0), colsB = min(128, g.Q - q0);
  const long mbeg = (long)blockIdx.z * g.m_chunk;
  const long mend = min((long)g.M, mbeg + g.m_chunk);
  if (mbeg >= mend) return;
  const T* A = reinterpret_cast<const T*>(g.A) + mbeg * g.lda + p0;
  const T* B = reinterpret_cast<const T*>(g.B) + mbeg * g.ldb + q0;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wp = wave >> 1, wq = wave & 1;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  TileStage<T, TN_BMK, RB, 256> sa, sb;
  const int rows_total = (int)(mend - mbeg);
  const int nt = (rows_total + TN_BMK - 1) / TN_BMK;
  // fused bias gradient: column sums of A (= dY) ride along in the workgroups of the first Q tile.
  // Every thread always stages the same 16-byte column chunk (256 % chunks-per-row == 0).
  const bool do_colsum = g.colsum != nullptr && blockIdx.x == 0;
  constexpr int EPC = 16 / sizeof(T);
  float csum[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) csum[e] = 0.f;
  auto add_colsum = [&]() {
    if (!do_colsum) return;
#pragma unroll
    for (int i = 0; i < sa.PER; ++i) {
      if constexpr (sizeof(T) == 2) {
        const X8<T> v = __builtin_bit_cast(X8<T>, sa.regs[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) csum[e] += (float)v[e];
      } else {
        const f32x4 v = __builtin_bit_cast(f32x4, sa.regs[i]);
#pragma unroll
        for (int e = 0; e < 4; ++e) csum[e] += v[e];
      }
    }
  };
  sa.issue(A, g.lda, rows_total, colsA);
  sb.issue(B, g.ldb, rows_total, colsB);
  add_colsum();
  sa.template commit<true>(tileA(0));
  sb.template commit<true>(tileB(0));
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) {
      const long r1 = (long)(t + 1) * TN_BMK;
      sa.issue(A + r1 * g.lda, g.lda, rows_total - (int)r1, colsA);
      sb.issue(B + r1 * g.ldb, g.ldb, rows_total - (int)r1, colsB);
      add_colsum();
    }
    const lds_char* ta = tileA(cur);
    const lds_char* tb = tileB(cur);
#pragma unroll
    for (int ks = 0; ks < TN_BMK; ks += 16) {
      Frag<T> fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = load_frag_tr<T, RB, 1>(ta, ks, wp * 64 + i * 32);
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = load_frag_tr<T, RB, 1>(tb, ks, wq * 64 + j * 32);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mma32(fa[i], fb[j], acc[i][j]);
    }
    if (t + 1 < nt) {
      sa.template commit<true>(tileA(cur ^ 1));
      sb.template commit<true>(tileB(cur ^ 1));
    }
    __syncthreads();
  }

  const float osc = loss_scale_down(g.scale_amax);      // fp16 backward: the gradient leaves unscaled (pfn_device.h)
  if (do_colsum) {
    // threads tid, tid+NCH, ... share a column chunk: reduce over the 256/NCH row groups through LDS
    constexpr int NCH = RB / 16;
    float* red = reinterpret_cast<float*>(smem_raw);  // all tiles are dead after the last barrier
#pragma unroll
    for (int e = 0; e < EPC; ++e) red[threadIdx.x * EPC + e] = csum[e];
    __syncthreads();
    if (threadIdx.x < NCH) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        float t = 0.f;
        for (int j = 0; j < 256 / NCH; ++j) t += red[(j * NCH + threadIdx.x) * EPC + e];
        const int col = p0 + threadIdx.x * EPC + e;
        if (col < g.P) unsafeAtomicAdd(g.colsum + col, t * loss_scale_down(g.scale_amax));
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int p = p0 + wp * 64 + i * 32 + acc_row(r, lane);
        const int q = q0 + wq * 64 + j * 32 + (lane & 31);
        if (p < g.P && q < g.Q) {
          float* c = g.C + (long)p * g.ldc + q;
          if (g.atomic) unsafeAtomicAdd(c, acc[i][j][r] * osc);
          else *c = acc[i][j][r] * osc;
        }
      }
}

// ---------------------------------------------------------------------------------------------
// gemm_tn_big_kernel: grouped weight-gradient GEMMs  C_g[P,Q] (+)= A_g[M,P]^T . B_g[M,Q]  (bf16).
//   One launch covers every weight gradient of the encoder stack (pfn_stack_backward keeps the
//   per-layer output-gradient operands resident and defers the weight gradients to one grouped
//   launch), so there are enough 256 x 256 output tiles to fill the chip WITHOUT splitting the
//   long token axis: no atomics, a deterministic summation order, plain read-modify-write of C.
//   (An optional split over tokens with f32 atomics stays available for small groups.)
//   * 256 x 256 tile, 64-token stages, 8 waves as 2 (P) x 4 (Q), each 128 x 64;
//   * both operands are token-major, so their LDS images are [token][256 columns] (512-byte rows)
//     filled by LDS-DMA and read through ds_read_b64_tr_b16; the 64-byte-unit XOR swizzle of
//     load_frag_tr is applied to the per-lane DMA source offset;
//   * operand staging (TnStager, shared with gemm_tn_wide_kernel): one buffer descriptor per operand and workgroup whose base is
//     the first token row of the stage requested next and whose num_records ends at the LAST ROW OF THE TOKEN SPLIT.  A lane's
//     byte offsets (token row of its piece x row pitch + swizzled column) are computed once in front of the loop; per stage only
//     the descriptor moves, in scalar registers (pfn_device.h dma_rsrc_advance).  Rows past the end of the split fail the range
//     check and arrive in LDS as zeros, for A and for B: a ragged last stage needs no clamp, no branch and no clearing pass.
//     The stage loop reads nothing from the problem table and multiplies no addresses (it used to: a scalar load with its wait,
//     sixteen 64-bit multiply-adds and the clamps per wave and stage, then a zero-fill loop with a second barrier for the tail);
//   * bias gradients (column sums of A) ride along as one extra MFMA against a constant ones
//     fragment in the workgroups of the first Q tile, split over the four Q waves.
// Requirements: P % 256 == 0, Q % 256 == 0, 16-byte aligned rows, row pitches of at least 256 elements, and -- the lane offsets and
// the descriptor's num_records are 32-bit -- token split rows x row pitch x 2 bytes <= 0x7ffffff0 for both operands
// (launch_gemm_tn_group answers PFN_ERR_UNSUPPORTED otherwise).
// ---------------------------------------------------------------------------------------------
// Stage depth / ring length: two stages of 64 tokens.  Measured at the north
// star (tools/bench_wgrad.py --batch 16) with the per-stage address arithmetic still in the loop: 64 x 2 950 us, 32 x 3 952, 32 x 4 965,
// 32 x 5 965; and again without it (--batch 32, profiles/wgrad_stage_issue.txt): 64 x 2 1566-1621 us, 32 x 3 1706-1716, 32 x 4 1743,
// 32 x 5 1730-1748 -- up to four stages in flight instead of one buy nothing either way: the operand stream is not bound by latency.
// The address arithmetic itself was 130 us of the 1734-1767 us the launch took with it, its position another 30: requested right behind
// the stage barrier the issue block (8 DMA instructions and 70 scalar ones) holds up the first fragment reads of all eight waves at once;
// behind the first 16-token step's MFMAs (the slot it fills is free from the barrier on) it runs under them.
constexpr int TNB_KT = 64;                       // tokens per stage
constexpr int TNB_NS = 2;                        // stages in LDS: one in flight under the one being multiplied
constexpr int TNB_TILE = TNB_KT * 512;           // bytes per operand per stage
constexpr int TNB_LDS = TNB_NS * 2 * TNB_TILE;
static_assert(TNB_LDS <= 160 * 1024, "weight-gradient stages do not fit the CU's LDS");
constexpr long TN_GROUP_MAX_SPLIT_BYTES = 0x7ffffff0L;      // token split rows x row pitch x 2 (TnStager's 32-bit byte range)

// Operand staging of the grouped kernels (NW waves; a 1-KiB DMA piece is 2 token rows x 512 B, wave w moves pieces w, w + NW, ... of each
// operand's stage).  16-bit operands.
template <int NW> struct TnStager {
  static constexpr int NP = TNB_KT / 2 / NW;      // pieces per wave per operand per stage
  DmaRsrc ra, rb;                                 // base: first row of the stage requested next; num_records: from there to the end of the split's last row
  unsigned a_lo, a_hi, b_lo, b_hi;                // the split's first row (where the profiling wrap goes back to)
  unsigned step_a, step_b;                        // bytes per stage
  int va[NP], vb[NP];                             // the lane's byte offset for each of its pieces
  int wave, srow, mask;                           // srow: token row (inside the split) of the stage requested next
  PFN_DEV void init(const TnProblem& pr, long mbeg, int rows, int p0, int q0, int wave_, int lane, int debug_mask) {
    const long lda2 = pr.lda * 2, ldb2 = pr.ldb * 2;
    ra = make_dma_rsrc(reinterpret_cast<const char*>(pr.A) + mbeg * lda2 + p0 * 2, (rows - 1) * lda2 + 512);
    rb = make_dma_rsrc(reinterpret_cast<const char*>(pr.B) + mbeg * ldb2 + q0 * 2, (rows - 1) * ldb2 + 512);
    a_lo = ra.w[0]; a_hi = ra.w[1]; b_lo = rb.w[0]; b_hi = rb.w[1];
    step_a = __builtin_amdgcn_readfirstlane((unsigned)(TNB_KT * lda2));
    step_b = __builtin_amdgcn_readfirstlane((unsigned)(TNB_KT * ldb2));
    wave = wave_; srow = 0; mask = debug_mask;
    const int row0 = wave * 2 + (lane >> 5);
    const int colb = ((((lane & 31) >> 2) ^ (row0 & 3)) * 32 + (lane & 3) * 8) * 2;      // 2 NW i = 0 mod 4: the swizzle is the same for every piece
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      va[i] = (row0 + 2 * NW * i) * (int)lda2 + colb;
      vb[i] = (row0 + 2 * NW * i) * (int)ldb2 + colb;
    }
  }
  // request the next stage into the ring slot at `slot` (A tile, then B tile), then move on by one stage
  PFN_DEV void issue(LdsPtr slot) {
    LdsPtr ta = slot + wave * 1024;
    LdsPtr tb = ta + TNB_TILE;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      // assembly form (pfn_device.h dma16): with the builtin hipcc waits vmcnt(0) in front of the first ds_read_b64_tr_b16 of
      // the stage being MULTIPLIED -- the intrinsic carries no address, so the DMA just issued for a LATER stage "may alias" --
      // and the copy never overlapped the MFMAs
      dma16(ra, ta + i * NW * 1024, va[i]);
      dma16(rb, tb + i * NW * 1024, vb[i]);
    }
    dma_rsrc_advance(ra, step_a);
    dma_rsrc_advance(rb, step_b);
    srow += TNB_KT;
    // profiling with cache-resident operands (GemmTNGroup::debug_mask = 2^k - 1 >= TNB_KT - 1): the stage row wraps, i.e. the bases go back to the
    // split's first row (num_records keeps counting down, so the ragged tail is still cut).  All ones otherwise: never taken.
    if ((srow & mask) == 0) { ra.w[0] = a_lo; ra.w[1] = a_hi; rb.w[0] = b_lo; rb.w[1] = b_hi; }
  }
};

template <typename T>
__global__ __launch_bounds__(512, 1) void gemm_tn_big_kernel(GemmTNGroup g) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  LdsPtr smem = lds_cast(smem_raw);

  const int ntiles = g.tile_start[g.n];
  const int id = xcd_remap(blockIdx.x, ntiles * g.splits);
  const int split = id / ntiles, tile = id % ntiles;
  int pi = 0;
  while (tile >= g.tile_start[pi + 1]) ++pi;
  const TnProblem& pr = g.p[pi];
  const int tq = pr.Q / 256;
  const int tl = tile - g.tile_start[pi];
  const int p0 = (tl / tq) * 256, q0 = (tl % tq) * 256;
  const long mbeg = (long)split * g.m_chunk;
  const long mend = min((long)g.M, mbeg + g.m_chunk);
  const int rows_total = (int)(mend - mbeg);
  if (rows_total <= 0) return;

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int wp = wave >> 2, wq = wave & 3;

  TnStager<8> stg;
  stg.init(pr, mbeg, rows_total, p0, q0, wave, lane, g.debug_mask);

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  f32x16 cs;
#pragma unroll
  for (int r = 0; r < 16; ++r) cs[r] = 0.f;
  const bool do_colsum = pr.colsum != nullptr && q0 == 0;
  Frag<T> ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones.v[e] = (T)1.0f;

  const int nt = (rows_total + TNB_KT - 1) / TNB_KT;
  // Two stages: stage t is multiplied while stage t+1 is requested into the slot stage t-1 has just released.  Nothing younger than
  // stage t is in flight when it is wanted, so "stage t has landed" is vmcnt(0) -- explicit s_waitcnt + raw s_barrier (wait_vm_barrier).
  // (Touching later stages' lines to pull them into L2 instead made the launch slower: 916 us without, 990 / 1030 / 1070 us
  // touching 2 / 3 / 5 stages ahead.)
#pragma unroll
  for (int st = 0; st < TNB_NS - 1; ++st)      // (the one stage requested ahead of the loop)
    if (st < nt) stg.issue(smem + st * 2 * TNB_TILE);
  // the main loop exists twice (with / without the bias-gradient MFMA) so neither carries a branch.  (Captures by name, in this order: the order is
  // the closure's layout, and hipcc's scalar register assignment in the loop follows it.)
  auto main_loop = [&nt, &stg, &smem, &wq, &wp, &acc, &cs, &ones](auto with_colsum) {
    constexpr bool CS = decltype(with_colsum)::value;
    int slot = 0, slot_next = 1;
    for (int t = 0; t < nt; ++t) {
      wait_vm_barrier<0>();
      const bool more = t + 1 < nt;
      LdsPtr ta = smem + slot * 2 * TNB_TILE;
      LdsPtr tb = ta + TNB_TILE;
#pragma unroll
      for (int ks = 0; ks < TNB_KT; ks += 16) {
        Frag<T> fa[4], fb[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j] = load_frag_tr<T, 512, 1>(tb, ks, wq * 64 + j * 32);
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[i] = load_frag_tr<T, 512, 1>(ta, ks, wp * 128 + i * 32);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = mma32(fa[i], fb[j], acc[i][j]);
        // bias gradient: Q wave wq sums the columns of P sub-tile wq (one more fragment read, one more MFMA)
        if constexpr (CS) cs = mma32(load_frag_tr<T, 512, 1>(ta, ks, wp * 128 + wq * 32), ones, cs);
        if (ks == 0) {      // the other slot is free from the stage barrier on: the issue block goes under the first step's MFMAs
          PFN_PIN_LDS_MFMA();
          if (more) stg.issue(smem + slot_next * 2 * TNB_TILE);
          PFN_PIN_LDS_MFMA();
        }
      }
      slot_next = slot;
      slot = slot + 1 == TNB_NS ? 0 : slot + 1;
    }
  };
  if (do_colsum) main_loop(std::true_type{});
  else main_loop(std::false_type{});

  const int pv = pr.Pv > 0 ? pr.Pv : pr.P;    // rows of C that exist (A may end in zero-padding columns)
  const float osc = loss_scale_down(g.scale_amax);      // fp16 backward: the gradients leave unscaled (pfn_device.h)
  if (do_colsum && (lane & 31) == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int pp = p0 + wp * 128 + wq * 32 + acc_row(r, lane);
      if (pp < pv) unsafeAtomicAdd(pr.colsum + pp, cs[r] * osc);
    }
  }
  // always atomic: token splits add into the same tile, and concurrent backward passes (micro-batches on several
  // HIP streams, streams.py) accumulate into the same gradient buffer
  const bool atomic = true;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int pp = p0 + wp * 128 + i * 32 + acc_row(r, lane);
        const int qq = q0 + wq * 64 + j * 32 + (lane & 31);
        float* c = pr.C + (long)pp * pr.ldc + qq;
        if (pp >= pv) continue;
        if (atomic) unsafeAtomicAdd(c, acc[i][j][r] * osc);
        else *c += acc[i][j][r] * osc;
      }
}

// ---------------------------------------------------------------------------------------------
// gemm_tn_wide_kernel (round 6): the same grouped product on the same 256 x 256 tile with FOUR waves of 128 x 128 instead of eight of 128 x 64.
// Why: both operands are token-major, so every fragment is a transposing LDS read of 8 bytes per lane (ds_read_b64_tr_b16) -- 12 of them per 8 MFMAs in the 8-wave
// shape.  Counted per CU and 16-token step that is 96 LDS read instructions + the DMA's own 16 KiB of LDS writes against 512 cycles of MFMA per SIMD: the LDS port,
// not the matrix pipe, is what the 8-wave kernel runs at (838 TF/s = a third of the MFMA rate, whatever the depth of the operand ring: gemm_tn_big_kernel's header).
// A wave that owns 128 x 128 reads (128 + 128) columns for twice the MFMAs: 64 read instructions per CU and step, a third less LDS traffic per flop.
// Price: the 16 accumulator tiles are 256 registers, so a wave needs the whole register file (one wave per SIMD: no second wave to cover its LDS round trips) --
// the fragments of step s + 1 are therefore requested before the MFMAs of step s (two fragment sets, PFN_PIN_LDS_MFMA keeps the machine scheduler from sinking the
// reads back to their consumers), the first step of the next stage right behind the stage barrier.
// With the staging of gemm_tn_big_kernel (TnStager; the clamp and the 64-bit multiply per piece were in this loop too): 1977-1985 us against 2014-2041 us at the
// north star's 64 000 tokens, against 1566-1621 us of the eight-wave kernel (profiles/wgrad_stage_issue.txt): eight waves stay the default.
// ---------------------------------------------------------------------------------------------
constexpr int TNW_NW = 4;                              // waves: 2 (P) x 2 (Q), each 128 x 128
template <typename T>
__global__ __launch_bounds__(TNW_NW * 64, 1) void gemm_tn_wide_kernel(GemmTNGroup g) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  LdsPtr smem = lds_cast(smem_raw);
  const int ntiles = g.tile_start[g.n];
  const int id = xcd_remap(blockIdx.x, ntiles * g.splits);
  const int split = id / ntiles, tile = id % ntiles;
  int pi = 0;
  while (tile >= g.tile_start[pi + 1]) ++pi;
  const TnProblem& pr = g.p[pi];
  const int tq = pr.Q / 256;
  const int tl = tile - g.tile_start[pi];
  const int p0 = (tl / tq) * 256, q0 = (tl % tq) * 256;
  const long mbeg = (long)split * g.m_chunk;
  const long mend = min((long)g.M, mbeg + g.m_chunk);
  const int rows_total = (int)(mend - mbeg);
  if (rows_total <= 0) return;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int wp = wave >> 1, wq = wave & 1;

  TnStager<TNW_NW> stg;      // the staging of gemm_tn_big_kernel: loop-invariant lane offsets, the descriptors advance per stage, the ragged tail arrives as zeros
  stg.init(pr, mbeg, rows_total, p0, q0, wave, lane, g.debug_mask);

  f32x16 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  // bias gradient (column sums of A over the tokens): on the vector ALU, straight from the A fragments the products read anyway -- lane l holds 8 tokens of column
  // l & 31 of each of its 4 sub-tiles; Q wave wq sums sub-tiles 2 wq and 2 wq + 1 (64 adds per step under 512 cycles of MFMA; two more accumulator tiles do not fit)
  float cs[2] = {0.f, 0.f};
  const bool do_colsum = pr.colsum != nullptr && q0 == 0;

  const int nt = (rows_total + TNB_KT - 1) / TNB_KT;
  struct Frs { Frag<T> a[4], b[4]; };
  auto main_loop = [&](auto with_colsum) {
    constexpr bool CS = decltype(with_colsum)::value;
    Frs f0, f1;
    auto ld = [&](Frs& f, const lds_char* ta, const lds_char* tb, int ks) {
#pragma unroll
      for (int j = 0; j < 4; ++j) f.b[j] = load_frag_tr<T, 512, 1>(tb, ks, wq * 128 + j * 32);
#pragma unroll
      for (int i = 0; i < 4; ++i) f.a[i] = load_frag_tr<T, 512, 1>(ta, ks, wp * 128 + i * 32);
    };
    auto mm = [&](const Frs& f) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mma32(f.a[i], f.b[j], acc[i][j]);
      // bias gradient: Q wave wq sums the columns of the wave's P sub-tiles 2 wq and 2 wq + 1 (their fragments are in registers already)
      if constexpr (CS) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int e = 0; e < 8; ++e) cs[c] += (float)(wq ? f.a[2 + c] : f.a[c]).v[e];
      }
    };
    // stage t has landed for every wave and every read of the slot it is about to overwrite has retired (wait_vm_barrier waits lgkmcnt(0) too);
    // request stage t + 1 into the other slot
    auto enter_stage = [&](int t, int slot) {
      wait_vm_barrier<0>();
      if (t + 1 < nt) stg.issue(smem + (slot ^ 1) * 2 * TNB_TILE);
    };
    int slot = 0;
    enter_stage(0, slot);
    ld(f0, smem, smem + TNB_TILE, 0);
    for (int t = 0; t < nt; ++t) {
      const lds_char* ta = smem + slot * 2 * TNB_TILE;
      const lds_char* tb = ta + TNB_TILE;
      ld(f1, ta, tb, 16);
      PFN_PIN_LDS_MFMA();
      mm(f0);
      PFN_PIN_LDS_MFMA();
      ld(f0, ta, tb, 32);
      PFN_PIN_LDS_MFMA();
      mm(f1);
      PFN_PIN_LDS_MFMA();
      ld(f1, ta, tb, 48);
      PFN_PIN_LDS_MFMA();
      mm(f0);
      PFN_PIN_LDS_MFMA();
      slot ^= 1;
      if (t + 1 < nt) {
        enter_stage(t + 1, slot);
        const lds_char* tan = smem + slot * 2 * TNB_TILE;
        ld(f0, tan, tan + TNB_TILE, 0);
      }
      PFN_PIN_LDS_MFMA();
      mm(f1);
      PFN_PIN_LDS_MFMA();
    }
  };
  stg.issue(smem);
  if (do_colsum) main_loop(std::true_type{});
  else main_loop(std::false_type{});

  const int pv = pr.Pv > 0 ? pr.Pv : pr.P;
  const float osc = loss_scale_down(g.scale_amax);
  if (do_colsum) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float s = cs[c] + __shfl_xor(cs[c], 32, 64);      // the two half-waves hold the other 8 tokens of every step
      const int pp = p0 + wp * 128 + (2 * wq + c) * 32 + (lane & 31);
      if (lane < 32 && pp < pv) unsafeAtomicAdd(pr.colsum + pp, s * osc);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int pp = p0 + wp * 128 + i * 32 + acc_row(r, lane);
        const int qq = q0 + wq * 128 + j * 32 + (lane & 31);
        if (pp < pv) unsafeAtomicAdd(pr.C + (long)pp * pr.ldc + qq, acc[i][j][r] * osc);
      }
}

// ---------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int g_tn_debug_wrap = 0;
void set_gemm_tn_debug_wrap(int rows) { g_tn_debug_wrap = rows; }
static bool g_tn_wide = false;
void set_gemm_tn_group_waves(int waves) { g_tn_wide = waves == 4; }

int launch_gemm_tn(GemmTN g, int precision, hipStream_t stream) {
  if (g.M <= 0 || g.P <= 0 || g.Q <= 0) return PFN_OK;
  const size_t es = prec_esize(precision);
  if ((g.lda * es) % 16 || (g.ldb * es) % 16 || !aligned16(g.A) || !aligned16(g.B)) return PFN_ERR_ALIGNMENT;
  const int tp = (g.P + 127) / 128, tq = (g.Q + 127) / 128;
  int splits = (1024 + tp * tq - 1) / (tp * tq);
  const int max_splits = (g.M + 4 * TN_BMK - 1) / (4 * TN_BMK);
  if (splits > max_splits) splits = max_splits;
  if (g.max_splits > 0 && splits > g.max_splits) splits = g.max_splits;
  if (splits < 1) splits = 1;
  if (!g.atomic) splits = 1;
  int chunk = (g.M + splits - 1) / splits;
  chunk = (chunk + TN_BMK - 1) / TN_BMK * TN_BMK;
  splits = (g.M + chunk - 1) / chunk;
  g.m_chunk = chunk;
  const size_t lds = 4 * TN_BMK * 128 * es;
  PFN_DISPATCH_OP(precision, hipLaunchKernelGGL(gemm_tn_kernel<T>, dim3(tq, tp, splits), dim3(256), lds, stream, g));
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

bool gemm_tn_group_supported(const TnProblem& p) {
  return p.P % 256 == 0 && p.Q % 256 == 0 && (p.lda * 2) % 16 == 0 && (p.ldb * 2) % 16 == 0 && aligned16(p.A) && aligned16(p.B);
}

int launch_gemm_tn_group(GemmTNGroup g, int precision, hipStream_t stream) {
  if (g.n <= 0 || g.M <= 0) return PFN_OK;
  if (g.n > TN_GROUP_MAX) return PFN_ERR_ARGUMENT;
  if (!prec_is16(precision)) return PFN_ERR_UNSUPPORTED;
  int tiles = 0;
  for (int i = 0; i < g.n; ++i) {
    if (!gemm_tn_group_supported(g.p[i])) return PFN_ERR_UNSUPPORTED;
    g.tile_start[i] = tiles;
    tiles += (g.p[i].P / 256) * (g.p[i].Q / 256);
  }
  g.tile_start[g.n] = tiles;
  // split the token axis only when the group cannot occupy the chip by itself
  // automatic: the smallest split count (<= 8) whose workgroup count fills whole rounds of the 256 CUs to >= 90 %
  int splits = g.splits;
  if (splits <= 0) {
    splits = 8;
    for (int sp = 1; sp <= 8; ++sp) {   // (a 256 x 256 partial tile is 65536 atomics: more than 8 splits cost more than they fill)
      const int blocks = tiles * sp, rounds = (blocks + 255) / 256;
      if (blocks >= 0.9 * rounds * 256) { splits = sp; break; }
    }
  }
  const int max_splits = (g.M + 4 * TNB_KT - 1) / (4 * TNB_KT);
  if (splits > max_splits) splits = max_splits;
  int chunk = (g.M + splits - 1) / splits;
  chunk = (chunk + TNB_KT - 1) / TNB_KT * TNB_KT;
  splits = (g.M + chunk - 1) / chunk;
  g.splits = splits;
  g.m_chunk = chunk;
  // TnStager: 32-bit lane offsets and num_records, and a row pitch that keeps the row behind the split's last one out of range
  for (int i = 0; i < g.n; ++i) {
    const TnProblem& p = g.p[i];
    if (p.lda < 256 || p.ldb < 256 || (long)chunk * p.lda * 2 > TN_GROUP_MAX_SPLIT_BYTES || (long)chunk * p.ldb * 2 > TN_GROUP_MAX_SPLIT_BYTES) return PFN_ERR_UNSUPPORTED;
  }
  // PFN_TUNE_GEMM_TN_WRAP: a power of two >= TNB_KT wraps the stage row; anything else leaves the wrap off
  const int wrap = g_tn_debug_wrap;
  g.debug_mask = wrap >= TNB_KT && (wrap & (wrap - 1)) == 0 ? wrap - 1 : 0x7fffffff;
  if (g_tn_wide) {      // PFN_TUNE_WGRAD_WAVES = 4: four waves of 128 x 128 (gemm_tn_wide_kernel)
    static LdsAllowance allow_w[2];
    if (precision == PFN_PREC_FP16) {
      allow_w[1].ensure(gemm_tn_wide_kernel<f16>, TNB_LDS);
      hipLaunchKernelGGL(gemm_tn_wide_kernel<f16>, dim3(tiles * splits), dim3(TNW_NW * 64), TNB_LDS, stream, g);
    } else {
      allow_w[0].ensure(gemm_tn_wide_kernel<bf16>, TNB_LDS);
      hipLaunchKernelGGL(gemm_tn_wide_kernel<bf16>, dim3(tiles * splits), dim3(TNW_NW * 64), TNB_LDS, stream, g);
    }
    return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
  }
  static LdsAllowance allowance[2];
  if (precision == PFN_PREC_FP16) {
    allowance[1].ensure(gemm_tn_big_kernel<f16>, TNB_LDS);
    hipLaunchKernelGGL(gemm_tn_big_kernel<f16>, dim3(tiles * splits), dim3(512), TNB_LDS, stream, g);
  } else {
    allowance[0].ensure(gemm_tn_big_kernel<bf16>, TNB_LDS);
    hipLaunchKernelGGL(gemm_tn_big_kernel<bf16>, dim3(tiles * splits), dim3(512), TNB_LDS, stream, g);
  }
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

}  // namespace pfn
