// Fused QK^T -> masked online softmax -> PV ("flash") attention for the PFN eval-position mask,
// forward and backward, on gfx950 MFMA.
//
// Replaces the scores/softmax/PV part of torch multi_head_attention_forward as called from
// nn.TransformerEncoderLayer inside TransformerModel.forward (reference transformer.py:84) with the
// additive mask of TransformerModel.generate_D_q_matrix (transformer.py:34-41):
//     query i may attend key j   iff   j < sep   or   j == i
// The [S,S] mask is never built: the kernels stream key tiles over [0, sep) and treat the
// "self" key of a test row (i >= sep) as the initial state of the online softmax (forward) or
// as a row-wise correction term (backward).
//
// Formulation (all MFMAs are 32x32, "swapped" so softmax statistics are lane-local):
//   fwd kernel       : lane <-> query.   S^T = K.Q^T, O^T = V^T.P^T
//   bwd key pass     : lane <-> key.     S = Q.K^T, dP = dO.V^T, dV^T = dO^T.P, dK^T = Q^T.dS;  stores dS^T
//   bwd query pass   : lane <-> query.   dQ^T = K^T.dS^T  (dS^T read back)
// Operands that are k-major in memory (V, K^T, Q^T, dO^T) come from LDS through
// ds_read_b64_tr_b16 (bf16) in the accumulator-order slot mapping M2, so P / dS never move
// between lanes.
#include <algorithm>
#include <type_traits>
#include "pfn_device.h"
#include "pfn_kernels.h"

namespace pfn {

template <typename T, int D> struct AttnCfg {
  static constexpr int RB = D * (int)sizeof(T);              // bytes per K/V/Q row of one head
  static constexpr int KVB = (sizeof(T) == 2 && D <= 128) ? 64 : 32;  // keys per LDS tile
  static constexpr int NKB = KVB / 32;
  static constexpr int NKK = D / 16;
  static constexpr int NDB = D / 32;
  static constexpr int TILE = KVB * RB;
  static constexpr int RS = PadStride<RB>::ROW, CS = PadStride<RB>::COL;   // padded LDS row strides (pfn_device.h)
  static constexpr int RIMG = KVB * RS, CIMG = KVB * CS;                  // bytes of one row / col image of a tile
  // bf16 up to head dim 128 (product path): 8 waves share every K/V (or Q/dO) tile and the kernel is held to 256
  // registers, so two waves are resident per SIMD and one wave's MFMAs cover the other's softmax / LDS waits.
  // Head dim 256 and the exact-f32 parity mode have twice the accumulator / fragment registers and keep 4 waves
  // with the whole register file (at 256 registers they spill into scratch inside the tile loop).
  static constexpr int NW = (sizeof(T) == 2 && D <= 128) ? 8 : 4;
  static constexpr int NT = NW * 64;        // threads per workgroup
  static constexpr int QBLK = NW * 32;      // query (or key) rows per workgroup
};

template <typename T> PFN_DEV Frag<T> load_frag_global(const T* p) {
  Frag<T> f;
  if constexpr (sizeof(T) == 2) {
    f.v = *reinterpret_cast<const X8<T>*>(p);
  } else {
    f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { f.v[e] = a[e]; f.v[4 + e] = b[e]; }
  }
  return f;
}
template <typename T> PFN_DEV void store_frag_global(T* p, const float (&x)[8]) {
  if constexpr (sizeof(T) == 2) {
    X8<T> v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (T)x[e];
    *reinterpret_cast<X8<T>*>(p) = v;
  } else {
    f32x4 a, b;
#pragma unroll
    for (int e = 0; e < 4; ++e) { a[e] = x[e]; b[e] = x[4 + e]; }
    *reinterpret_cast<f32x4*>(p) = a;
    *reinterpret_cast<f32x4*>(p + 4) = b;
  }
}
template <typename T> PFN_DEV float frag_get(const Frag<T>& f, int e) { return (float)f.v[e]; }
// the same value read out of the PACKED registers: element e of a bf16 fragment is the low (e even) or high half of dword e / 2
template <typename T> PFN_DEV float frag_get_bits(const Frag<T>& f, int e) {
  if constexpr (std::is_same<T, f16>::value) {
    return (float)f.v[e];      // v_cvt_f32_f16 (the high half through SDWA): one instruction as well
  } else if constexpr (sizeof(T) == 2) {
    const unsigned w = __builtin_bit_cast(u32x4, f.v)[e >> 1];
    return __builtin_bit_cast(float, (e & 1) ? (w & 0xffff0000u) : (w << 16));
  } else return f.v[e];
}
template <typename T> PFN_DEV float dot8(const Frag<T>& a, const Frag<T>& b) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) s += frag_get(a, e) * frag_get(b, e);
  return s;
}
template <typename T> PFN_DEV f32x4 load4(const T* p) {
  f32x4 r;
  if constexpr (sizeof(T) == 2) {
    X4<T> v = *reinterpret_cast<const X4<T>*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (float)v[e];
  } else r = *reinterpret_cast<const f32x4*>(p);
  return r;
}
template <typename T> PFN_DEV void store4(T* p, f32x4 x) {
  if constexpr (sizeof(T) == 2) {
    X4<T> v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (T)x[e];
    *reinterpret_cast<X4<T>*>(p) = v;
  } else *reinterpret_cast<f32x4*>(p) = x;
}
PFN_DEV float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// Workgroup -> (row block, head, dataset) for a 1-D launch of nblk * H * B workgroups.  Hardware deals
// consecutive workgroup ids round-robin over the 8 XCDs (each with a private L2); every row block of one
// (dataset, head) streams the SAME K/V (or Q/dO) rows, so the ids are remapped (bijectively, as in gemm.hip) to
// give each XCD whole (dataset, head) groups: the operand rows are then fetched into one L2 once instead of
// into all eight.
struct AttnBlock { int blk, hd, b; };
PFN_DEV AttnBlock attn_block(int nblk, int H) {
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
  const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  AttnBlock o;
  o.blk = id % nblk;
  const int bh = id / nblk;
  o.hd = bh % H;
  o.b = bh / H;
  return o;
}

// The same for the key-block pass, whose LAST block of every (dataset, head) pair is ragged (sep mod 256 keys; its dead waves skip
// the tile work) and therefore cheap: every XCD gets its share of the full blocks first (block index fastest inside a pair, so a
// pair's blocks still run together on one L2) and its share of the ragged blocks last -- longest first.  At the north-star
// micro-batch (32 datasets x 4 heads, sep 1604: 6 full blocks + 68 keys) the full blocks are exactly 3 rounds of 256 workgroups
// and the fourth round holds only the cheap ones, instead of four rounds of mixed work.
PFN_DEV AttnBlock attn_block_ragged_last(int nblk, int nfull, int H) {
  if (nfull == nblk) return attn_block(nblk, H);
  const int nwg = gridDim.x, bid = blockIdx.x, npairs = nwg / nblk;
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, j = bid >> 3;
  const int n_x = q + (xcd < r ? 1 : 0);                                  // workgroups of this XCD (hardware round-robin)
  const int first = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q; // workgroups of the XCDs before this one
  const int r_lo = (int)((long)first * npairs / nwg), r_hi = (int)((long)(first + n_x) * npairs / nwg);   // its ragged blocks: pairs [r_lo, r_hi)
  const int f_x = n_x - (r_hi - r_lo);
  const int f_off = first - r_lo;                                         // full blocks handed to the XCDs before this one
  AttnBlock o;
  int pair;
  if (j < f_x) { const int id = f_off + j; pair = id / nfull; o.blk = id % nfull; }
  else { pair = r_lo + (j - f_x); o.blk = nfull; }
  o.hd = pair % H;
  o.b = pair / H;
  return o;
}

typedef __attribute__((address_space(3))) void lvoid_t;
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr float RESCALE_THR = 6.f;  // log2 units: lazily raised running max of the online softmax (see attn_fwd_kernel)

// Predict against a K / V cache whose datasets hold DIFFERENT numbers of train rows (pfn_stack_*_ragged): sep_of [B] on the device, `sep` the context's rows per
// dataset (the longest one; the launch geometry is sized for it).  The count is clamped to [0, sep], so no value behind the pointer can carry a read outside the
// context; it is one scalar load per workgroup (b comes from the block index).  nullptr = every dataset at `sep` (the uniform calls: nothing changes for them).
PFN_DEV int cache_sep(const int* sep_of, int b, int sep) { return sep_of ? min(max(sep_of[b], 0), sep) : sep; }
// EMPTY SPLITS: a split z > 0 whose key range starts at or beyond its dataset's last key writes NOTHING (it returns ahead of every barrier), and the merge kernels
// read the first cache_live_splits partials of a dataset only -- split 0 always exists (it holds the self key), so no row is ever empty.
PFN_DEV int cache_live_splits(const int* sep_of, int b, int sep, int split_keys, int nsplit) {
  return sep_of ? max(1, min(nsplit, (cache_sep(sep_of, b, sep) + split_keys - 1) / split_keys)) : nsplit;
}

// =============================================================================================
// forward
// =============================================================================================
// DV < D (exact-f32 kernels at head dim 256, inference): the head dimension of V / O is split over gridDim.y workgroups, each of which
// forms the whole score row (Q.K over all D columns) and the D / gridDim.y output columns [blockIdx.y * DV, + DV) -- a full f32 K tile
// and a full V tile of 256 columns do not fit the LDS side by side (2 x 33 KB + 4 x 34 KB), a K tile and a half V tile do.  The softmax
// statistics are recomputed per slice (identical values; slice 0 writes lse).  1.5 x the matrix work of an unsplit kernel, for a pass
// that is not the throughput path (reference transformer.py:55-91 under model.eval(), priors/fast_gp_mix.py:139-153 validate).
// A 32 x 32 accumulator tile whose ROWS are the contraction index of the next product (rows acc_row(r) = accumulator order, lane = column) as the operand fragment of
// contraction chunk c (rows 16 c .. 16 c + 15) in MEMORY order (mapping M1: slot (h, e) = row 16 c + 8 h + e): the half-waves exchange their middle quads
// (v_permlane32_swap, as store_row_block does for its 16-byte stores), `add8` is added in f32 first (add8[4 g + e] belongs to row 16 c + 8 g + 4 h + e).
template <typename T> PFN_DEV Frag<T> acc_to_frag_m1(const f32x16& acc, int c, const float (&add8)[8]) {
  static_assert(sizeof(T) == 2, "16-bit operands");
  typedef X2<T> x2;
  const x2 a0 = {(T)(acc[8 * c + 0] + add8[0]), (T)(acc[8 * c + 1] + add8[1])}, a1 = {(T)(acc[8 * c + 2] + add8[2]), (T)(acc[8 * c + 3] + add8[3])};
  const x2 b0 = {(T)(acc[8 * c + 4] + add8[4]), (T)(acc[8 * c + 5] + add8[5])}, b1 = {(T)(acc[8 * c + 6] + add8[6]), (T)(acc[8 * c + 7] + add8[7])};
  const auto r0 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a0), __builtin_bit_cast(unsigned, b0), false, false);
  const auto r1 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a1), __builtin_bit_cast(unsigned, b1), false, false);
  const u32x4 w = {r0[0], r1[0], r0[1], r1[1]};
  Frag<T> f;
  f.v = __builtin_bit_cast(X8<T>, w);
  return f;
}

// FUSEQ (AttnArgs::xq): the workgroup's Q slice is formed here instead of read from qkv -- see AttnArgs.  Q^T[d][query] = W_q[h] x^T as "swapped" MFMAs (A = 32 rows
// of W_q[h], B = the wave's 32 x rows), so a lane ends up with its own query's 128 values, 16 per accumulator tile in accumulator order; acc_to_frag_m1 turns them
// into the very fragments the K.Q^T product wants.  W_q[h] ([D, E], 128 KB at emsize 512) goes through the K / V tile buffers (not yet in use) in chunks of 128
// columns, double-buffered; the x rows come straight from global memory, 16 bytes per lane and k-step (whole 1-KiB rows over the prologue).
// CACHE (AttnArgs::kv; launch_attn_fwd_cache): the queries are S = n test rows whose keys [0, sep) were cached by pfn_stack_condition.  The key tiles stream from the
// context instead of qkv, every query is a test row (its own key / value from qkv is the initial state), and with gridDim.z > 1 the workgroup streams only its split
// of the keys -- the self key in split 0 -- and leaves unnormalised (o, m, l) for attn_merge_kernel.
template <typename T, int D, bool DROP = false, int DV = D, bool FUSEQ = false, bool CACHE = false>
__global__ __launch_bounds__((AttnCfg<T, D>::NT)) void attn_fwd_kernel(AttnArgs a) {
  static_assert(!CACHE || (!DROP && !FUSEQ), "predict against a cache: no dropout, Q from qkv");
  operand_store_mode<T>();
  using C = AttnCfg<T, D>;
  using CV = AttnCfg<T, DV>;      // the V / O side: CV::NDB column blocks, CV::CIMG bytes per tile image
  static_assert(C::KVB == CV::KVB && D % DV == 0, "V slices share the K tile's key count");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  LdsPtr smem = lds_cast(smem_raw);
  // two K buffers (row images) followed by four V buffers (col images): P.V runs one tile behind Q.K (below), and with the
  // ping-pong schedule half of the waves run another half tile behind the others
  auto Kt = [&](int buf) { return smem + buf * C::RIMG; };
  auto Vt = [&](int buf) { return smem + 2 * C::RIMG + buf * CV::CIMG; };
  constexpr int NVB = 4;
  const int vcol0 = DV == D ? 0 : (int)blockIdx.y * DV;      // first V / O column of this workgroup inside the head

  AttnBlock wg = attn_block((a.S + C::QBLK - 1) / C::QBLK - a.q_begin / C::QBLK, a.H);
  wg.blk += a.q_begin / C::QBLK;      // (q_begin: a multiple of 256, i.e. whole query blocks)
  const int b = wg.b, hd = wg.hd;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, li = lane & 31;
  // PING-PONG (8-wave configurations): a SIMD holds waves w and w + 4.  With one barrier at the end of every tile all eight waves
  // run in lock-step -- both waves of a SIMD issue their 16 Q.K MFMAs together (vector ALU idle) and then their exponentials together
  // (the matrix pipe has only the P.V MFMAs to chew on).  The per-wave instruction sequence stays what it is; waves 4..7 merely take
  // their one barrier per tile BETWEEN the Q.K half and the softmax / P.V half instead of after it, so they run half a tile behind
  // waves 0..3 and one wave's MFMA-only half overlaps the other's vector-heavy half.  LDS cost: a fourth V buffer (tile t-1 is
  // still being read by the lagging waves while tile t+2 is being written).
  const int lag = (C::NW == 8 && (a.pingpong & 1)) ? (wave >> 2) : 0;
  const long rs = 3L * a.E;
  const T* base = reinterpret_cast<const T*>(a.qkv) + (long)b * a.S * rs;
  const T* Qp = base + hd * D;
  const T* Kp = base + a.E + hd * D;
  const T* Vp = base + 2 * a.E + hd * D + vcol0;
  const int qi = wg.blk * C::QBLK + wave * 32 + li;
  const bool qvalid = qi < a.S;
  const int qc = min(qi, a.S - 1);
  // keys streamed by this workgroup: [0, sep) of qkv, or (CACHE) `sep` keys of the context from k_lo on
  const int k_lo = CACHE ? (int)blockIdx.z * a.split_keys : 0;
  const int sep = CACHE ? min(cache_sep(a.sep_of, b, a.sep) - k_lo, a.split_keys) : a.sep_of ? a.sep_of[b] : a.sep;      // (wave-uniform: b comes from the block index)
  if constexpr (CACHE) { if (blockIdx.z > 0 && sep <= 0) return; }      // ragged context: an empty split (cache_live_splits), ahead of every barrier and LDS access
  const long kld = CACHE ? a.kv_ld : rs;
  const T* Ksrc = CACHE ? reinterpret_cast<const T*>(a.kv) + b * a.kv_sb + k_lo * kld + hd * D : Kp;
  const T* Vsrc = CACHE ? Ksrc + a.E + vcol0 : Vp;
  if (a.q_from_sep && (wg.blk + 1) * C::QBLK <= sep / 256 * 256) return;      // ragged batch, top layer: this dataset's queries start above the block (ahead of every barrier)
  const float scale_log2 = rsqrtf((float)D) * LOG2E;
  // DROP: dropout on the probabilities (pfn_device.h dropout_keep with i = query, j = key).  The normaliser (row sum, lse) is that of
  // the UNMASKED softmax -- torch drops entries of the normalised P -- so only the values fed to the P.V product are masked, and the
  // 1 / (1 - p) is folded into the final 1 / l.
  const unsigned dseed = DROP ? dropout_pair_seed(a.drop_seed, b * a.H + hd) : 0u;
  const unsigned dthr = DROP ? dropout_threshold(a.p_drop) : 0u;

  Frag<T> qf[C::NKK];
  if constexpr (FUSEQ) {
    static_assert(sizeof(T) == 2 && D <= 128 && C::NW == 8, "fused Q projection: the 8-wave 16-bit configurations");
    constexpr int EC = 128, WS = EC * 2 + 16, WIMG = D * WS;      // W_q chunk image: D rows x 128 columns, padded row stride (conflict-free ds_read_b128 along rows)
    static_assert(2 * WIMG <= 2 * C::RIMG + 4 * CV::CIMG, "W_q chunk buffers must fit the (idle) K / V tile buffers");
    const T* xrow = reinterpret_cast<const T*>(a.xq) + ((long)b * a.S + qc) * a.E;
    const T* wq_h = reinterpret_cast<const T*>(a.wq) + (long)(hd * D) * a.E;
    f32x16 qa[C::NDB];
#pragma unroll
    for (int db = 0; db < C::NDB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) qa[db][r] = 0.f;
    TileStage<T, D, EC * 2, C::NT> sw;
    const int nch = a.E / EC;
    sw.issue(wq_h, a.E, D, EC);
    sw.template commit_p<WS>(smem);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
      const lds_char* wimg = smem + (ch & 1) * WIMG;
      if (ch + 1 < nch) sw.issue(wq_h + (ch + 1) * EC, a.E, D, EC);      // the next chunk's loads stay in flight under this chunk's products
      Frag<T> xf[EC / 16];
#pragma unroll
      for (int ks = 0; ks < EC / 16; ++ks) xf[ks] = load_frag_global<T>(xrow + ch * EC + ks * 16 + 8 * h);
#pragma unroll
      for (int ks = 0; ks < EC / 16; ++ks) {
        Frag<T> wf[C::NDB];
#pragma unroll
        for (int db = 0; db < C::NDB; ++db) wf[db] = load_frag_row_p<T, WS>(wimg, db * 32 + li, ks * 16);
#pragma unroll
        for (int db = 0; db < C::NDB; ++db) qa[db] = mma32(wf[db], xf[ks], qa[db]);
      }
      if (ch + 1 < nch) sw.template commit_p<WS>(smem + ((ch + 1) & 1) * WIMG);
      __syncthreads();
    }
    const float* bq = a.bq + hd * D;
    T* qout = reinterpret_cast<T*>(const_cast<void*>(a.qkv)) + (long)b * a.S * rs + hd * D + (long)qc * rs;
#pragma unroll
    for (int db = 0; db < C::NDB; ++db)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(bq + db * 32 + 16 * c + 4 * h), b1 = *reinterpret_cast<const f32x4*>(bq + db * 32 + 16 * c + 8 + 4 * h);
        const float add8[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
        qf[2 * db + c] = acc_to_frag_m1<T>(qa[db], c, add8);
        if (a.q_store && qvalid) *reinterpret_cast<X8<T>*>(qout + (2 * db + c) * 16 + 8 * h) = qf[2 * db + c].v;      // the backward reads Q from qkv
      }
  } else {
#pragma unroll
    for (int kk = 0; kk < C::NKK; ++kk) qf[kk] = load_frag_global<T>(Qp + (long)qc * rs + kk * 16 + 8 * h);
  }

  // initial state: the self key for test rows, empty for train rows.  The self K / V rows are only fetched by waves
  // that hold a test row at all (wave-uniform branch): 7 of 8 waves at the north star skip 24 loads per lane.
  const bool is_test = CACHE || qc >= sep;
  const bool wave_has_test = CACHE ? blockIdx.z == 0 : wg.blk * C::QBLK + wave * 32 + 31 >= sep;
  float m = -1e30f, lsum = 0.f;
  f32x16 o[CV::NDB];
#pragma unroll
  for (int db = 0; db < CV::NDB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
  if (wave_has_test) {
    float part = 0.f;
#pragma unroll
    for (int kk = 0; kk < C::NKK; ++kk) part += dot8(qf[kk], load_frag_global<T>(Kp + (long)qc * rs + kk * 16 + 8 * h));
    part += __shfl_xor(part, 32, 64);
    m = is_test ? part * scale_log2 : -1e30f;
    lsum = (is_test && h == 0) ? 1.f : 0.f;
#pragma unroll
    for (int db = 0; db < CV::NDB; ++db)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        f32x4 v = load4<T>(Vp + (long)qc * rs + db * 32 + 8 * rg + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[db][4 * rg + e] = (is_test && (!DROP || dropout_keep(dseed, (unsigned)qc, (unsigned)qc, dthr))) ? v[e] : 0.f;
      }
  }

  const int nfull = sep / C::KVB;
  const int ntiles = (sep + C::KVB - 1) / C::KVB;
  TileStage<T, C::KVB, C::RB, C::NT> sk;
  TileStage<T, C::KVB, CV::RB, C::NT> sv;
  if (ntiles > 0) {
    sk.issue(Ksrc, kld, sep, D);
    sv.issue(Vsrc, kld, sep, DV);
    sk.template commit_p<C::RS>(Kt(0));
    sv.template commit_p<CV::CS>(Vt(0));
    if (ntiles > 1) {   // tile 1 stays in flight across the barrier (see the loop)
      sk.issue(Ksrc + (long)C::KVB * kld, kld, sep - C::KVB, D);
      sv.issue(Vsrc + (long)C::KVB * kld, kld, sep - C::KVB, DV);
    }
  }
  __syncthreads();

  // Software pipeline over key tiles, P.V ONE TILE BEHIND Q.K:
  //   iteration t :  S = K_t Q^T (MFMA)  |  running-max check (rare rescale)  |  { P_t = exp2(S - m)  +  O += V_{t-1} P_{t-1} }
  // The exponentials of tile t (the bulk of the vector work: fma, exp, row sums, bf16 packing) and the 16 P.V
  // MFMAs of tile t-1 are independent and sit in one basic block, so the matrix pipe runs under the vector ALU
  // instead of after it.  P_{t-1} waits in registers as packed operand fragments; V needs three LDS buffers
  // (tile t-1 is read while tile t+1 is written), K two.
  // The running max is only raised -- and O, the row sums and the pending P_{t-1} only rescaled -- when some row's
  // tile max exceeds it by more than RESCALE_THR (log2 units): P stays below 2^THR, which neither the bf16
  // operand rounding (relative) nor the f32 sums notice, and the O-wide rescale runs on the first tile and then
  // almost never.  The key mask only runs on the ragged last tile.
  // What the parts of a tile cost at the north-star shape (timed with each taken out, profiles/r01_attention_sq_counters.txt): the global tile
  // requests 9-14 %, the LDS tile writes 6-7 %, the barrier 4 %.
  constexpr int NPF = C::KVB / 16;
  Frag<T> pf[NPF];                       // P_{t-1}, in the slot order the P.V MFMA consumes
  auto pv_prev = [&](int vb) __attribute__((always_inline)) {
    const lds_char* vt = Vt(vb);
#pragma unroll
    for (int c = 0; c < NPF; ++c)
#pragma unroll
      for (int db = 0; db < CV::NDB; ++db)
        o[db] = mma32(load_frag_tr_p<T, CV::CS, 2>(vt, c * 16, db * 32), pf[c], o[db]);
  };
  int vb_prev = 0, vb_cur = 0;           // V buffer of tile t-1 / tile t
  for (int t = 0; t < ntiles; ++t) {
    const int k0 = t * C::KVB;
    // all K fragments of the tile are requested before anything else: the LDS round trip (>100 cycles under load)
    // then overlaps the global-load issue below and the first MFMAs instead of stalling each one
    const lds_char* kt = Kt(t & 1);
    Frag<T> kfr[C::NKK][C::NKB];
#pragma unroll
    for (int kk = 0; kk < C::NKK; ++kk)
#pragma unroll
      for (int kb = 0; kb < C::NKB; ++kb) kfr[kk][kb] = load_frag_row_p<T, C::RS>(kt, kb * 32 + li, kk * 16);
    PFN_PIN_LDS_MFMA();
    f32x16 st[C::NKB];
#pragma unroll
    for (int kb = 0; kb < C::NKB; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) st[kb][r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < C::NKK; ++kk)
#pragma unroll
      for (int kb = 0; kb < C::NKB; ++kb) st[kb] = mma32(kfr[kk][kb], qf[kk], st[kb]);
    PFN_PIN_LDS_MFMA();
    // Global -> LDS staging, one tile ahead with the loads in flight across the barrier: the staged registers hold
    // tile t+1 (requested one iteration ago); they are written to the buffers tile t-1 has released -- the wait for
    // them sits behind the queued Q.K MFMAs -- and at once re-used for the request of tile t+2.  On the last tile the
    // registers are stale and go to buffers nobody reads again (a branch here would split the block and strand the
    // exponentials behind the P.V MFMAs).
    const int vb_next = vb_cur == NVB - 1 ? 0 : vb_cur + 1;   // the slot tile t-3 has released
    sk.template commit_p<C::RS>(Kt((t + 1) & 1));
    sv.template commit_p<CV::CS>(Vt(vb_next));
    if (t + 2 < ntiles) {
      const long k2 = k0 + 2 * C::KVB;
      sk.issue(Ksrc + k2 * kld, kld, sep - (int)k2, D);
      sv.issue(Vsrc + k2 * kld, kld, sep - (int)k2, DV);
    }
    if (t == nfull) {   // ragged last tile: keys >= sep do not exist
#pragma unroll
      for (int kb = 0; kb < C::NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (k0 + kb * 32 + acc_row(r, lane) >= sep) st[kb][r] = -INFINITY;
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < C::NKB; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[kb][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mc = mx * scale_log2;
    if (__builtin_amdgcn_ballot_w64(mc > m + RESCALE_THR) != 0) {
      const float m_new = fmaxf(m, mc);
      const float alpha = fast_exp2(m - m_new);
      m = m_new;
      lsum *= alpha;
#pragma unroll
      for (int db = 0; db < CV::NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
      if (t > 0) {     // P_{t-1} is still at the old maximum
#pragma unroll
        for (int c = 0; c < NPF; ++c)
#pragma unroll
          for (int e = 0; e < 8; ++e) pf[c].set(e, frag_get(pf[c], e) * alpha);
      }
    }
    if (lag) __syncthreads();     // the lagging waves' barrier of this tile (ping-pong, above)
    if (t > 0) {
      // one basic block: exponentials of tile t + P.V MFMAs of tile t-1
      float rsum = 0.f;
#pragma unroll
      for (int kb = 0; kb < C::NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = fast_exp2(__builtin_fmaf(st[kb][r], scale_log2, -m));
          st[kb][r] = p;
          rsum += p;
        }
      lsum += rsum;
      pv_prev(vb_prev);
    } else {
      float rsum = 0.f;
#pragma unroll
      for (int kb = 0; kb < C::NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = fast_exp2(__builtin_fmaf(st[kb][r], scale_log2, -m));
          st[kb][r] = p;
          rsum += p;
        }
      lsum += rsum;
    }
    if constexpr (DROP) {     // (after the row sums: they belong to the unmasked softmax)
#pragma unroll
      for (int kb = 0; kb < C::NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (!dropout_keep(dseed, (unsigned)qc, (unsigned)(k0 + kb * 32 + acc_row(r, lane)), dthr)) st[kb][r] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < NPF; ++c) pf[c] = acc_to_frag<T>(st[c >> 1], c & 1);
    vb_prev = vb_cur;
    vb_cur = vb_next;
    if (!lag) __syncthreads();
  }
  if (ntiles > 0) pv_prev(vb_prev);

  lsum += __shfl_xor(lsum, 32, 64);
  if constexpr (CACHE) {
    if (gridDim.z > 1) {      // one split of several: unnormalised output and (m, l) for attn_merge_kernel
      const long prow = ((long)blockIdx.z * a.B + b) * a.S + qc;
      float* out = a.part_o + prow * a.E + hd * D + vcol0;
#pragma unroll
      for (int db = 0; db < CV::NDB; ++db) {
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = o[db][r];
        store_row_block<float>(out + db * 32, v, h, qvalid);
      }
      if (qvalid && h == 0 && vcol0 == 0) *reinterpret_cast<float2*>(a.part_ml + 2 * (prow * a.H + hd)) = make_float2(m, lsum);
      return;
    }
  }
  const float inv = DROP ? 1.f / (lsum * (1.f - a.p_drop)) : 1.f / lsum;
  {
    T* out = reinterpret_cast<T*>(a.ctx) + ((long)b * a.S + qc) * a.E + hd * D + vcol0;
#pragma unroll
    for (int db = 0; db < CV::NDB; ++db) {
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = o[db][r] * inv;
      store_row_block<T>(out + db * 32, v, h, qvalid);
    }
    // (CACHE: only when the predict pass keeps its activations for a backward -- pfn_stack_predict_saved)
    if ((!CACHE || a.lse) && qvalid && h == 0 && vcol0 == 0) a.lse[((long)b * a.H + hd) * a.S + qi] = (m + __builtin_amdgcn_logf(lsum)) * LN2;
  }
}

// The splits of a predict pass (attn_fwd_kernel CACHE, gridDim.z > 1) merged: ctx = sum_z 2^(m_z - M) o_z / sum_z 2^(m_z - M) l_z with M = max_z m_z.
// One thread per (test row, 4 columns); the split count is small (attn_cache_splits), the pass reads nsplit x B n E floats once.
template <typename T>
__global__ __launch_bounds__(256) void attn_merge_kernel(AttnArgs a, int nsplit, int D) {
  const long rows = (long)a.B * a.S, c4n = a.E / 4, total = rows * c4n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long row = i / c4n;
    const int c = (int)(i - row * c4n) * 4, hd = c / D;
    const int nz = cache_live_splits(a.sep_of, (int)(row / a.S), a.sep, a.split_keys, nsplit);      // (the splits beyond wrote nothing)
    float mx = -INFINITY;
    for (int z = 0; z < nz; ++z) mx = fmaxf(mx, a.part_ml[2 * ((z * rows + row) * a.H + hd)]);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float l = 0.f;
    for (int z = 0; z < nz; ++z) {
      const float2 ml = *reinterpret_cast<const float2*>(a.part_ml + 2 * ((z * rows + row) * a.H + hd));
      const float w = fast_exp2(ml.x - mx);
      l += w * ml.y;
      const f32x4 v = *reinterpret_cast<const f32x4*>(a.part_o + (z * rows + row) * a.E + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += w * v[e];
    }
    const float inv = 1.f / l;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] *= inv;
    store4<T>(reinterpret_cast<T*>(a.ctx) + row * a.E + c, acc);
    // the merged log-sum-exp (natural units, as the unsplit kernel writes it) when a backward will read it
    if (a.lse && c % D == 0) a.lse[((row / a.S) * a.H + hd) * a.S + row % a.S] = (mx + __builtin_amdgcn_logf(l)) * LN2;
  }
}

// =============================================================================================
// predict backward against a K / V cache (pfn_stack_predict_backward): d(q | k | v) of the test rows, the cached keys and values being constants
// =============================================================================================
// The forward's CACHE layout (lane <-> query, S^T = K Q^T) with the saved log-sum-exp in place of the online softmax.  Per key tile of KVB keys and wave:
//   S^T  = K Q^T     (accumulator pre-loaded with -lse2 / c:  P = exp2(c S'))
//   dP^T = V dO^T    (pre-loaded with -delta:                 dS = P dP')
//   dQ^T += K^T dS^T (K from a column image of the same tile; dS^T leaves the accumulator as the forward's P does for P.V)
// The training query-block pass with P recomputed instead of read: no dS^T is stored, and dQ stays in registers over the key sweep.  delta = rowsum(dO o O) is
// formed in the prologue from the lane's own rows.  The self key is the initial state: dQ^T starts at ds_self k_self, and split 0 writes
// dk_self = ds_self q / sqrt(D) and dv_self = p_self dO.  (Centred keys change nothing: the shift is one vector per dataset and sum_j dS_j = 0.)
// One split: dQ / sqrt(D) goes straight to dqkv.  Several (gridDim.z): f32 partials [nsplit, B, n, E], summed in split order by attn_bwd_cache_merge_kernel.
// DQ < D (exact f32 at head dim 256, as the forward's V slices): the dQ columns in gridDim.y slices, each of which forms the whole S and dP.
template <typename T, int D> struct BwdCacheCfg {
  static constexpr int DQ = (sizeof(T) == 4 && D == 256) ? 128 : D;
  static constexpr int KVB = 32;                       // keys per tile: one 32 x 32 accumulator each for S and dP
  static constexpr int NKK = D / 16, NDQ = DQ / 32, NPF = KVB / 16;
  static constexpr int RB = D * (int)sizeof(T), QB = DQ * (int)sizeof(T);
  static constexpr int RS = PadStride<RB>::ROW, CSQ = PadStride<QB>::COL;
  static constexpr int KROW = KVB * RS, KCOL = KVB * CSQ;
  static constexpr size_t LDS = 2 * KROW + KCOL;       // K and V row images, the K column image (the dQ slice's columns)
  // the next tile's loads in flight under this tile's products -- except in exact f32 at head dim 256, where the staging registers (80) would spill
  static constexpr bool PREFETCH = !(sizeof(T) == 4 && D == 256);
};

template <typename T, int D>
__global__ __launch_bounds__((AttnCfg<T, D>::NT)) void attn_bwd_cache_kernel(AttnCacheBwdArgs a) {
  operand_store_mode<T>();
  using C = AttnCfg<T, D>;
  using G = BwdCacheCfg<T, D>;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  LdsPtr smem = lds_cast(smem_raw);
  LdsPtr Krow = smem, Vrow = smem + G::KROW, Kcol = smem + 2 * G::KROW;
  const AttnBlock wg = attn_block((a.S + C::QBLK - 1) / C::QBLK, a.H);
  const int b = wg.b, hd = wg.hd;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, li = lane & 31;
  const int qcol0 = G::DQ == D ? 0 : (int)blockIdx.y * G::DQ;
  const long rs = 3L * a.E;
  const int qi = wg.blk * C::QBLK + wave * 32 + li;
  const bool qvalid = qi < a.S;
  const long row = (long)b * a.S + min(qi, a.S - 1);
  const T* qrow = reinterpret_cast<const T*>(a.qkv) + row * rs + hd * D;
  const T* orow = reinterpret_cast<const T*>(a.ctx) + row * a.E + hd * D;
  const T* dorow = reinterpret_cast<const T*>(a.dctx) + row * a.E + hd * D;
  const int z = blockIdx.z, k_lo = z * a.split_keys;
  const int nkeys = max(0, min(cache_sep(a.sep_of, b, a.sep) - k_lo, a.split_keys));      // (wave-uniform, as the forward's)
  if (z > 0 && nkeys == 0) return;      // ragged context: an empty split leaves no partial (cache_live_splits); the self-key terms belong to split 0
  const long kld = a.kv_ld;
  const T* Ksrc = reinterpret_cast<const T*>(a.kv) + b * a.kv_sb + k_lo * kld + hd * D;
  const T* Vsrc = Ksrc + a.E;
  const float scale = rsqrtf((float)D), c2 = scale * LOG2E;

  Frag<T> qf[G::NKK], df[G::NKK];
  float dpart = 0.f;
#pragma unroll
  for (int kk = 0; kk < G::NKK; ++kk) {
    qf[kk] = load_frag_global<T>(qrow + kk * 16 + 8 * h);
    df[kk] = load_frag_global<T>(dorow + kk * 16 + 8 * h);
    dpart += dot8(df[kk], load_frag_global<T>(orow + kk * 16 + 8 * h));
  }
  const float delta = dpart + __shfl_xor(dpart, 32, 64);
  const float lse2 = a.lse[((long)b * a.H + hd) * a.S + (row - (long)b * a.S)] * LOG2E;

  f32x16 o[G::NDQ];      // dQ^T (rows = the slice's columns, lane = query), unscaled
#pragma unroll
  for (int db = 0; db < G::NDQ; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
  if (z == 0) {      // the self key: its probability and score gradient from the lane's own rows
    const T* krow = qrow + a.E;
    const T* vrow = qrow + 2 * a.E;
    float sp = 0.f, dpp = 0.f;
#pragma unroll
    for (int kk = 0; kk < G::NKK; ++kk) {
      sp += dot8(qf[kk], load_frag_global<T>(krow + kk * 16 + 8 * h));
      dpp += dot8(df[kk], load_frag_global<T>(vrow + kk * 16 + 8 * h));
    }
    sp += __shfl_xor(sp, 32, 64);
    dpp += __shfl_xor(dpp, 32, 64);
    const float p = fast_exp2(__builtin_fmaf(sp, c2, -lse2)), ds = p * (dpp - delta);
#pragma unroll
    for (int db = 0; db < G::NDQ; ++db)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const f32x4 kv4 = load4<T>(krow + qcol0 + db * 32 + 8 * rg + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[db][4 * rg + e] = ds * kv4[e];
      }
    if (qvalid && blockIdx.y == 0) {
      T* dst = reinterpret_cast<T*>(a.dqkv) + row * rs + hd * D;
#pragma unroll
      for (int kk = 0; kk < G::NKK; ++kk) {
        float vk[8], vv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { vk[e] = scale * ds * frag_get(qf[kk], e); vv[e] = p * frag_get(df[kk], e); }
        store_frag_global<T>(dst + a.E + kk * 16 + 8 * h, vk);
        store_frag_global<T>(dst + 2 * a.E + kk * 16 + 8 * h, vv);
      }
    }
  }

  // key tiles through one LDS set, staged in registers one tile ahead where the budget allows (BwdCacheCfg::PREFETCH)
  const int ntiles = (nkeys + G::KVB - 1) / G::KVB;
  TileStage<T, G::KVB, G::RB, C::NT> sk, sv;
  TileStage<T, G::KVB, G::QB, C::NT> skc;      // (DQ < D only: the slice's K columns)
  auto issue = [&](int t) __attribute__((always_inline)) {
    const long k0 = (long)t * G::KVB;
    sk.issue(Ksrc + k0 * kld, kld, nkeys - (int)k0, D);
    sv.issue(Vsrc + k0 * kld, kld, nkeys - (int)k0, D);
    if constexpr (G::DQ < D) skc.issue(Ksrc + k0 * kld + qcol0, kld, nkeys - (int)k0, G::DQ);
  };
  if constexpr (G::PREFETCH) { if (ntiles > 0) issue(0); }
  const float s0 = -lse2 / c2;
  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();      // every wave is done with tile t - 1
    if constexpr (!G::PREFETCH) issue(t);
    sk.template commit_p<G::RS>(Krow);
    sv.template commit_p<G::RS>(Vrow);
    if constexpr (G::DQ < D) skc.template commit_p<G::CSQ>(Kcol);
    else sk.template commit_p<G::CSQ>(Kcol);
    __syncthreads();
    if constexpr (G::PREFETCH) { if (t + 1 < ntiles) issue(t + 1); }
    f32x16 st, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) { st[r] = s0; dp[r] = -delta; }
#pragma unroll
    for (int kk = 0; kk < G::NKK; ++kk) st = mma32(load_frag_row_p<T, G::RS>(Krow, li, kk * 16), qf[kk], st);
#pragma unroll
    for (int kk = 0; kk < G::NKK; ++kk) dp = mma32(load_frag_row_p<T, G::RS>(Vrow, li, kk * 16), df[kk], dp);
    const int k0 = t * G::KVB;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = (k0 + acc_row(r, lane) < nkeys) ? fast_exp2(st[r] * c2) : 0.f;      // (keys past the split: zero rows of the tile)
      st[r] = p * dp[r];
    }
    Frag<T> dsf[G::NPF];
#pragma unroll
    for (int c = 0; c < G::NPF; ++c) dsf[c] = acc_to_frag<T>(st, c);
#pragma unroll
    for (int c = 0; c < G::NPF; ++c)
#pragma unroll
      for (int db = 0; db < G::NDQ; ++db) o[db] = mma32(load_frag_tr_p<T, G::CSQ, 2>(Kcol, c * 16, db * 32), dsf[c], o[db]);
  }

  if (gridDim.z == 1) {
    T* out = reinterpret_cast<T*>(a.dqkv) + row * rs + hd * D + qcol0;
#pragma unroll
    for (int db = 0; db < G::NDQ; ++db) {
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = o[db][r] * scale;
      store_row_block<T>(out + db * 32, v, h, qvalid);
    }
  } else {
    float* out = a.part_dq + ((long)z * a.B * a.S + row) * a.E + hd * D + qcol0;
#pragma unroll
    for (int db = 0; db < G::NDQ; ++db) {
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = o[db][r];
      store_row_block<float>(out + db * 32, v, h, qvalid);
    }
  }
}

// The splits' partial dQ summed in split order (no atomics: the same bits on every run) and scaled into dqkv's Q columns; one thread per (test row, 4 columns)
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_cache_merge_kernel(AttnCacheBwdArgs a, int nsplit, float scale) {
  const long rows = (long)a.B * a.S, c4n = a.E / 4, total = rows * c4n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long row = i / c4n;
    const int c = (int)(i - row * c4n) * 4;
    const int nz = cache_live_splits(a.sep_of, (int)(row / a.S), a.sep, a.split_keys, nsplit);
    f32x4 acc = *reinterpret_cast<const f32x4*>(a.part_dq + row * a.E + c);
    for (int z = 1; z < nz; ++z) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(a.part_dq + (z * rows + row) * a.E + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += v[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] *= scale;
    store4<T>(reinterpret_cast<T*>(a.dqkv) + row * 3L * a.E + c, acc);
  }
}

// =============================================================================================
// backward, step 0: delta[b,h,i] = sum_d dO[i,d] * O[i,d]
// =============================================================================================
template <typename T>
__global__ __launch_bounds__(256) void attn_delta_kernel(AttnArgs a, int D) {
  // one 16-lane group per (token, head) pair; grid-stride over B*S*H pairs
  const long pairs = (long)a.B * a.S * a.H;
  const int sub = threadIdx.x & 15;
  for (long pr = (long)blockIdx.x * 16 + (threadIdx.x >> 4); pr < pairs; pr += (long)gridDim.x * 16) {
    const long tok = pr / a.H;
    const int hd = (int)(pr % a.H);
    if ((int)(tok % a.S) < (a.q_from_sep ? a.sep_of[tok / a.S] / 256 * 256 : a.q_begin)) continue;      // (uniform over the 16-lane group; no wave-wide operation below)
    const T* o = reinterpret_cast<const T*>(a.ctx) + tok * a.E + hd * D;
    const T* d = reinterpret_cast<const T*>(a.dctx) + tok * a.E + hd * D;
    float s = 0.f;
    for (int c = sub * 4; c < D; c += 64) {
      f32x4 x = load4<T>(o + c), y = load4<T>(d + c);
      s += x[0] * y[0] + x[1] * y[1] + x[2] * y[2] + x[3] * y[3];
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (sub == 0) {
      const long bb = tok / a.S, i = tok % a.S;
      a.delta[(bb * a.H + hd) * a.S + i] = s;
      // second half of the scratch: the row's log-sum-exp in log2 units, so the key-block pass forms P = exp2(S c - lse2) with ONE fma per
      // element (it read the natural-log value and paid a multiply per element for the conversion: 16 of ~190 vector slots per tile)
      a.delta[(long)a.B * a.H * a.S + (bb * a.H + hd) * a.S + i] = a.lse[(bb * a.H + hd) * a.S + i] * LOG2E;
    }
  }
}

// =============================================================================================
// backward, key-block pass: dK and dV for the train keys [0, sep), and dS^T for the dQ pass.
//
// A workgroup owns QBLK keys (one per lane, 32 per wave) and streams all S queries in tiles of 32.  Per tile and
// wave:   S = Q K^T,  dP = dO V^T   (lane <-> key, rows <-> queries; 8 + 8 MFMAs at head dim 128)
//         P = exp2(S scale - lse),  dS = P (dP - delta)
//         dV^T += dO^T P,  dK^T += Q^T dS   (P and dS go from the accumulator straight into the operand slots)
//         dS^T[key][query] -> global, in operand precision -- the exact values the dK product consumed.
// S and dP are computed ONCE for the whole backward (round 1 recomputed S three times and dP twice: 8 product
// units for 4 algorithmic ones; now 5 with the dQ pass below).  Register budget at head dim 128, bf16: K fragments
// of the wave's keys 32 + dK and dV accumulators 128 stay for the whole kernel; the V fragments (B operand of the dP
// product) would be another 32 and push the kernel out of the 256 registers that two waves per SIMD allow, so the
// workgroup's V rows live in LDS as a row image (69 KB, loaded once) and are read per tile like the Q / dO rows.
// The 4-wave configurations (exact-f32 mode, head dim 256) have the whole register file and keep V in registers.
// Keys >= sep in the last key block run on clamped data: never stored (dK, dV) and never read (the dQ pass
// zero-fills dS^T rows >= sep when it stages them).
// =============================================================================================
// LDS row of query q of a 32-query tile in the one-image layout of the key-block pass (BwdKvCfg::ONE): the two 2-bit fields of the row index swapped
__host__ __device__ constexpr int kv_row_perm(int q) { return 4 * (q & 3) + ((q >> 2) & 3) + (q & ~15); }
// The transposed fragment (MAP 2 of load_frag_tr_p: k = query rows k0 + 4h + {0..3} and k0 + 8 + 4h + {0..3}, the accumulator's row order) from that
// image: kv_row_perm(k0 + 4h + j) = 4 j + h + k0 and kv_row_perm(k0 + 8 + 4h + j) = 4 j + h + 2 + k0 for k0 in {0, 16} -- one lane base, immediate offsets
template <typename T, int STRIDE> PFN_DEV Frag<T> load_frag_tr_perm(const lds_char* tile, int k0, int col0) {
  static_assert(sizeof(T) == 2, "one-image layout: 2-byte operands");
  const int l = lane_id(), h = l >> 5, i = l & 15, g = (l >> 4) & 1;
  const int colb = (col0 + 16 * g + 4 * (i & 3)) * 2;
  const int row = 4 * (i >> 2) + h + k0;
  Frag<T> f;
  const auto lo = ds_read_tr16_b64<T>(tile + row * STRIDE + colb);
  const auto hi = ds_read_tr16_b64<T>(tile + (row + 2) * STRIDE + colb);
  f.v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return f;
}

template <typename T, int D> struct BwdKvCfg {
  using C = AttnCfg<T, D>;
  static constexpr int QB = 32;                         // queries per tile
  static constexpr bool VLDS = C::NW == 8;              // V rows of the workgroup's keys in LDS instead of registers
  static constexpr int VIMG = VLDS ? C::QBLK * C::RS : 0;
  // A Q / dO tile is read twice per wave: along its rows (ds_read_b128, A operand of S = Q K^T / dP = dO V^T) and transposed (ds_read_b64_tr_b16, A
  // operand of dV^T += dO^T P / dK^T += Q^T dS).  The two patterns want different paddings (PadStride: row stride = 4 x odd dwords for the
  // first, 16 x odd for the second), so rounds 1-3 kept every tile twice -- and paid for it in LDS-DMA instructions, the largest single item of
  // the pass (profiles/r03_attention_experiments.txt: 36 one-KiB pieces per tile, -75 us of 523 without them).  ONE image serves both when query
  // q sits in LDS row perm(q) = 4 (q & 3) + ((q >> 2) & 3) + 16 (q >> 4) (the two 2-bit fields of the row index swapped) under the ROW padding:
  // the transposed read's four consecutive queries are then rows 4 apart = 16 x odd dwords apart, and the row read's 16-lane groups
  // ({0-3, 12-15, 20-27}, ...) still cover every residue mod 16.  Both stay conflict-free; the tile costs half the DMA pieces and half the LDS.
  static constexpr bool ONE = sizeof(T) == 2;
  // Q / dO tiles go global -> LDS by LDS-DMA in 1-KiB pieces (64 lanes x 16 bytes, lane-linear in LDS): every image is
  // allocated in whole pieces; piece p of an image holds its bytes [1024 p, 1024 p + 1024)
  static constexpr int NPR = (QB * C::RS + 1023) / 1024, NPC = ONE ? 0 : (QB * C::CS + 1023) / 1024;   // pieces of a row / col image
  static constexpr int RIMG = NPR * 1024, CIMG = NPC * 1024;
  static constexpr int NP = 2 * (NPR + NPC);                  // Q rows, Q cols, dO rows, dO cols
  static constexpr int NI = (NP + C::NW - 1) / C::NW;         // pieces per wave
  static constexpr int IMG = 2 * (RIMG + CIMG);
  static constexpr int BUF = IMG + 2 * QB * 4;                // + lse2[QB], delta[QB]
  // Tile buffers: two (tile t is computed while tile t+1 lands) -- three in the 8-wave one-image configurations, where the LDS has the room and the
  // PING-PONG schedule needs it: waves 4..7 take their one barrier per tile BETWEEN the S / dP half (row reads, exponentials) and the dV / dK half
  // (transposed reads, 16 MFMAs) instead of at the tile's end, so the two waves of a SIMD run half a tile apart and one's vector-heavy half overlaps the
  // other's matrix-heavy half (the forward's schedule, attn_fwd_kernel).  The lagging waves still read tile t's buffer while the leading ones request
  // tile t+2: that request goes to the THIRD buffer (last read in tile t-1, which every wave has left at the barrier in front of the request).
  static constexpr int NBUF = (ONE && C::NW == 8) ? 3 : 2;
  // fragment prefetch depth (k-steps of 16) of the two row-operand chains: how far the LDS reads of the Q / dO (and V) row fragments run ahead of their MFMAs
  static constexpr int PD = 2;
  // the lanes' DMA source offsets (one per piece of the wave) live in an LDS table when there is room (every shipped shape):
  // recomputing them per tile costs ~20 vector instructions per piece, keeping them in registers costs registers this kernel
  // does not have
  static constexpr bool PVLDS = VIMG + NBUF * BUF + NI * C::NT * 4 <= 160 * 1024;
  static constexpr int PVTAB = PVLDS ? NI * C::NT * 4 : 0;
  static constexpr int LDS = VIMG + NBUF * BUF + PVTAB;
};

// dK and dV in ONE pass at every head dim.  At head dim 256 both accumulators fit the whole register file beside the K and V fragments
// (508 VGPRs, no scratch) because the transposed fragments of the dV / dK products are held one group of four at a time and P is unpacked
// from its packed registers: 64 MFMAs per tile and one sweep over the Q / dO tiles (two passes, dV then dK, take 80 and two sweeps).
template <typename T, int D, bool DROP = false>
__global__ __launch_bounds__((AttnCfg<T, D>::NT)) void attn_bwd_kv_kernel(AttnArgs a) {
  operand_store_mode<T>();
  using C = AttnCfg<T, D>;
  using K = BwdKvCfg<T, D>;
  constexpr int QB = K::QB;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  LdsPtr smem = lds_cast(smem_raw);
  auto Vimg = [&]() { return smem; };
  auto Qr = [&](int buf) { return smem + K::VIMG + buf * K::BUF; };
  auto Qc = [&](int buf) { return smem + K::VIMG + buf * K::BUF + (K::ONE ? 0 : K::RIMG); };      // (ONE: the one image of the tile)
  auto Or = [&](int buf) { return smem + K::VIMG + buf * K::BUF + K::RIMG + K::CIMG; };
  auto Oc = [&](int buf) { return smem + K::VIMG + buf * K::BUF + (K::ONE ? K::RIMG : 2 * K::RIMG + K::CIMG); };
  auto St = [&](int buf) { return smem + K::VIMG + buf * K::BUF + K::IMG; };   // [lse x QB][delta x QB]

  // (ragged batch: the grid has ceil(max position / 256) blocks per (dataset, head); a dataset's blocks past ITS position leave at once)
  const AttnBlock wg = a.sep_of ? attn_block((a.sep + C::QBLK - 1) / C::QBLK, a.H) : attn_block_ragged_last((a.sep + C::QBLK - 1) / C::QBLK, a.sep / C::QBLK, a.H);
  const int b = wg.b, hd = wg.hd;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, h = lane >> 5, li = lane & 31;
  const long rs = 3L * a.E;
  const T* base = reinterpret_cast<const T*>(a.qkv) + (long)b * a.S * rs;
  const T* Qp = base + hd * D;
  const T* Kp = base + a.E + hd * D;
  const T* Vp = base + 2 * a.E + hd * D;
  const T* dOp = reinterpret_cast<const T*>(a.dctx) + (long)b * a.S * a.E + hd * D;
  T* dbase = reinterpret_cast<T*>(a.dqkv) + (long)b * a.S * rs;
  const int sep = a.sep_of ? a.sep_of[b] : a.sep;
  if (wg.blk * C::QBLK >= sep) return;      // (only in a ragged batch; uniform over the workgroup, ahead of every barrier)
  const int lip = K::ONE ? kv_row_perm(li) : li;      // the LDS row of the Q / dO tiles this lane reads along (query li of the tile)
  const bool lag = K::NBUF == 3 && (a.pingpong & 2) && wave >= 4;      // ping-pong (BwdKvCfg::NBUF): this wave takes its barrier in the middle of the tile
  const int key0 = wg.blk * C::QBLK;
  const int key = key0 + wave * 32 + li;
  const bool kvalid = key < sep;
  const int kc = min(key, a.S - 1);
  const float scale = rsqrtf((float)D);
  const float scale_log2 = scale * LOG2E;
  const float* lse_g = a.delta + (long)a.B * a.H * a.S + ((long)b * a.H + hd) * a.S;    // lse in log2 units (attn_delta_kernel)
  const float* delta_g = a.delta + ((long)b * a.H + hd) * a.S;
  // DROP (dropout on the probabilities): dV takes P' = P keep / (1 - p), dP = dP' keep / (1 - p) with dP' = dO V^T, and dS = P (dP - delta)
  // with the UNMASKED P (delta = rowsum(dO O) already is sum_k P'_k dP'_k).  The 1 / (1 - p) of dV is applied when dV is stored.
  const unsigned dseed = DROP ? dropout_pair_seed(a.drop_seed, b * a.H + hd) : 0u;
  const unsigned dthr = DROP ? dropout_threshold(a.p_drop) : 0u;
  const float dscale = DROP ? 1.f / (1.f - a.p_drop) : 1.f;
  const bool wave_all_valid = __builtin_amdgcn_readfirstlane(key0 + wave * 32 + 31) < sep;   // only the last key block has keys >= sep
  const bool wave_live = __builtin_amdgcn_readfirstlane(key0 + wave * 32) < sep;             // ... and waves with no key below sep at all
  // dS^T of this (dataset, head): 32 x 32 blocks, block (key / 32, query / 32) at ((key / 32) * (ds_ld / 32) + query / 32) blocks
  // (store_frag_pair_blocked); the wave owns block row key / 32
  constexpr int DSBLK = 32 * 32;   // elements per block
  T* dsT = reinterpret_cast<T*>(a.ds) + ((long)b * a.H + hd) * a.ds_rows * a.ds_ld + (long)(key0 / 32 + wave) * (a.ds_ld / 32) * DSBLK;
  const bool ds_row_live = key0 + wave * 32 < a.ds_rows;   // wave-uniform: this wave's block row exists in the buffer

  Frag<T> kf[C::NKK], vf[K::VLDS ? 1 : C::NKK];
#pragma unroll
  for (int kk = 0; kk < C::NKK; ++kk) {
    kf[kk] = load_frag_global<T>(Kp + (long)kc * rs + kk * 16 + 8 * h);
    if constexpr (!K::VLDS) vf[kk] = load_frag_global<T>(Vp + (long)kc * rs + kk * 16 + 8 * h);
  }
  if constexpr (K::VLDS) {   // the workgroup's V rows -> LDS row image (rows >= S read as zero)
    TileStageBuf<T, C::QBLK, C::RB, C::NT> sv;
    sv.init((int)(rs * sizeof(T)));
    sv.issue(make_rsrc(Vp, ((long)(a.S - 1) * rs + D) * (long)sizeof(T)), key0 * (int)(rs * sizeof(T)));
    sv.template commit_p<C::RS>(Vimg());
  }
  f32x16 dk[C::NDB], dv[C::NDB];
#pragma unroll
  for (int db = 0; db < C::NDB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dk[db][r] = 0.f;
      dv[db][r] = 0.f;
    }

  const int ntiles = (a.S + QB - 1) / QB;
  // Q / dO tiles: global -> LDS by LDS-DMA through buffer descriptors (rows >= S are out of the descriptor's range and
  // arrive as zeros), issued from assembly (pfn_device.h dma16: why).  No staging registers: the pieces of tile t+1 are issued at the top of tile t into the other buffer and
  // waited for at its end.  Wave w moves pieces w, w + NW, ... of the list [Q rows | Q cols | dO rows | dO cols]; lane l of
  // piece p supplies the 16 bytes at image offset 1024 p + 16 l (a padded row's pad chunk, or the tail past the image, is
  // pointed out of range).
  const DmaRsrc rq = make_dma_rsrc(Qp, ((long)(a.S - 1) * rs + D) * (long)sizeof(T));
  const DmaRsrc ro = make_dma_rsrc(dOp, ((long)(a.S - 1) * a.E + D) * (long)sizeof(T));
  const int tq_bytes = QB * (int)rs * (int)sizeof(T), to_bytes = QB * a.E * (int)sizeof(T);
  const int ldq = (int)rs * (int)sizeof(T), ldo = a.E * (int)sizeof(T);
  // piece i of this wave: wave-uniform LDS offset inside a buffer (bit 30: dO tensor; < 0: none) ...
  int pdst[K::NI];
#pragma unroll
  for (int i = 0; i < K::NI; ++i) {
    const int g = wave + C::NW * i;
    const int img = g < K::NPR ? 0 : g < K::NPR + K::NPC ? 1 : g < 2 * K::NPR + K::NPC ? 2 : 3;
    const int start = img == 0 ? 0 : img == 1 ? K::NPR : img == 2 ? K::NPR + K::NPC : 2 * K::NPR + K::NPC;
    const int ibase = img == 0 ? 0 : img == 1 ? K::RIMG : img == 2 ? K::RIMG + K::CIMG : 2 * K::RIMG + K::CIMG;
    pdst[i] = g < K::NP ? __builtin_amdgcn_readfirstlane((ibase + (g - start) * 1024) | (img >= 2 ? (1 << 30) : 0)) : -1;
  }
  // ... and the lane's source byte offset inside a tile (pad chunks and the tail past the image point out of range)
  auto piece_offset = [&](int i, int ln) {
    const int g = wave + C::NW * i;
    const int img = g < K::NPR ? 0 : g < K::NPR + K::NPC ? 1 : g < 2 * K::NPR + K::NPC ? 2 : 3;
    const int start = img == 0 ? 0 : img == 1 ? K::NPR : img == 2 ? K::NPR + K::NPC : 2 * K::NPR + K::NPC;
    const int c = (g - start) * 64 + ln;
    int row, col;
    if (img & 1) { row = c / (C::CS / 16); col = c % (C::CS / 16); }
    else { row = c / (C::RS / 16); col = c % (C::RS / 16); }
    if constexpr (K::ONE) row = row < QB ? kv_row_perm(row) : row;      // LDS row r holds query perm(r) (an involution)
    return (row < QB && col < C::RB / 16) ? row * (img >= 2 ? ldo : ldq) + col * 16 : BUF_OOB;
  };
  LdsPtr pvtab = smem + K::VIMG + K::NBUF * K::BUF;   // [NI][NT] ints
  if constexpr (K::PVLDS) {
#pragma unroll
    for (int i = 0; i < K::NI; ++i)
      *reinterpret_cast<__attribute__((address_space(3))) int*>(pvtab + (i * C::NT + threadIdx.x) * 4) = piece_offset(i, lane);
  }
  auto dma = [&](int buf, int t) {
    int ln = lane;
    if constexpr (!K::PVLDS) asm volatile("" : "+v"(ln));   // opaque: keeps the offset arithmetic inside the loop (hoisted, it costs a register per piece)
    if constexpr (K::PVLDS) {
      int pv[K::NI];
#pragma unroll
      for (int i = 0; i < K::NI; ++i) pv[i] = *reinterpret_cast<const __attribute__((address_space(3))) int*>(pvtab + (i * C::NT + threadIdx.x) * 4);
#pragma unroll
      for (int i = 0; i < K::NI; ++i) {
        if (pdst[i] < 0) continue;
        LdsPtr dst = smem + K::VIMG + buf * K::BUF + (pdst[i] & 0xffffff);
        if (pdst[i] & (1 << 30)) dma16(ro, dst, pv[i] + t * to_bytes);
        else dma16(rq, dst, pv[i] + t * tq_bytes);
      }
    } else {
#pragma unroll
      for (int i = 0; i < K::NI; ++i) {   // one offset at a time: NI is 18 here and the offsets must not all be live at once
        if (pdst[i] < 0) continue;
        LdsPtr dst = smem + K::VIMG + buf * K::BUF + (pdst[i] & 0xffffff);
        const int pv = piece_offset(i, ln);
        if (pdst[i] & (1 << 30)) dma16(ro, dst, pv + t * to_bytes);
        else dma16(rq, dst, pv + t * tq_bytes);
      }
    }
  };
  // row statistics of the tile's queries: wave 0 brings lse, wave 1 delta (lanes 0..QB-1), by LDS-DMA like the tiles -- a load
  // into a register would be waited for by the compiler with vmcnt(0) at its use (its count cannot see the branches around the
  // dS^T stores), which made waves 0 and 1, and behind the barrier everyone, wait for those stores every tile.  A query beyond S
  // reads zeros everywhere (Q, dO, lse, delta): P = 1 there but dO = 0 and delta = 0, so dV, dS and dK get nothing from it.
  const DmaRsrc rl = make_dma_rsrc(lse_g, (long)a.S * 4), rdl = make_dma_rsrc(delta_g, (long)a.S * 4);
  auto stage_stats = [&](int buf, int q0) {
    if (wave == 0) { if (lane < QB) dma4(rl, St(buf), (lane + q0) * 4); }
    else if (wave == 1) { if (lane < QB) dma4(rdl, St(buf) + QB * 4, (lane + q0) * 4); }
  };
  const int t0 = (a.q_from_sep ? sep / 256 * 256 : a.q_begin) / QB;      // first query tile (0 unless the caller skips the queries below q_begin: AttnArgs; ragged: the dataset's own)
  dma(0, t0);
  stage_stats(0, t0 * QB);
  dma_wait_all();
  __syncthreads();
  if (t0 + 1 < ntiles) {     // the second tile -> the second buffer; from here on a tile's successor-but-one is requested at its end
    dma(1, t0 + 1);
    stage_stats(1, (t0 + 1) * QB);
  }
  constexpr int DST_TILE_WRITES = sizeof(T) == 2 ? 2 : 4;   // store instructions of one tile's dS^T per wave
  bool stored = false;                // this wave's dS^T stores of the previous tile may still be in flight

  auto tile = [&](auto buf_c, int t) {
    constexpr int BUF = decltype(buf_c)::value;
    const lds_char* qr = Qr(BUF);
    const lds_char* orow = Or(BUF);
    const lds_char* stt = St(BUF);
    const lds_char* qc = Qc(BUF);
    const lds_char* oc = Oc(BUF);
    // Register plan (head dim 128, bf16): 160 registers are pinned (K fragments, dK, dV); S and dP take 32 more; every operand
    // stream therefore runs only PD k-steps ahead of its MFMAs and the two products run one after the other, the second
    // one's first fragments requested under the first one's tail.
    constexpr int PD = C::NKK < K::PD ? C::NKK : K::PD;      // both chains: S = Q K^T and dP = dO V^T
    // rows of the S / dP tiles are queries: acc_row(r) = 8*(r>>2) + 4h + (r&3)
    Frag<T> pf0, pf1;
    Frag<T> df0, df1;
    unsigned mbits = 0xffffu;      // DROP: bit r = keep flag of (query row r of the tile, this lane's key)
    // A wave whose 32 keys all lie at or beyond sep (the tail of the last key block) has nothing to compute: it keeps moving its
    // DMA pieces and keeps the barriers, and leaves the matrix pipe, the vector ALU and the LDS ports of its SIMD to its partner.
    // The workgroup of a ragged last block therefore finishes early and frees its CU for the next one (sep mod 256 is uniform:
    // on average half of that block's waves are dead).
    // one barrier per tile and wave: at the tile's end, or (lagging waves of the ping-pong schedule) between its two halves.  Either way it is passed
    // with this wave's LDS reads done and its pieces of tile t+1 landed (vmcnt = the dS^T stores issued behind them: loads and stores retire in order)
    auto sync_tile = [&]() __attribute__((always_inline)) {
      if (stored) wait_vm_barrier<DST_TILE_WRITES>();
      else wait_vm_barrier<0>();
    };
    if (wave_live) {
    {
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
      Frag<T> qfr[C::NKK];
#pragma unroll
      for (int kk = 0; kk < PD; ++kk) qfr[kk] = load_frag_row_p<T, C::RS>(qr, lip, kk * 16);
      PFN_PIN_LDS_MFMA();
#pragma unroll
      for (int kk = 0; kk < C::NKK; ++kk) {
        if (kk + PD < C::NKK) qfr[kk + PD] = load_frag_row_p<T, C::RS>(qr, lip, (kk + PD) * 16);
        s = mma32(qfr[kk], kf[kk], s);
        PFN_PIN_LDS_MFMA();
      }
      // P = exp2(S scale - lse), straight into operand precision: S is dead before the dP chain starts (register plan above)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const f32x4 l2 = __builtin_bit_cast(f32x4, lds_read16(stt + (8 * rg + 4 * h) * 4));   // lse in log2 units
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * rg + e;
          const float arg = __builtin_fmaf(s[r], scale_log2, -l2[e]);
          s[r] = fast_exp2(arg);
        }
      }
      if constexpr (DROP) {
        mbits = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          mbits |= (dropout_keep(dseed, (unsigned)(t * QB + acc_row(r, lane)), (unsigned)key, dthr) ? 1u : 0u) << r;
      }
      pf0 = acc_to_frag<T>(s, 0);
      pf1 = acc_to_frag<T>(s, 1);
      // opaque to the optimizer: the dS stage below unpacks P from these packed registers (a shift or a mask per element); left to
      // see through the packing, hipcc re-rounds every element from the f32 value with a second, single-element conversion + shift
      if constexpr (sizeof(T) == 2) asm volatile("" : "+v"(pf0.v), "+v"(pf1.v));
    }
    {
      f32x16 dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) dp[r] = 0.f;
      Frag<T> ofr[C::NKK], vfr[K::VLDS ? C::NKK : 1];
#pragma unroll
      for (int kk = 0; kk < PD; ++kk) {
        ofr[kk] = load_frag_row_p<T, C::RS>(orow, lip, kk * 16);
        if constexpr (K::VLDS) vfr[kk] = load_frag_row_p<T, C::RS>(Vimg(), wave * 32 + li, kk * 16);
      }
      PFN_PIN_LDS_MFMA();
#pragma unroll
      for (int kk = 0; kk < C::NKK; ++kk) {
        if (kk + PD < C::NKK) {
          ofr[kk + PD] = load_frag_row_p<T, C::RS>(orow, lip, (kk + PD) * 16);
          if constexpr (K::VLDS) vfr[kk + PD] = load_frag_row_p<T, C::RS>(Vimg(), wave * 32 + li, (kk + PD) * 16);
        }
        if constexpr (K::VLDS) dp = mma32(ofr[kk], vfr[kk], dp);
        else dp = mma32(ofr[kk], vf[kk], dp);
        PFN_PIN_LDS_MFMA();
      }
      // dS = P (dP - delta), with the P the dV product consumes (operand precision)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const f32x4 dl = __builtin_bit_cast(f32x4, lds_read16(stt + (QB + 8 * rg + 4 * h) * 4));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * rg + e;
          const float dpr = DROP ? (((mbits >> r) & 1u) ? dp[r] * dscale : 0.f) : dp[r];
          dp[r] = frag_get_bits(r < 8 ? pf0 : pf1, r & 7) * (dpr - dl[e]);
        }
      }
      // (keys >= sep of the last key block: their dS is garbage from clamped rows; it only reaches accumulator columns that are never
      // stored, and is zeroed where it leaves the kernel -- the dS^T store below -- instead of element by element here)
      df0 = acc_to_frag<T>(dp, 0);
      df1 = acc_to_frag<T>(dp, 1);
    }
    }
    if (lag) sync_tile();
    if (wave_live) {
    if constexpr (DROP) {     // the dV product sees the masked probabilities (the dS stage above wanted the unmasked ones)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (!((mbits >> e) & 1u)) pf0.set(e, 0.f);
        if (!((mbits >> (8 + e)) & 1u)) pf1.set(e, 0.f);
      }
    }
    // dV^T += dO^T P,  dK^T += Q^T dS as a list of steps (product, column group): product 0 / 1 = dV with the two halves of P, 2 / 3 = dK
    // with the two halves of dS; a group is CG of the NDB 32-column blocks of the head dimension.  One set of CG transposed fragments
    // is live: the next step's are requested right behind the MFMAs that consume the current ones (head dim 256 takes its 8 blocks
    // as two groups of 4 -- 16 registers instead of 32, which is what the single-pass variant lacked).
    constexpr int CG = C::NDB > 4 ? 4 : C::NDB, NG = C::NDB / CG;
    Frag<T> cf[CG];
    auto request = [&](int step) __attribute__((always_inline)) {
      const int prod = step / NG, grp = step % NG;
      const lds_char* img = prod < 2 ? oc : qc;
#pragma unroll
      for (int c = 0; c < CG; ++c) {
        if constexpr (K::ONE) cf[c] = load_frag_tr_perm<T, C::RS>(img, (prod & 1) * 16, (grp * CG + c) * 32);
        else cf[c] = load_frag_tr_p<T, C::CS, 2>(img, (prod & 1) * 16, (grp * CG + c) * 32);
      }
    };
    request(0);
    PFN_PIN_LDS_MFMA();
#pragma unroll
    for (int step = 0; step < 4 * NG; ++step) {
      const int prod = step / NG, grp = step % NG;
#pragma unroll
      for (int c = 0; c < CG; ++c) {
        const int db = grp * CG + c;
        if (prod < 2) dv[db] = mma32(cf[c], prod == 0 ? pf0 : pf1, dv[db]);
        else dk[db] = mma32(cf[c], prod == 2 ? df0 : df1, dk[db]);
      }
      if (step + 1 < 4 * NG) request(step + 1);
      PFN_PIN_LDS_MFMA();
    }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) { df0.set(e, 0.f); df1.set(e, 0.f); }    // its dS^T rows (if the dQ pass reads them at all) are zeros
    }
    // End of the tile.  gfx9 counts loads and stores in ONE counter and they retire in order: a wait for a load is a wait for
    // every store issued before it.  So the order of issue at a tile's end is: the DMA of tile t+2 (into this tile's buffer, free
    // behind the barrier), THEN this tile's dS^T stores (block (key / 32, t), operand precision: exactly what the dK product
    // consumed) -- and the wait for tile t+1 one tile earlier is vmcnt(stores of the previous tile), which leaves those stores two
    // tile times to be acknowledged instead of stalling every tile on them (with them in front of the DMA: 70 us of 372).
    if (!lag) sync_tile();
    if (t + 2 < ntiles) {
      constexpr int NXT = (BUF + 2) % K::NBUF;      // two buffers: this tile's own (free behind the barrier); three: the one tile t-1 used
      dma(NXT, t + 2);
      stage_stats(NXT, (t + 2) * QB);
    }
    // keys >= sep of a block row the dQ pass reads (rows < ds_rows) leave as zeros: that pass does not mask rows
    if (!wave_all_valid) {      // last key block only (wave-uniform)
      if (!kvalid) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { df0.set(e, 0.f); df1.set(e, 0.f); }
      }
    }
    if (ds_row_live) store_frag_pair_blocked<T>(dsT + (long)t * DSBLK, df0, df1, li, h, true);
    stored = ds_row_live;
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2 % K::NBUF>;
  for (int t = t0; t < ntiles; t += K::NBUF) {
    tile(I0{}, t);
    if (t + 1 < ntiles) tile(I1{}, t + 1);
    if (K::NBUF == 3 && t + 2 < ntiles) tile(I2{}, t + 2);
  }

  {
    // row index and lane half are derived again from an opaque copy of the lane id: kept from before the loop they cost registers across
    // it, i.e. a scratch slot (harmless, outside the loop, but the loop's budget is exactly the register file)
    int lane2 = lane;
    asm volatile("" : "+v"(lane2));
    const int li2 = lane2 & 31, h2 = lane2 >> 5;
    const int key2 = key0 + wave * 32 + li2;
    const bool kvalid = key2 < sep;
    const int kc = min(key2, a.S - 1);
    T* outk = dbase + (long)kc * rs + a.E + hd * D;
    T* outv = dbase + (long)kc * rs + 2 * a.E + hd * D;
#pragma unroll
    for (int db = 0; db < C::NDB; ++db) {
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = dk[db][r] * scale;
      store_row_block<T>(outk + db * 32, v, h2, kvalid);
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = dv[db][r] * dscale;
      store_row_block<T>(outv + db * 32, v, h2, kvalid);
    }
  }
}

// =============================================================================================
// backward, query-block pass: dQ = scale * dS K over the train keys, from the dS^T the key-block pass stored
// (one product unit, no softmax arithmetic), plus the self-key terms of the test rows (dQ_i, dK_i, dV_i, i >= sep).
// A workgroup owns QBLK queries (lane <-> query) and streams key tiles: dS^T[keys][its queries] and K[keys][D]
// both land in LDS as column images (rows = the contraction index) and are read transposed:
//     dQ^T[d][i] += K^T[d][j] dS^T[j][i]
// Reads 2 bytes per (query, key) pair: HBM-bound (449 MB per launch at the north star against 56 GFLOP).  The
// workgroups walk the (dataset, head) pairs in the REVERSE of the key-block pass's order: what that pass wrote last is
// still in the 256 MB Infinity Cache.
// =============================================================================================
template <typename T, int D> struct BwdDqCfg {
  using C = AttnCfg<T, D>;
  // dS^T reaches LDS exactly as the key-block pass stored it: 32 x 32 blocks of 1-KiB panels ([32 keys][32 bytes of queries],
  // store_frag_pair_blocked).  A wave multiplies only ITS 32 queries, i.e. one block column, so each wave copies its own
  // KVB/32 blocks of a key tile -- contiguous kilobytes, one whole-line LDS-DMA instruction per panel -- into a private ring and
  // reads its fragments straight from the panels (the transposing LDS read wants 4 key rows x 32 bytes, which is a panel's shape).
  // (The first version gathered a [keys][256 queries] image for the whole workgroup: every DMA instruction then touched ~28
  // cache lines for 32 bytes each.)  The tiles come from HBM and the MFMAs of a tile (0.5 us) are far shorter than a fetch, so
  // THREE tiles rotate (two in flight under the one being multiplied); the K tiles, shared by the workgroup and by the eight
  // query blocks of a head through L2, keep two in a column image.
  static constexpr int BLK = 32 * 32 * (int)sizeof(T);        // bytes of one block
  static constexpr int DSW = (C::KVB / 32) * BLK;             // one wave's dS^T bytes per key tile
  static constexpr int NPW = DSW / 1024;                      // ... = its DMA instructions per tile
  static constexpr int NDS = 3, NK = 2;
  static constexpr int NPK = C::CIMG / 1024, NIK = (NPK + C::NW - 1) / C::NW;
  static constexpr int RING = C::NW * NDS * DSW + NK * C::CIMG;
  static constexpr int TSELF = C::NW * 32 * (C::RB + 16);     // the self-key tail's image (re-uses the tile buffers after the loop)
  static constexpr int LDS = RING > TSELF ? RING : TSELF;
  static_assert(C::CIMG % 1024 == 0, "dQ-pass K image must be whole DMA pieces");
};

// dS^T fragment (contraction = keys k0 .. k0+15 of the tile, columns = the wave's 32 queries) from the wave's private copy of its blocks
template <typename T> PFN_DEV Frag<T> load_frag_ds_blocked(const lds_char* blocks, int k0) {
  const int l = lane_id(), h = l >> 5;
  const lds_char* blk = blocks + (k0 >> 5) * (32 * 32 * (int)sizeof(T));
  const int r0 = (k0 & 31) + 8 * h;
  Frag<T> f;
  if constexpr (sizeof(T) == 2) {
    const int i = l & 15, g = (l >> 4) & 1;
    const lds_char* p = blk + g * 1024 + (r0 + (i >> 2)) * 32 + 8 * (i & 3);
    const auto lo = ds_read_tr16_b64<T>(p), hi = ds_read_tr16_b64<T>(p + 4 * 32);
    f.v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  } else {
    const int n = l & 31;
    const lds_char* p = blk + (n >> 3) * 1024 + (n & 7) * 4;
#pragma unroll
    for (int e = 0; e < 8; ++e) f.v[e] = lds_read_f32(p + (r0 + e) * 32);
  }
  return f;
}

template <typename T, int D, bool DROP = false>
__global__ __launch_bounds__((AttnCfg<T, D>::NT)) void attn_bwd_dq_kernel(AttnArgs a) {
  operand_store_mode<T>();
  using C = AttnCfg<T, D>;
  using Q = BwdDqCfg<T, D>;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  LdsPtr smem = lds_cast(smem_raw);
  auto Kc = [&](int slot) { return smem + C::NW * Q::NDS * Q::DSW + slot * C::CIMG; };

  AttnBlock wg = attn_block((a.S + C::QBLK - 1) / C::QBLK - a.q_begin / C::QBLK, a.H);
  wg.blk += a.q_begin / C::QBLK;    // (q_begin: AttnArgs; the launcher zero-fills the dQ rows below it)
  wg.b = a.B - 1 - wg.b;            // most recently written dS^T first (see above)
  wg.hd = a.H - 1 - wg.hd;
  const int b = wg.b, hd = wg.hd;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, li = lane & 31;
  const long rs = 3L * a.E;
  const T* base = reinterpret_cast<const T*>(a.qkv) + (long)b * a.S * rs;
  const T* Qp = base + hd * D;
  const T* Kp = base + a.E + hd * D;
  const T* Vp = base + 2 * a.E + hd * D;
  T* dbase = reinterpret_cast<T*>(a.dqkv) + (long)b * a.S * rs;
  const int q0 = wg.blk * C::QBLK;
  const int qi = q0 + wave * 32 + li;
  const bool qvalid = qi < a.S;
  const int qc = min(qi, a.S - 1);
  const int sep = a.sep_of ? a.sep_of[b] : a.sep;
  if (a.q_from_sep && (wg.blk + 1) * C::QBLK <= sep / 256 * 256) return;      // (as the forward: the launcher zero-fills those dQ rows)
  const float scale = rsqrtf((float)D);
  const float scale_log2 = scale * LOG2E;
  f32x16 dq[C::NDB];
#pragma unroll
  for (int db = 0; db < C::NDB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[db][r] = 0.f;

  // Key tiles go global -> LDS by LDS-DMA issued from assembly (pfn_device.h dma16), no staging registers: the wave's dS^T blocks
  // verbatim into its ring (BwdDqCfg), the K tile into a column image shared by the workgroup.  Rows of keys >= sep: the key-block
  // pass stored zeros for them (dS^T), the descriptor's range ends at sep (K).  At the top of tile t the K tile t+1 and then the
  // dS^T tile t+2 are issued; the end of tile t waits for everything EXCEPT that last dS^T tile (vmcnt = its instruction count:
  // loads return in order), so a dS^T fetch has two tile times to arrive.  (One tile ahead, the pass ran at 3.4 TB/s.)
  const long ds_bh = ((long)b * a.H + hd) * a.ds_rows * a.ds_ld;
  const DmaRsrc rd = make_dma_rsrc(reinterpret_cast<const T*>(a.ds) + ds_bh, (long)a.ds_rows * a.ds_ld * (long)sizeof(T));
  const DmaRsrc rk = make_dma_rsrc(Kp, ((long)(sep - 1) * rs + D) * (long)sizeof(T));   // rows >= sep read as zero
  const int uwave = __builtin_amdgcn_readfirstlane(wave);
  LdsPtr dsw = smem + uwave * Q::NDS * Q::DSW;                 // this wave's ring
  const int blocks_per_row = a.ds_ld / 32;
  const int pvd = (q0 / 32 + uwave) * Q::BLK + lane * 16;      // the wave's block column; + key block row * blocks_per_row * BLK
  int pvk[Q::NIK];                                             // K image: row = key, 16-byte chunks of the head's D columns
#pragma unroll
  for (int i = 0; i < Q::NIK; ++i) {
    const int byte = (uwave + C::NW * i) * 1024 + lane * 16;
    const int row = byte / C::CS, cb = byte % C::CS;
    pvk[i] = cb < C::RB ? row * (int)(rs * sizeof(T)) + cb : BUF_OOB;
  }
  const int ntiles = (sep + C::KVB - 1) / C::KVB;
  const int row_bytes = blocks_per_row * Q::BLK, tile_k_bytes = C::KVB * (int)(rs * sizeof(T));
  auto dma_ds = [&](int slot, int t) {
#pragma unroll
    for (int i = 0; i < Q::NPW; ++i)      // piece i: block row i / (BLK / 1024) of the tile, KiB i % (BLK / 1024) of that block
      dma16(rd, dsw + slot * Q::DSW + i * 1024, pvd + (t * (C::KVB / 32) + i / (Q::BLK / 1024)) * row_bytes + (i % (Q::BLK / 1024)) * 1024);
  };
  auto dma_k = [&](int slot, int t) {
#pragma unroll
    for (int i = 0; i < Q::NIK; ++i)
      if (uwave + C::NW * i < Q::NPK) dma16(rk, Kc(slot) + (uwave + C::NW * i) * 1024, pvk[i] + t * tile_k_bytes);
  };
  constexpr int my_ds_pieces = Q::NPW;
  auto wait_all_but = [&](int n) {     // vmcnt(n): everything but the n most recent loads has landed (n is wave-uniform)
    switch (n) {
#define PFN_VMW(N) case N: __builtin_amdgcn_s_waitcnt(0x0F70 | N); asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
      PFN_VMW(1) PFN_VMW(2) PFN_VMW(3) PFN_VMW(4) PFN_VMW(5) PFN_VMW(6) PFN_VMW(7) PFN_VMW(8) PFN_VMW(9) PFN_VMW(10)
#undef PFN_VMW
      default: dma_wait_all();
    }
  };
  static_assert(Q::NPW <= 10, "piece count per wave exceeds the vmcnt cases above");
  if (ntiles > 0) { dma_k(0, 0); dma_ds(0, 0); }
  if (ntiles > 1) dma_ds(1, 1);
  wait_all_but(ntiles > 1 ? my_ds_pieces : 0);
  __syncthreads();
  int sd = 0, sk = 0;                  // ring slots of tile t
  for (int t = 0; t < ntiles; ++t) {
    const lds_char* dst = dsw + sd * Q::DSW;
    const lds_char* kc = Kc(sk);
    constexpr int NKS = C::KVB / 16;     // contraction steps per tile
    const int sd2 = sd == 0 ? 2 : sd - 1;                      // (t + 2) % 3
    const bool more_ds = t + 2 < ntiles;
    if (t + 1 < ntiles) dma_k(sk ^ 1, t + 1);                  // slots last read in tile t-1: every wave is past that tile's barrier
    if (more_ds) dma_ds(sd2, t + 2);
    Frag<T> dsf[NKS];
#pragma unroll
    for (int c = 0; c < NKS; ++c) dsf[c] = load_frag_ds_blocked<T>(dst, c * 16);
    Frag<T> cf[2][C::NDB];
#pragma unroll
    for (int db = 0; db < C::NDB; ++db) cf[0][db] = load_frag_tr_p<T, C::CS, 1>(kc, 0, db * 32);
    PFN_PIN_LDS_MFMA();
#pragma unroll
    for (int c = 0; c < NKS; ++c) {
      if (c + 1 < NKS) {
#pragma unroll
        for (int db = 0; db < C::NDB; ++db) cf[(c + 1) & 1][db] = load_frag_tr_p<T, C::CS, 1>(kc, (c + 1) * 16, db * 32);
      }
#pragma unroll
      for (int db = 0; db < C::NDB; ++db) dq[db] = mma32(cf[c & 1][db], dsf[c], dq[db]);
      PFN_PIN_LDS_MFMA();
    }
    wait_all_but(more_ds ? my_ds_pieces : 0);
    __syncthreads();
    sd = sd == 2 ? 0 : sd + 1;
    sk ^= 1;
  }

  // ---- self key of the test rows (i >= sep): p_i = exp(q_i.k_i scale - lse_i), ds_i = p_i (dO_i.v_i - delta_i),
  //      dQ_i += ds_i k_i,  dK_i = scale ds_i q_i,  dV_i = p_i dO_i
  // Only waves that hold a test row do this.  The rows are walked with the lanes ALONG a row (64 / CPR rows per step, CPR lanes of
  // 16 bytes each on a row): every load and store instruction covers whole rows -- with one row per lane (the accumulator
  // layout) each instruction touched 32 to 64 different cache lines and this tail cost 32 us of the pass's 144.  ds_i k_i reaches
  // the accumulator layout through a wave-private LDS image (the tile buffers are free after the loop).
  const bool wave_has_test = q0 + wave * 32 + 31 >= sep;
  constexpr int TS = C::RB + 16;                       // row stride of the self-term image
  LdsPtr tself = smem + wave * 32 * TS;
  if (wave_has_test) {
    constexpr int CPR = C::RB / 16, RPS = 64 / CPR, NST = 32 / RPS, EPC = 16 / (int)sizeof(T);
    const int rsub = lane / CPR, c = lane % CPR;
    const T* dOb = reinterpret_cast<const T*>(a.dctx) + (long)b * a.S * a.E + hd * D;
    const float* lse_g = a.lse + ((long)b * a.H + hd) * a.S;
    const float* delta_g = a.delta + ((long)b * a.H + hd) * a.S;
    auto unpack = [](const u32x4& raw, float (&x)[EPC]) {
      if constexpr (sizeof(T) == 2) {
        const X8<T> v = __builtin_bit_cast(X8<T>, raw);
#pragma unroll
        for (int e = 0; e < EPC; ++e) x[e] = (float)v[e];
      } else {
        const f32x4 v = __builtin_bit_cast(f32x4, raw);
#pragma unroll
        for (int e = 0; e < EPC; ++e) x[e] = v[e];
      }
    };
    auto pack = [](const float (&x)[EPC]) {
      if constexpr (sizeof(T) == 2) {
        X8<T> v;
#pragma unroll
        for (int e = 0; e < EPC; ++e) v[e] = (T)x[e];
        return __builtin_bit_cast(u32x4, v);
      } else {
        return __builtin_bit_cast(u32x4, f32x4{x[0], x[1], x[2], x[3]});
      }
    };
    // every load first, then every store: the compiler cannot prove that the dqkv rows written below do not alias the qkv /
    // dctx rows read here, so a load placed after a store waits for it -- eight dependent round trips instead of one
    u32x4 rq_[NST], rk_[NST], rv_[NST], ro_[NST];
    float rl_[NST], rd_[NST];
#pragma unroll
    for (int st = 0; st < NST; ++st) {
      const int qcl = min(q0 + wave * 32 + st * RPS + rsub, a.S - 1);
      rq_[st] = *reinterpret_cast<const u32x4*>(Qp + (long)qcl * rs + c * EPC);
      rk_[st] = *reinterpret_cast<const u32x4*>(Kp + (long)qcl * rs + c * EPC);
      rv_[st] = *reinterpret_cast<const u32x4*>(Vp + (long)qcl * rs + c * EPC);
      ro_[st] = *reinterpret_cast<const u32x4*>(dOb + (long)qcl * a.E + c * EPC);
      rl_[st] = lse_g[qcl];
      rd_[st] = delta_g[qcl];
    }
#pragma unroll
    for (int st = 0; st < NST; ++st) {
      const int row = st * RPS + rsub;
      const int q = q0 + wave * 32 + row;
      const bool test = q >= sep && q < a.S;
      float qv[EPC], kv[EPC], vv[EPC], dv_[EPC];
      unpack(rq_[st], qv);
      unpack(rk_[st], kv);
      unpack(rv_[st], vv);
      unpack(ro_[st], dv_);
      float tq = 0.f, dpv = 0.f;
#pragma unroll
      for (int e = 0; e < EPC; ++e) { tq += qv[e] * kv[e]; dpv += dv_[e] * vv[e]; }
#pragma unroll
      for (int off = 1; off < CPR; off <<= 1) { tq += __shfl_xor(tq, off, 64); dpv += __shfl_xor(dpv, off, 64); }
      const float p_self = test ? fast_exp2(tq * scale_log2 - rl_[st] * LOG2E) : 0.f;
      float mfac = 1.f;      // DROP: keep(i, i) / (1 - p) of the self key's probability
      if constexpr (DROP)
        mfac = dropout_keep(dropout_pair_seed(a.drop_seed, b * a.H + hd), (unsigned)q, (unsigned)q, dropout_threshold(a.p_drop)) ? 1.f / (1.f - a.p_drop) : 0.f;
      const float ds_self = p_self * (mfac * dpv - rd_[st]);
      float xk[EPC], xv[EPC], xt[EPC];
#pragma unroll
      for (int e = 0; e < EPC; ++e) { xk[e] = ds_self * scale * qv[e]; xv[e] = p_self * mfac * dv_[e]; xt[e] = ds_self * kv[e]; }
      if (test) {
        *reinterpret_cast<u32x4*>(dbase + (long)q * rs + a.E + hd * D + c * EPC) = pack(xk);
        *reinterpret_cast<u32x4*>(dbase + (long)q * rs + 2 * a.E + hd * D + c * EPC) = pack(xv);
      }
      lds_write16(tself + row * TS + c * 16, pack(xt));
    }
  }
  {
    T* dQo = dbase + (long)qc * rs + hd * D;
#pragma unroll
    for (int db = 0; db < C::NDB; ++db) {
      float v[16];
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int d0 = db * 32 + 8 * rg + 4 * h;
        f32x4 ts = {0.f, 0.f, 0.f, 0.f};
        if (wave_has_test) {   // (the wave's own LDS writes above are ordered before these reads)
          if constexpr (sizeof(T) == 2) {
            const X4<T> t4 = *reinterpret_cast<const __attribute__((address_space(3))) X4<T>*>(tself + li * TS + d0 * 2);
#pragma unroll
            for (int e = 0; e < 4; ++e) ts[e] = (float)t4[e];
          } else {
            ts = __builtin_bit_cast(f32x4, lds_read16(tself + li * TS + d0 * 4));
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * rg + e] = (dq[db][4 * rg + e] + ts[e]) * scale;
      }
      store_row_block<T>(dQo + db * 32, v, h, qvalid);
    }
  }
  // delta of the wave's 32 queries has had its last reader (the key-block pass before this launch, the self-key term above): cleared for the next layer's
  // GEMM epilogue, which ADDS into it (EPI_ROWDOT; AttnArgs::zero_delta)
  if (a.zero_delta && h == 0 && qvalid) a.delta[((long)b * a.H + hd) * a.S + qi] = 0.f;
}

// =============================================================================================
// backward, exact-f32 mode at head dim 256: plain vector-ALU kernels.
//
// The MFMA backward above keeps a key block's V rows (or, in the 4-wave configurations, the K and V fragments of 256 f32 columns) beside two tile
// buffers; in f32 at head dim 256 neither fits (V image alone 256 KiB).  `precision='f32'` is the parity mode -- the reference trains in fp32
// everywhere (train.py:93, transformer.py:17-18) and this mode exists so that a layout or algorithm mistake shows at 1e-6 instead of hiding under
// bf16 rounding -- so at this head dim the backward runs as two plain tiled kernels on f32 FMAs (no matrix instructions, no dS^T scratch: the
// query pass recomputes S and dP).  Same contract as launch_bwd_k: lse / delta from attn_delta_kernel, queries below q_begin skipped (their dQ rows
// zero-filled by the launcher), dK / dV rows of the test keys (>= sep) come from the self-key term of the query pass.
//   key pass   : a workgroup owns 32 keys and streams the queries in tiles of 32:  S, dP -> P, dS (LDS) -> dV += P^T dO, dK += dS^T Q
//   query pass : a workgroup owns 32 queries and streams the keys  in tiles of 32:  S, dP -> dS (LDS)   -> dQ += dS K;  + the self key of a test row
// Thread t of 256: phase 1 computes the (query t / 8, keys 4 (t % 8) .. + 3) entries of the 32 x 32 tile; phase 2 owns output row t / 8, columns
// 4 (t % 8) + 32 m .. + 3 (m < D / 32).  Not a throughput path: ~3.5 kFLOP per (query, key) pair at the vector rate.
// =============================================================================================
template <int D> struct BwdPlainCfg {
  static constexpr int TB = 32;                       // tile: 32 queries x 32 keys
  static constexpr int RS = D + 4;                    // LDS row stride in floats (16-byte aligned rows, rows 4 banks apart)
  static constexpr int TILE = TB * RS;                // floats of one [32][D] tile
  static constexpr int PS = TB + 1;                   // P / dS tile row stride
  static constexpr int LDS = (4 * TILE + 2 * TB * PS + 2 * TB) * 4;    // Q, dO, K, V tiles; P, dS; lse, delta
};

template <int D> PFN_DEV void plain_load_tile(float* dst, const float* src, long ld, int row0, int row_lo, int row_hi) {
  // rows [row0, row0 + 32) of a [*, ld] matrix (D columns from src) -> dst[32][RS]; rows outside [row_lo, row_hi) read as zero
  using P = BwdPlainCfg<D>;
  for (int c = threadIdx.x; c < P::TB * (D / 4); c += 256) {
    const int r = c / (D / 4), c4 = c % (D / 4), row = row0 + r;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row >= row_lo && row < row_hi) v = *reinterpret_cast<const f32x4*>(src + (long)row * ld + c4 * 4);
    *reinterpret_cast<f32x4*>(dst + r * P::RS + c4 * 4) = v;
  }
}

// phase 1 of both passes: s[j] = q_row . k_rows[kj0 + j], dp[j] = do_row . v_rows[kj0 + j]
template <int D> PFN_DEV void plain_dots(const float* qrow, const float* orow, const float* Ks, const float* Vs, int kj0, float (&s)[4], float (&dp)[4]) {
  using P = BwdPlainCfg<D>;
#pragma unroll
  for (int j = 0; j < 4; ++j) { s[j] = 0.f; dp[j] = 0.f; }
  for (int d = 0; d < D; d += 4) {
    const f32x4 q4 = *reinterpret_cast<const f32x4*>(qrow + d), o4 = *reinterpret_cast<const f32x4*>(orow + d);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 k4 = *reinterpret_cast<const f32x4*>(Ks + (kj0 + j) * P::RS + d), v4 = *reinterpret_cast<const f32x4*>(Vs + (kj0 + j) * P::RS + d);
      s[j] += q4[0] * k4[0] + q4[1] * k4[1] + q4[2] * k4[2] + q4[3] * k4[3];
      dp[j] += o4[0] * v4[0] + o4[1] * v4[1] + o4[2] * v4[2] + o4[3] * v4[3];
    }
  }
}

template <int D>
__global__ __launch_bounds__(256) void attn_bwd_plain_kv_kernel(AttnArgs a) {
  using P = BwdPlainCfg<D>;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* Qs = reinterpret_cast<float*>(smem_raw);
  float* Os = Qs + P::TILE; float* Ks = Os + P::TILE; float* Vs = Ks + P::TILE;
  float* Ps = Vs + P::TILE; float* Ds = Ps + P::TB * P::PS; float* Ls = Ds + P::TB * P::PS; float* Dl = Ls + P::TB;
  const int nkb = (a.sep + P::TB - 1) / P::TB;
  const int kb = blockIdx.x % nkb, hd = (blockIdx.x / nkb) % a.H, b = blockIdx.x / (nkb * a.H);
  const long rs = 3L * a.E;
  const float* base = reinterpret_cast<const float*>(a.qkv) + (long)b * a.S * rs;
  const float* Qp = base + hd * D; const float* Kp = base + a.E + hd * D; const float* Vp = base + 2 * a.E + hd * D;
  const float* dOp = reinterpret_cast<const float*>(a.dctx) + (long)b * a.S * a.E + hd * D;
  float* dbase = reinterpret_cast<float*>(a.dqkv) + (long)b * a.S * rs;
  const float* lse_g = a.lse + ((long)b * a.H + hd) * a.S;
  const float* delta_g = a.delta + ((long)b * a.H + hd) * a.S;
  const int key0 = kb * P::TB, t = threadIdx.x, r1 = t >> 3, c1 = (t & 7) * 4;
  const int sep = a.sep_of ? a.sep_of[b] : a.sep;
  if (key0 >= sep) return;      // (ragged batch: the grid covers the largest position)
  const int qbeg = a.q_from_sep ? sep / 256 * 256 : a.q_begin;
  const float scale = rsqrtf((float)D), scale_log2 = scale * LOG2E;
  // dropout on the probabilities (as in attn_bwd_kv_kernel): dV takes P' = P keep / (1 - p), dP = (dO V^T) keep / (1 - p), dS = P (dP - delta) with the unmasked P
  const bool drop = a.p_drop > 0.f;
  const unsigned dseed = dropout_pair_seed(a.drop_seed, b * a.H + hd), dthr = dropout_threshold(a.p_drop);
  const float dscale = drop ? 1.f / (1.f - a.p_drop) : 1.f;
  plain_load_tile<D>(Ks, Kp, rs, key0, 0, sep);
  plain_load_tile<D>(Vs, Vp, rs, key0, 0, sep);
  f32x4 dk[D / 32], dv[D / 32];
#pragma unroll
  for (int m = 0; m < D / 32; ++m) { dk[m] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[m] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  for (int q0 = qbeg / P::TB * P::TB; q0 < a.S; q0 += P::TB) {
    __syncthreads();                                   // the previous tile's phase 2 has read Qs / Os / Ps / Ds (first tile: K / V tiles written)
    plain_load_tile<D>(Qs, Qp, rs, q0, qbeg, a.S);
    plain_load_tile<D>(Os, dOp, a.E, q0, qbeg, a.S);
    if (t < P::TB) { const int q = min(q0 + t, a.S - 1); Ls[t] = lse_g[q] * LOG2E; Dl[t] = delta_g[q]; }
    __syncthreads();
    {
      float s[4], dp[4];
      plain_dots<D>(Qs + r1 * P::RS, Os + r1 * P::RS, Ks, Vs, c1, s, dp);
      const int q = q0 + r1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = q >= qbeg && q < a.S && key0 + c1 + j < sep;
        const float p = live ? fast_exp2(s[j] * scale_log2 - Ls[r1]) : 0.f;
        const float mf = !drop ? 1.f : dropout_keep(dseed, (unsigned)q, (unsigned)(key0 + c1 + j), dthr) ? dscale : 0.f;
        Ps[r1 * P::PS + c1 + j] = p * mf;
        Ds[r1 * P::PS + c1 + j] = p * (mf * dp[j] - Dl[r1]);
      }
    }
    __syncthreads();
    for (int qi = 0; qi < P::TB; ++qi) {               // thread: key r1, columns c1 + 32 m
      const float p = Ps[qi * P::PS + r1], ds = Ds[qi * P::PS + r1];
#pragma unroll
      for (int m = 0; m < D / 32; ++m) {
        const f32x4 o4 = *reinterpret_cast<const f32x4*>(Os + qi * P::RS + c1 + 32 * m), q4 = *reinterpret_cast<const f32x4*>(Qs + qi * P::RS + c1 + 32 * m);
#pragma unroll
        for (int e = 0; e < 4; ++e) { dv[m][e] += p * o4[e]; dk[m][e] += ds * q4[e]; }
      }
    }
  }
  const int key = key0 + r1;
  if (key < sep) {
#pragma unroll
    for (int m = 0; m < D / 32; ++m) {
      f32x4 k4;
#pragma unroll
      for (int e = 0; e < 4; ++e) k4[e] = dk[m][e] * scale;
      *reinterpret_cast<f32x4*>(dbase + (long)key * rs + a.E + hd * D + c1 + 32 * m) = k4;
      *reinterpret_cast<f32x4*>(dbase + (long)key * rs + 2 * a.E + hd * D + c1 + 32 * m) = dv[m];
    }
  }
}

template <int D>
__global__ __launch_bounds__(256) void attn_bwd_plain_dq_kernel(AttnArgs a) {
  using P = BwdPlainCfg<D>;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* Qs = reinterpret_cast<float*>(smem_raw);
  float* Os = Qs + P::TILE; float* Ks = Os + P::TILE; float* Vs = Ks + P::TILE;
  float* Ps = Vs + P::TILE; float* Ds = Ps + P::TB * P::PS; float* Ls = Ds + P::TB * P::PS; float* Dl = Ls + P::TB;
  const int qb0 = a.q_begin / P::TB, nqb = (a.S + P::TB - 1) / P::TB - qb0;
  const int qb = qb0 + blockIdx.x % nqb, hd = (blockIdx.x / nqb) % a.H, b = blockIdx.x / (nqb * a.H);
  const long rs = 3L * a.E;
  const float* base = reinterpret_cast<const float*>(a.qkv) + (long)b * a.S * rs;
  const float* Qp = base + hd * D; const float* Kp = base + a.E + hd * D; const float* Vp = base + 2 * a.E + hd * D;
  const float* dOp = reinterpret_cast<const float*>(a.dctx) + (long)b * a.S * a.E + hd * D;
  float* dbase = reinterpret_cast<float*>(a.dqkv) + (long)b * a.S * rs;
  const float* lse_g = a.lse + ((long)b * a.H + hd) * a.S;
  const float* delta_g = a.delta + ((long)b * a.H + hd) * a.S;
  const int q0 = qb * P::TB, t = threadIdx.x, r1 = t >> 3, c1 = (t & 7) * 4;
  const int sep = a.sep_of ? a.sep_of[b] : a.sep;
  const int qbeg = a.q_from_sep ? sep / 256 * 256 : a.q_begin;
  if ((qb + 1) * P::TB <= qbeg) return;      // (ragged batch: the grid starts at the smallest first block; the launcher zero-fills these dQ rows)
  const float scale = rsqrtf((float)D), scale_log2 = scale * LOG2E;
  const bool drop = a.p_drop > 0.f;
  const unsigned dseed = dropout_pair_seed(a.drop_seed, b * a.H + hd), dthr = dropout_threshold(a.p_drop);
  const float dscale = drop ? 1.f / (1.f - a.p_drop) : 1.f;
  plain_load_tile<D>(Qs, Qp, rs, q0, qbeg, a.S);
  plain_load_tile<D>(Os, dOp, a.E, q0, qbeg, a.S);
  if (t < P::TB) { const int q = min(q0 + t, a.S - 1); Ls[t] = lse_g[q] * LOG2E; Dl[t] = delta_g[q]; }
  f32x4 dq[D / 32];
#pragma unroll
  for (int m = 0; m < D / 32; ++m) dq[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int q = q0 + r1;
  const bool qlive = q >= qbeg && q < a.S;
  for (int key0 = 0; key0 < sep; key0 += P::TB) {
    __syncthreads();
    plain_load_tile<D>(Ks, Kp, rs, key0, 0, sep);
    plain_load_tile<D>(Vs, Vp, rs, key0, 0, sep);
    __syncthreads();
    {
      float s[4], dp[4];
      plain_dots<D>(Qs + r1 * P::RS, Os + r1 * P::RS, Ks, Vs, c1, s, dp);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = qlive && key0 + c1 + j < sep;
        const float p = live ? fast_exp2(s[j] * scale_log2 - Ls[r1]) : 0.f;
        const float mf = !drop ? 1.f : dropout_keep(dseed, (unsigned)q, (unsigned)(key0 + c1 + j), dthr) ? dscale : 0.f;
        Ds[r1 * P::PS + c1 + j] = p * (mf * dp[j] - Dl[r1]);
      }
    }
    __syncthreads();
    for (int kj = 0; kj < P::TB; ++kj) {               // thread: query r1, columns c1 + 32 m
      const float ds = Ds[r1 * P::PS + kj];
#pragma unroll
      for (int m = 0; m < D / 32; ++m) {
        const f32x4 k4 = *reinterpret_cast<const f32x4*>(Ks + kj * P::RS + c1 + 32 * m);
#pragma unroll
        for (int e = 0; e < 4; ++e) dq[m][e] += ds * k4[e];
      }
    }
  }
  // ---- the self key of a test row (i >= sep), as in attn_bwd_dq_kernel: p_i = exp(q_i.k_i scale - lse_i), ds_i = p_i (dO_i.v_i - delta_i),
  //      dQ_i += ds_i k_i,  dK_i = scale ds_i q_i,  dV_i = p_i dO_i.  The 8 threads of a row hold partial dots over their columns.
  __syncthreads();                                     // (sep == 0: the Q / dO tiles and Ls / Dl written above)
  const bool test = qlive && q >= sep;
  const int qc = min(max(q, 0), a.S - 1);
  float tq = 0.f, dpv = 0.f;
  f32x4 kself[D / 32], vself[D / 32];
#pragma unroll
  for (int m = 0; m < D / 32; ++m) {
    kself[m] = *reinterpret_cast<const f32x4*>(Kp + (long)qc * rs + c1 + 32 * m);
    vself[m] = *reinterpret_cast<const f32x4*>(Vp + (long)qc * rs + c1 + 32 * m);
    const f32x4 q4 = *reinterpret_cast<const f32x4*>(Qs + r1 * P::RS + c1 + 32 * m), o4 = *reinterpret_cast<const f32x4*>(Os + r1 * P::RS + c1 + 32 * m);
#pragma unroll
    for (int e = 0; e < 4; ++e) { tq += q4[e] * kself[m][e]; dpv += o4[e] * vself[m][e]; }
  }
#pragma unroll
  for (int off = 1; off < 8; off <<= 1) { tq += __shfl_xor(tq, off, 64); dpv += __shfl_xor(dpv, off, 64); }
  const float p_self = test ? fast_exp2(tq * scale_log2 - Ls[r1]) : 0.f;
  const float mself = !drop ? 1.f : dropout_keep(dseed, (unsigned)max(q, 0), (unsigned)max(q, 0), dthr) ? dscale : 0.f;      // keep(i, i) / (1 - p) of the self key
  const float ds_self = p_self * (mself * dpv - Dl[r1]);
  if (qlive) {
#pragma unroll
    for (int m = 0; m < D / 32; ++m) {
      const f32x4 q4 = *reinterpret_cast<const f32x4*>(Qs + r1 * P::RS + c1 + 32 * m), o4 = *reinterpret_cast<const f32x4*>(Os + r1 * P::RS + c1 + 32 * m);
      f32x4 xq, xk, xv;
#pragma unroll
      for (int e = 0; e < 4; ++e) { xq[e] = (dq[m][e] + ds_self * kself[m][e]) * scale; xk[e] = ds_self * scale * q4[e]; xv[e] = p_self * mself * o4[e]; }
      *reinterpret_cast<f32x4*>(dbase + (long)q * rs + hd * D + c1 + 32 * m) = xq;
      if (test) {
        *reinterpret_cast<f32x4*>(dbase + (long)q * rs + a.E + hd * D + c1 + 32 * m) = xk;
        *reinterpret_cast<f32x4*>(dbase + (long)q * rs + 2 * a.E + hd * D + c1 + 32 * m) = xv;
      }
    }
  }
}

// =============================================================================================
// launchers
// =============================================================================================
bool attn_fwd_can_fuse_q(int E, int H, int precision) {
  const int D = H > 0 ? E / H : 0;
  return prec_is16(precision) && (D == 32 || D == 64 || D == 128) && E % 128 == 0;
}
template <typename T, int D, bool DROP> static int launch_fwd_k(const AttnArgs& a, hipStream_t s) {
  using C = AttnCfg<T, D>;
  // exact-f32 at head dim 256: the V / O columns in two slices of 128 (attn_fwd_kernel, DV)
  constexpr int DV = (sizeof(T) == 4 && D == 256) ? 128 : D;
  constexpr size_t lds = 2 * C::RIMG + 4 * AttnCfg<T, DV>::CIMG;
  static_assert(lds <= 160 * 1024, "attention forward: tile buffers exceed the CU's LDS");
  if ((a.S + C::QBLK - 1) / C::QBLK <= a.q_begin / C::QBLK) return PFN_OK;      // no query at or above q_begin
  const dim3 grid(((a.S + C::QBLK - 1) / C::QBLK - a.q_begin / C::QBLK) * a.H * a.B, D / DV);
  if constexpr (sizeof(T) == 2 && D <= 128 && !DROP) {
    if (a.xq) {      // the Q projection inside the kernel (AttnArgs::xq)
      if (!a.wq || !a.bq || a.E % 128) return PFN_ERR_ARGUMENT;
      static LdsAllowance allowance_q;
      allowance_q.ensure(attn_fwd_kernel<T, D, false, DV, true>, lds);
      ProfScope ps(PFN_PROF_ATTN_FWD + (a.q_begin > 0 ? 1 : 0), s);
      hipLaunchKernelGGL((attn_fwd_kernel<T, D, false, DV, true>), grid, dim3(C::NT), lds, s, a);
      return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
    }
  }
  if (a.xq) return PFN_ERR_UNSUPPORTED;
  static LdsAllowance allowance;
  allowance.ensure(attn_fwd_kernel<T, D, DROP, DV>, lds);
  ProfScope ps(PFN_PROF_ATTN_FWD + (a.q_begin > 0 ? 1 : 0), s);
  hipLaunchKernelGGL((attn_fwd_kernel<T, D, DROP, DV>), grid, dim3(C::NT), lds, s, a);
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}
template <typename T, int D> static int launch_fwd_t(const AttnArgs& a, hipStream_t s) {
  return a.p_drop > 0.f ? launch_fwd_k<T, D, true>(a, s) : launch_fwd_k<T, D, false>(a, s);     // dropout: the variants with the mask arithmetic
}
static int g_attn_cache_split_cap = 0;      // PFN_TUNE_ATTN_CACHE_SPLITS
void set_attn_cache_split_cap(int splits) { g_attn_cache_split_cap = std::max(splits, 0); }
// predict against a K / V cache: the forward kernel's CACHE instantiation over gridDim.z = attn_cache_splits key ranges, merged by attn_merge_kernel when there are several
template <typename T, int D> static int launch_fwd_cache_t(const AttnArgs& a_in, hipStream_t s) {
  using C = AttnCfg<T, D>;
  constexpr int DV = (sizeof(T) == 4 && D == 256) ? 128 : D;
  constexpr size_t lds = 2 * C::RIMG + 4 * AttnCfg<T, DV>::CIMG;
  AttnArgs a = a_in;
  int nsplit = attn_cache_splits(a.B, a.S, a.E, a.H, a.sep, sizeof(T) == 4 ? PFN_PREC_F32 : PFN_PREC_BF16);
  if (g_attn_cache_split_cap > 0) nsplit = std::min(nsplit, g_attn_cache_split_cap);
  const int ntiles = (a.sep + C::KVB - 1) / C::KVB;
  a.split_keys = nsplit > 1 ? (ntiles + nsplit - 1) / nsplit * C::KVB : std::max(a.sep, 1);
  const int nz = nsplit > 1 ? (a.sep + a.split_keys - 1) / a.split_keys : 1;      // (whole tiles per split: the last ones may merge)
  if (nz > 1 && (!a.part_o || !a.part_ml)) return PFN_ERR_ARGUMENT;
  static LdsAllowance allowance;
  allowance.ensure(attn_fwd_kernel<T, D, false, DV, false, true>, lds);
  const dim3 grid(((a.S + C::QBLK - 1) / C::QBLK) * a.H * a.B, D / DV, nz);
  hipLaunchKernelGGL((attn_fwd_kernel<T, D, false, DV, false, true>), grid, dim3(C::NT), lds, s, a);
  if (nz > 1) {
    const long work = (long)a.B * a.S * (a.E / 4);
    hipLaunchKernelGGL(attn_merge_kernel<T>, dim3((unsigned)std::min<long>((work + 255) / 256, 4096)), dim3(256), 0, s, a, nz, D);
  }
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}
template <typename T, int D, bool DROP> static int launch_bwd_k(const AttnArgs& a, hipStream_t s) {
  using C = AttnCfg<T, D>;
  const int parts = a.parts ? a.parts : ~0;
  if (parts & ATTN_BWD_DELTA) {
    const long pairs = (long)a.B * a.S * a.H;
    int grid = (int)std::min<long>((pairs + 15) / 16, 4096);
    ProfScope ps(PFN_PROF_ATTN_BWD_DELTA + (a.q_begin > 0 ? 1 : 0), s);
    hipLaunchKernelGGL(attn_delta_kernel<T>, dim3(grid), dim3(256), 0, s, a, D);
  }
  constexpr size_t lds_kv = BwdKvCfg<T, D>::LDS, lds_dq = BwdDqCfg<T, D>::LDS;
  static_assert(lds_kv <= 160 * 1024 && lds_dq <= 160 * 1024, "attention backward: tile buffers exceed the CU's LDS");
  static LdsAllowance allow_kv, allow_dq;      // (per device; hipFuncSetAttribute costs tens of microseconds of host time per call)
  // (Launching the pair for a few datasets at a time into one scratch, so that dS^T -- 436 MB per 16 datasets -- stays in the
  // 256 MB memory-side cache, was measured: 432 vs 436 us with two chunks, slower with more: each launch ends in a partial round.
  // Measured again with every group through the front of the scratch, 25.7 MB per dataset: slower at every group size,
  // profiles/r06_attention_bwd_groups.txt.)
  if ((parts & ATTN_BWD_KV) && a.sep > 0) {
    ProfScope ps(PFN_PROF_ATTN_BWD_KV + (a.q_begin > 0 ? 1 : 0), s);
    allow_kv.ensure(attn_bwd_kv_kernel<T, D, DROP>, lds_kv);
    hipLaunchKernelGGL((attn_bwd_kv_kernel<T, D, DROP>), dim3(((a.sep + C::QBLK - 1) / C::QBLK) * a.H * a.B), dim3(C::NT), lds_kv, s, a);
  }
  if (parts & ATTN_BWD_DQ) {
    if (a.q_from_sep) {       // ragged batch: every dataset's own prefix
      const int rc = launch_zero_row_prefix_ragged(a.dqkv, a.S, a.B, a.sep_of, 3L * a.E * (long)sizeof(T), (long)a.E * (long)sizeof(T), s);
      if (rc != PFN_OK) return rc;
    } else if (a.q_begin > 0) {      // dQ of the skipped queries: zeros (every row of dqkv is read by the GEMMs behind this launch)
      const int rc = launch_zero_row_prefix(a.dqkv, a.S, a.B, a.q_begin, 3L * a.E * (long)sizeof(T), (long)a.E * (long)sizeof(T), s);
      if (rc != PFN_OK) return rc;
    }
    if ((a.S + C::QBLK - 1) / C::QBLK <= a.q_begin / C::QBLK) return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
    allow_dq.ensure(attn_bwd_dq_kernel<T, D, DROP>, lds_dq);
    ProfScope ps(PFN_PROF_ATTN_BWD_DQ + (a.q_begin > 0 ? 1 : 0), s);
    hipLaunchKernelGGL((attn_bwd_dq_kernel<T, D, DROP>), dim3(((a.S + C::QBLK - 1) / C::QBLK - a.q_begin / C::QBLK) * a.H * a.B), dim3(C::NT), lds_dq, s, a);
  }
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}
template <typename T, int D> static int launch_bwd_t(const AttnArgs& a, hipStream_t s) {
  return a.p_drop > 0.f ? launch_bwd_k<T, D, true>(a, s) : launch_bwd_k<T, D, false>(a, s);
}
// exact-f32 mode at head dim 256: the plain kernels (attn_bwd_plain_*)
template <int D> static int launch_bwd_plain_f32(const AttnArgs& a, hipStream_t s) {
  using P = BwdPlainCfg<D>;
  static_assert(P::LDS <= 160 * 1024, "plain attention backward: tiles exceed the CU's LDS");
  const int parts = a.parts ? a.parts : ~0;
  if (parts & ATTN_BWD_DELTA) {
    const long pairs = (long)a.B * a.S * a.H;
    int grid = (int)std::min<long>((pairs + 15) / 16, 4096);
    hipLaunchKernelGGL(attn_delta_kernel<float>, dim3(grid), dim3(256), 0, s, a, D);
  }
  static LdsAllowance allow_kv, allow_dq;
  if ((parts & ATTN_BWD_KV) && a.sep > 0) {
    allow_kv.ensure(attn_bwd_plain_kv_kernel<D>, P::LDS);
    hipLaunchKernelGGL(attn_bwd_plain_kv_kernel<D>, dim3(((a.sep + P::TB - 1) / P::TB) * a.H * a.B), dim3(256), P::LDS, s, a);
  }
  if (parts & ATTN_BWD_DQ) {
    if (a.q_from_sep) {
      const int rc = launch_zero_row_prefix_ragged(a.dqkv, a.S, a.B, a.sep_of, 3L * a.E * 4L, (long)a.E * 4L, s);
      if (rc != PFN_OK) return rc;
    } else if (a.q_begin > 0) {
      const int rc = launch_zero_row_prefix(a.dqkv, a.S, a.B, a.q_begin, 3L * a.E * 4L, (long)a.E * 4L, s);
      if (rc != PFN_OK) return rc;
    }
    const int nqb = (a.S + P::TB - 1) / P::TB - a.q_begin / P::TB;
    if (nqb > 0) {
      allow_dq.ensure(attn_bwd_plain_dq_kernel<D>, P::LDS);
      hipLaunchKernelGGL(attn_bwd_plain_dq_kernel<D>, dim3(nqb * a.H * a.B), dim3(256), P::LDS, s, a);
    }
  }
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

static int check_attn(const AttnArgs& a, int precision) {
  if (a.B <= 0 || a.S <= 0 || a.H <= 0 || a.E % a.H) return PFN_ERR_ARGUMENT;
  if (a.sep < 0 || a.sep > a.S || a.q_begin < 0 || a.q_begin > a.S || (a.q_from_sep && !a.sep_of)) return PFN_ERR_ARGUMENT;
  const int es = prec_esize(precision);
  if ((a.E * es) % 16) return PFN_ERR_ALIGNMENT;
  return PFN_OK;
}

// F32_256: what the exact-f32 mode does at head dim 256 -- the forward runs the MFMA kernel with the V / O columns in two slices, the backward the plain
// vector-ALU kernels (attn_bwd_plain_*: the MFMA backward's tiles do not fit the LDS in f32 at that head dim)
#define PFN_ATTN_DISPATCH(FN, F32_256)                                                    \
  const int D = a.E / a.H;                                                                 \
  if (precision == PFN_PREC_BF16) {                                                        \
    switch (D) {                                                                           \
      case 32: return FN<bf16, 32>(a, s);                                                  \
      case 64: return FN<bf16, 64>(a, s);                                                  \
      case 128: return FN<bf16, 128>(a, s);                                                \
      case 256: return FN<bf16, 256>(a, s);                                                \
      default: return PFN_ERR_UNSUPPORTED;                                                 \
    }                                                                                      \
  } else if (precision == PFN_PREC_FP16) {                                                 \
    switch (D) {                                                                           \
      case 32: return FN<f16, 32>(a, s);                                                   \
      case 64: return FN<f16, 64>(a, s);                                                   \
      case 128: return FN<f16, 128>(a, s);                                                 \
      case 256: return FN<f16, 256>(a, s);                                                 \
      default: return PFN_ERR_UNSUPPORTED;                                                 \
    }                                                                                      \
  } else {                                                                                 \
    switch (D) {                                                                           \
      case 32: return FN<float, 32>(a, s);                                                 \
      case 64: return FN<float, 64>(a, s);                                                 \
      case 128: return FN<float, 128>(a, s);                                               \
      case 256: F32_256;                                                                   \
      default: return PFN_ERR_UNSUPPORTED;                                                 \
    }                                                                                      \
  }

// both bits since round 4: the key-block pass's ping-pong placement measures -2.5 % on the pass alone (profiles/r03_attention_experiments.txt), the whole GPU
// suite is green under it (gpurun call 1 of round 4), and the step is neutral to it (2411 / 2409 vs 2399 / 2414 datasets/s, same box)
static int g_attn_pingpong = 3;
void set_attn_pingpong(int mask) { g_attn_pingpong = mask; }
int launch_attn_fwd(const AttnArgs& a_in, int precision, hipStream_t s) {
  int rc = check_attn(a_in, precision);
  if (rc != PFN_OK) return rc;
  AttnArgs a = a_in;
  a.pingpong = g_attn_pingpong;
  a.q_begin = a.q_begin / 256 * 256;
  PFN_ATTN_DISPATCH(launch_fwd_t, return (launch_fwd_t<float, 256>(a, s)))
}
// Key-range splits of a predict pass: when the query blocks x heads x datasets (x V slices) of one pass over the keys fill less than the chip's 256 CUs, the keys are
// split into ranges of whole tiles until the grid holds about 512 workgroups (one to two rounds); one split means no merge.
int attn_cache_splits(int B, int n, int E, int H, int sep, int precision) {
  if (B < 1 || n < 1 || H < 1 || E % H) return 1;
  const int D = E / H;
  const bool w16 = prec_is16(precision);
  const int qblk = (w16 && D <= 128) ? 256 : 128, kvb = (w16 && D <= 128) ? 64 : 32, slices = (!w16 && D == 256) ? 2 : 1;
  const long wgs = (long)((n + qblk - 1) / qblk) * H * B * slices;
  if (wgs >= 256) return 1;
  const long want = 512 / wgs;
  if (sep < 0) return (int)std::max<long>(1, want);
  const long ntiles = (sep + kvb - 1) / kvb;
  return (int)std::max<long>(1, std::min(want, ntiles));
}
int launch_attn_fwd_cache(const AttnArgs& a_in, int precision, hipStream_t s) {
  if (a_in.B <= 0 || a_in.S <= 0 || a_in.H <= 0 || a_in.E % a_in.H || a_in.sep < 0 || (a_in.sep > 0 && !a_in.kv)) return PFN_ERR_ARGUMENT;
  if ((a_in.E * prec_esize(precision)) % 16 || (a_in.kv_ld * prec_esize(precision)) % 16) return PFN_ERR_ALIGNMENT;
  AttnArgs a = a_in;
  a.pingpong = g_attn_pingpong;
  a.q_begin = 0; a.q_from_sep = 0; a.p_drop = 0.f; a.xq = nullptr;      // (sep_of: per-dataset key counts of a ragged context, or nullptr)
  PFN_ATTN_DISPATCH(launch_fwd_cache_t, return (launch_fwd_cache_t<float, 256>(a, s)))
}
template <typename T, int D> static int launch_bwd_cache_t(const AttnCacheBwdArgs& a_in, hipStream_t s) {
  using C = AttnCfg<T, D>;
  using G = BwdCacheCfg<T, D>;
  static_assert(G::LDS <= 160 * 1024, "cached attention backward: tile buffers exceed the CU's LDS");
  AttnCacheBwdArgs a = a_in;
  int nsplit = attn_cache_splits(a.B, a.S, a.E, a.H, a.sep, sizeof(T) == 4 ? PFN_PREC_F32 : PFN_PREC_BF16);      // the forward's rule
  if (g_attn_cache_split_cap > 0) nsplit = std::min(nsplit, g_attn_cache_split_cap);
  const int ntiles = (a.sep + G::KVB - 1) / G::KVB;
  a.split_keys = nsplit > 1 ? (ntiles + nsplit - 1) / nsplit * G::KVB : std::max(a.sep, 1);
  const int nz = nsplit > 1 ? (a.sep + a.split_keys - 1) / a.split_keys : 1;
  if (nz > 1 && !a.part_dq) return PFN_ERR_ARGUMENT;
  static LdsAllowance allowance;
  allowance.ensure(attn_bwd_cache_kernel<T, D>, G::LDS);
  const dim3 grid(((a.S + C::QBLK - 1) / C::QBLK) * a.H * a.B, D / G::DQ, nz);
  hipLaunchKernelGGL((attn_bwd_cache_kernel<T, D>), grid, dim3(C::NT), G::LDS, s, a);
  if (nz > 1) {
    const long work = (long)a.B * a.S * (a.E / 4);
    hipLaunchKernelGGL(attn_bwd_cache_merge_kernel<T>, dim3((unsigned)std::min<long>((work + 255) / 256, 4096)), dim3(256), 0, s, a, nz, 1.f / sqrtf((float)D));
  }
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}
int launch_attn_bwd_cache(const AttnCacheBwdArgs& a, int precision, hipStream_t s) {
  if (a.B <= 0 || a.S <= 0 || a.H <= 0 || a.E % a.H || a.sep < 0 || (a.sep > 0 && !a.kv) || !a.qkv || !a.ctx || !a.lse || !a.dctx || !a.dqkv) return PFN_ERR_ARGUMENT;
  if ((a.E * prec_esize(precision)) % 16 || (a.kv_ld * prec_esize(precision)) % 16) return PFN_ERR_ALIGNMENT;
  PFN_ATTN_DISPATCH(launch_bwd_cache_t, return (launch_bwd_cache_t<float, 256>(a, s)))
}
// dst[b] = min(max(src[b], 0), hi): the condition pass of a ragged context hands the embedding, key-shift and attention kernels of the training path (which trust
// their sep_of) a copy that cannot carry them outside [0, sep_max]
__global__ __launch_bounds__(256) void clamp_sep_of_kernel(const int* src, int* dst, int B, int hi) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) dst[b] = min(max(src[b], 0), hi);
}
int launch_clamp_sep_of(const int* src, int* dst, int B, int hi, hipStream_t s) {
  if (!src || !dst || B < 1 || hi < 0) return PFN_ERR_ARGUMENT;
  hipLaunchKernelGGL(clamp_sep_of_kernel, dim3((B + 255) / 256), dim3(256), 0, s, src, dst, B, hi);
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}
void attn_bwd_ds_dims(int S, int sep, int* rows, int* ld) {
  *rows = (sep + 63) / 64 * 64;       // whole key tiles of the dQ pass
  *ld = (S + 255) / 256 * 256;        // whole query blocks of the dQ pass (and 16-byte aligned rows)
}
int64_t attn_bwd_ds_bytes(int B, int S, int H, int precision) {
  int rows, ld;
  attn_bwd_ds_dims(S, S, &rows, &ld);
  return (int64_t)B * H * rows * ld * prec_esize(precision);
}
// No train rows at all (sep = 0, one eval position, no dropout): every query sees its own key alone, P = 1, and the backward is dV = dO, dQ = dK = 0 EXACTLY.
// The general kernels return dS = P (dP - delta) there, a difference of two f32 sums of the same products in different orders: ~2^-24 |dP| of noise in dQ and dK
// (tests/test_gpu_attn_probe.py, S130-sep0).  This pass stands in for the query-block pass, which at sep = 0 writes all of dqkv (the key-block pass has no keys
// and is not launched); delta and lse2 have no reader then, so attn_delta_kernel is not launched either, and AttnArgs::zero_delta is honoured as that pass
// honours it.  One sweep over dqkv, 16 bytes per thread step; row widths are multiples of 16 bytes (check_attn).
__global__ void attn_bwd_self_only_kernel(const uint4* __restrict__ dctx, uint4* __restrict__ dqkv, long rows, int chunks, float* __restrict__ delta, long ndelta) {
  const long total = rows * 3 * chunks;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / (3 * chunks);
    const int c = (int)(i - row * 3 * chunks);
    dqkv[i] = c >= 2 * chunks ? dctx[row * chunks + (c - 2 * chunks)] : make_uint4(0u, 0u, 0u, 0u);
  }
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < ndelta; i += (long)gridDim.x * blockDim.x) delta[i] = 0.f;      // (ndelta = 0 unless zero_delta)
}
static int launch_bwd_self_only(const AttnArgs& a, int precision, hipStream_t s) {
  const int parts = a.parts ? a.parts : ~0;
  if (!(parts & ATTN_BWD_DQ)) return PFN_OK;
  if (!a.dctx || !a.dqkv || (a.zero_delta && !a.delta)) return PFN_ERR_ARGUMENT;
  const long rows = (long)a.B * a.S;
  const int chunks = a.E * prec_esize(precision) / 16;
  const int grid = (int)std::min<long>((rows * 3 * chunks + 255) / 256, 4096);
  ProfScope ps(PFN_PROF_ATTN_BWD_DQ, s);
  hipLaunchKernelGGL(attn_bwd_self_only_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<const uint4*>(a.dctx), reinterpret_cast<uint4*>(a.dqkv), rows, chunks,
                     a.delta, a.zero_delta ? (long)a.B * a.H * a.S : 0L);
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}
int launch_attn_bwd(const AttnArgs& a_in, int precision, hipStream_t s) {
  int rc = check_attn(a_in, precision);
  if (rc != PFN_OK) return rc;
  if (!a_in.ds) return PFN_ERR_ARGUMENT;
  if (a_in.sep == 0 && !a_in.sep_of && a_in.q_begin == 0 && a_in.p_drop == 0.f) {
    const int D = a_in.E / a_in.H;
    if (D != 32 && D != 64 && D != 128 && D != 256) return PFN_ERR_UNSUPPORTED;      // (the head dims of PFN_ATTN_DISPATCH: no shape gains support here)
    return launch_bwd_self_only(a_in, precision, s);
  }
  AttnArgs a = a_in;
  attn_bwd_ds_dims(a.S, a.sep, &a.ds_rows, &a.ds_ld);
  a.q_begin = a.q_begin / 256 * 256;
  PFN_ATTN_DISPATCH(launch_bwd_t, return (launch_bwd_plain_f32<256>(a, s)))
}

}  // namespace pfn
