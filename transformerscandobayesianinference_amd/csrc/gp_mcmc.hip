// Batched NUTS (iterative multinomial No-U-Turn sampler with diagonal mass and Stan's warmup adaptation): every chain's state machine advances by exactly
// one gradient evaluation per launch.  The kernels know nothing about the target: the caller evaluates the potential and its gradient at `trial`
// (pfn_gp_mll_grad for the GP hyper-posterior, any other differentiable target alike) and hands `value`, `grad` back.
//
// Layout: one wave of 64 lanes per chain, a lane holds coordinates `lane` and `lane + 64` (D <= 128); four chains per 256-thread block.  Every vector of a
// chain's state lives in the workspace and every lane reads and writes only its own two coordinates of it, so no lane ever reads memory another lane wrote in
// the same launch; reductions are wave shuffles, every decision goes through readfirstlane, the only atomic is the counter of finished chains.  The tree's
// checkpoint momenta (one row per set bit of the leaf index: max_tree_depth rows) are workspace rows selected by a wave-uniform index -- no per-thread arrays.
#include "pfn_device.h"
#include "pfn_host.h"

namespace pfn {
namespace {

constexpr int NUTS_WAVES = 4;
constexpr unsigned NUTS_MAGIC = 0x4e555453u;
enum { VEC_TL, VEC_RL, VEC_GL, VEC_TR, VEC_RR, VEC_GR, VEC_PROP, VEC_PROPG, VEC_SPROP, VEC_SPROPG, VEC_RSUM, VEC_SRSUM, VEC_WMEAN, VEC_WM2, VEC_CK };
enum { PH_INIT = 0, PH_RUN = 1, PH_DONE = 2 };

struct NutsHeader {      // 256 bytes at the head of the workspace, written by nuts_init_kernel
  unsigned long long seed;
  unsigned magic;
  int C, D, depth, W, N, flags, n_windows, window_start;
  int window_ends[PFN_NUTS_MAX_WINDOWS];
  float target, step_size;
  int pad[64 - 13 - PFN_NUTS_MAX_WINDOWS];
};
static_assert(sizeof(NutsHeader) == PFN_NUTS_INV_MASS_OFFSET, "header size");

struct NutsState {     // a chain's scalars
  int phase, t, depth, n, leaves, diverging, window, da_count, wf_count, dir;
  float H0, logW, s_logW, accept_sum, propU, spropU, eps, mu, hbar, log_eps_bar;
  unsigned id_lo, id_hi;      // the chain's Philox stream
};
struct alignas(128) NutsScalars { NutsState st; };     // 128 bytes per chain; lane 0 writes them at the end of a launch, every lane reads them at the start of the next
static_assert(sizeof(NutsScalars) == 128, "scalars size");

struct NutsLayout {
  NutsHeader* hdr;
  float* inv_mass;       // [C, D]
  NutsScalars* scal;     // [C]
  float* vecs;           // [14 + 2 depth][C][D]
};
inline __host__ __device__ int64_t nuts_vec_count(int depth) { return VEC_CK + 2 * depth; }
inline __host__ __device__ int64_t nuts_inv_mass_bytes(int C, int D) { return (sizeof(float) * (int64_t)C * D + 127) / 128 * 128; }      // keeps the scalars behind it 128-byte aligned
inline __host__ __device__ NutsLayout nuts_layout(void* ws, int C, int D, int depth) {
  char* p = (char*)ws;
  NutsLayout l;
  l.hdr = (NutsHeader*)p; p += sizeof(NutsHeader);
  l.inv_mass = (float*)p; p += nuts_inv_mass_bytes(C, D);
  l.scal = (NutsScalars*)p; p += sizeof(NutsScalars) * (int64_t)C;
  l.vecs = (float*)p;
  return l;
}

struct F2 { float a, b; };
PFN_DEV float uni_f(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }
PFN_DEV int uni_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
PFN_DEV float logaddexp_f(float a, float b) {
  const float hi = fmaxf(a, b), lo = fminf(a, b);
  if (hi == -INFINITY) return -INFINITY;
  return hi + log1pf(expf(lo - hi));
}

struct Chain {      // the lane's view of one chain's vectors
  float* vecs; int C, D, c, k0, k1; bool v0, v1;
  PFN_DEV float* row(int v) const { return vecs + ((long)v * C + c) * D; }
  PFN_DEV F2 ld(const float* p) const { return F2{v0 ? p[k0] : 0.f, v1 ? p[k1] : 0.f}; }
  PFN_DEV void st(float* p, F2 x) const { if (v0) p[k0] = x.a; if (v1) p[k1] = x.b; }
  PFN_DEV F2 get(int v) const { return ld(row(v)); }
  PFN_DEV void put(int v, F2 x) const { st(row(v), x); }
};
PFN_DEV float dot3(F2 m, F2 a, F2 b) { return uni_f(wave_sum(m.a * a.a * b.a + m.b * a.b * b.b)); }
// U-turn between the momenta a and b of a span whose momenta sum to s (both ends counted once)
PFN_DEV bool turning(F2 m, F2 a, F2 b, F2 s) {
  const F2 sp = {s.a - 0.5f * (a.a + b.a), s.b - 0.5f * (a.b + b.b)};
  return dot3(m, a, sp) <= 0.f || dot3(m, b, sp) <= 0.f;
}

struct NutsInitArgs {
  void* ws; int C, D, depth; long ld; int W, N, flags, n_windows, window_start; int window_ends[PFN_NUTS_MAX_WINDOWS];
  float step_size, target; unsigned long long seed; const long long* chain_ids; const float* theta0; const float* inv_mass0; float* trial; int* done_count;
};

__global__ __launch_bounds__(256) void nuts_init_kernel(NutsInitArgs a) {
  const NutsLayout L = nuts_layout(a.ws, a.C, a.D, a.depth);
  const int lane = threadIdx.x & 63;
  const int c = uni_i(blockIdx.x * NUTS_WAVES + (threadIdx.x >> 6));
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    NutsHeader* h = L.hdr;
    h->magic = NUTS_MAGIC; h->C = a.C; h->D = a.D; h->depth = a.depth; h->W = a.W; h->N = a.N; h->flags = a.flags; h->n_windows = a.n_windows; h->window_start = a.window_start;
    for (int i = 0; i < PFN_NUTS_MAX_WINDOWS; ++i) h->window_ends[i] = a.window_ends[i];
    h->seed = a.seed; h->target = a.target; h->step_size = a.step_size;
    *a.done_count = 0;
  }
  if (c >= a.C) return;
  const Chain ch{L.vecs, a.C, a.D, c, lane, lane + 64, lane < a.D, lane + 64 < a.D};
  const F2 th = ch.ld(a.theta0 + (long)c * a.ld);
  const F2 m = a.inv_mass0 ? ch.ld(a.inv_mass0 + (long)c * a.D) : F2{1.f, 1.f};
  ch.st(L.inv_mass + (long)c * a.D, m);
  ch.put(VEC_PROP, th);
  ch.put(VEC_WMEAN, F2{0.f, 0.f});
  ch.put(VEC_WM2, F2{0.f, 0.f});
  ch.st(a.trial + (long)c * a.ld, th);
  if (lane == 0) {
    const unsigned long long id = a.chain_ids ? (unsigned long long)a.chain_ids[c] : (unsigned long long)c;
    NutsState s{};
    s.id_lo = (unsigned)id; s.id_hi = (unsigned)(id >> 32);
    s.phase = PH_INIT;
    s.eps = a.step_size;
    s.mu = logf(10.f * a.step_size);
    L.scal[c].st = s;
  }
}

struct NutsAdvanceArgs {
  void* ws; int C, D, depth, W, N; long ld;
  const float* value; const float* grad; const int* info; const float* scale; const float* shift;
  float* trial; float* samples; float* stats; float* warm; int* done_count;
};

__global__ __launch_bounds__(256) void nuts_advance_kernel(NutsAdvanceArgs a) {
  const NutsLayout L = nuts_layout(a.ws, a.C, a.D, a.depth);
  const int lane = threadIdx.x & 63;
  const int c = uni_i(blockIdx.x * NUTS_WAVES + (threadIdx.x >> 6));
  if (c >= a.C) return;
  const NutsHeader* h = L.hdr;
  if (uni_i(h->magic != NUTS_MAGIC || h->C != a.C || h->D != a.D || h->depth != a.depth || h->W != a.W || h->N != a.N)) return;      // not what pfn_nuts_init laid out: touch nothing
  NutsState* const sp = &L.scal[c].st;
  NutsState s = *sp;
  const int phase = uni_i(s.phase);
  if (phase == PH_DONE) return;
  const int W = a.W, N = a.N, flags = uni_i(h->flags);
  const unsigned long long seed = h->seed;
  const unsigned long long id = ((unsigned long long)(unsigned)uni_i((int)s.id_hi) << 32) | (unsigned)uni_i((int)s.id_lo);
  const Chain ch{L.vecs, a.C, a.D, c, lane, lane + 64, lane < a.D, lane + 64 < a.D};
  float* mrow = L.inv_mass + (long)c * a.D;
  F2 m = ch.ld(mrow);

  int t = uni_i(s.t), depth = uni_i(s.depth), n = uni_i(s.n), leaves = uni_i(s.leaves), diverging = uni_i(s.diverging), dir = uni_i(s.dir);
  float eps = uni_f(s.eps);
  const int edge0 = dir > 0 ? VEC_TR : VEC_TL;      // (theta, r, g) rows of the moving edge

  // ---- the potential and its gradient at the trial point
  const F2 th = ch.get(phase == PH_INIT ? VEC_PROP : edge0);
  const F2 sh = a.shift ? ch.ld(a.shift) : F2{0.f, 0.f};
  const float sc = a.scale ? a.scale[c] : 1.f;
  const F2 graw = ch.ld(a.grad + (long)c * a.ld);
  F2 g = {sc * graw.a - sh.a, sc * graw.b - sh.b};
  float U = uni_f(sc * a.value[c] - wave_sum(sh.a * th.a + sh.b * th.b));
  const bool bad = uni_i((a.info && a.info[c] != 0) || !isfinite(U));
  if (bad) { U = INFINITY; g = F2{0.f, 0.f}; }

  bool new_transition = false, start_subtree = false, step = false;
  if (phase == PH_INIT) {
    ch.put(VEC_PROPG, g);
    s.propU = U;
    new_transition = true;
  } else {
    // ---- second half of the leapfrog, then the leaf's bookkeeping
    const float hv = 0.5f * (float)dir * eps;
    const F2 rh = ch.get(edge0 + 1);
    const F2 r = {rh.a - hv * g.a, rh.b - hv * g.b};
    const float dE = U + 0.5f * dot3(m, r, r) - uni_f(s.H0);
    const bool fin = isfinite(dE);
    s.accept_sum = uni_f(s.accept_sum) + (fin ? fminf(1.f, expf(-dE)) : 0.f);
    leaves += 1;
    bool end = false;
    int depth_out = depth + 1;
    if (!fin || dE > 1000.f) {
      diverging = 1;
      end = true;
    } else {
      ch.put(edge0 + 1, r);
      ch.put(edge0 + 2, g);
      const float s_logW = uni_f(s.s_logW);
      const float nw = logaddexp_f(s_logW, -dE);
      const int l = leaves - 1;
      const U4 q = philox4x32_10(((unsigned long long)t << 12) | (unsigned)(64 + (l >> 2)), id, seed);
      const int comp = l & 3;
      const float ul = u01(comp == 0 ? q.x : comp == 1 ? q.y : comp == 2 ? q.z : q.w);
      if (ul < expf(-dE - nw)) {
        ch.put(VEC_SPROP, th);
        ch.put(VEC_SPROPG, g);
        s.spropU = U;
      }
      s.s_logW = nw;
      F2 srs = r;
      if (n > 0) { const F2 o = ch.get(VEC_SRSUM); srs = F2{o.a + r.a, o.b + r.b}; }
      ch.put(VEC_SRSUM, srs);
      const int pc = __builtin_popcount(n >> 1);
      if ((n & 1) == 0) {
        ch.put(VEC_CK + pc, r);
        ch.put(VEC_CK + a.depth + pc, srs);
      } else {
        const int imin = pc - __builtin_ctz(~n) + 1;
        for (int i = pc; i >= imin; --i) {
          const F2 rc = ch.get(VEC_CK + i), sck = ch.get(VEC_CK + a.depth + i);
          if (turning(m, rc, r, F2{srs.a - sck.a + rc.a, srs.b - sck.b + rc.b})) { end = true; break; }
        }
      }
      n += 1;
      if (!end && n == (1 << depth)) {      // the subtree is complete: biased progressive sampling at the top, then the U-turn across the whole tree
        const U4 qd = philox4x32_10(((unsigned long long)t << 12) | (unsigned)(32 + depth), id, seed);
        const float logW = uni_f(s.logW);
        if (u01(qd.y) < fminf(1.f, expf(nw - logW))) {
          ch.put(VEC_PROP, ch.get(VEC_SPROP));
          ch.put(VEC_PROPG, ch.get(VEC_SPROPG));
          s.propU = uni_f(s.spropU);
        }
        s.logW = logaddexp_f(logW, nw);
        const F2 o = ch.get(VEC_RSUM);
        const F2 rsum = {o.a + srs.a, o.b + srs.b};
        ch.put(VEC_RSUM, rsum);
        depth += 1;
        depth_out = depth;
        const F2 other = ch.get(dir > 0 ? VEC_RL : VEC_RR);
        if (turning(m, other, r, rsum) || depth >= a.depth) end = true;
        else start_subtree = true;
      } else if (!end) {
        step = true;
      }
    }
    if (end) {
      // ---- the transition is over: its record, the adaptation, and either the next transition or the end of the chain
      const float acc = uni_f(s.accept_sum) / (float)leaves;
      const F2 kept = ch.get(VEC_PROP);
      if (lane < 8) {
        const float v = lane == 0 ? eps : lane == 1 ? acc : lane == 2 ? (float)depth_out : lane == 3 ? (float)leaves : lane == 4 ? (float)diverging : lane == 5 ? uni_f(s.propU) : 0.f;
        a.stats[((long)c * (W + N) + t) * 8 + lane] = v;
      }
      if (t >= W) ch.st(a.samples + ((long)c * N + (t - W)) * a.D, kept);
      else if ((flags & PFN_NUTS_KEEP_WARMUP) && a.warm) ch.st(a.warm + ((long)c * W + t) * a.D, kept);
      if (t < W) {
        // dual averaging (Hoffman & Gelman 2014, algorithm 5; gamma .05, t0 10, kappa .75)
        int cnt = uni_i(s.da_count) + 1;
        float hbar = uni_f(s.hbar), leb = uni_f(s.log_eps_bar);
        const float w = 1.f / ((float)cnt + 10.f);
        hbar = (1.f - w) * hbar + w * (uni_f(h->target) - acc);
        const float le = uni_f(s.mu) - sqrtf((float)cnt) / 0.05f * hbar;
        const float eta = powf((float)cnt, -0.75f);
        leb = eta * le + (1.f - eta) * leb;
        eps = expf(le);
        int window = uni_i(s.window);
        const int nwin = uni_i(h->n_windows);
        if ((flags & PFN_NUTS_ADAPT_MASS) && window < nwin && t >= uni_i(h->window_start)) {
          // Welford mean / M2 of the kept points over Stan's slow windows
          const int wn = uni_i(s.wf_count) + 1;
          F2 mean = ch.get(VEC_WMEAN), m2 = ch.get(VEC_WM2);
          const F2 d = {kept.a - mean.a, kept.b - mean.b};
          mean = F2{mean.a + d.a / (float)wn, mean.b + d.b / (float)wn};
          m2 = F2{m2.a + d.a * (kept.a - mean.a), m2.b + d.b * (kept.b - mean.b)};
          s.wf_count = wn;
          if (t + 1 == uni_i(h->window_ends[window])) {
            if (wn > 1) {
              const float fn = (float)wn, k = fn / (fn + 5.f), reg = 1e-3f * (5.f / (fn + 5.f));
              m = F2{m2.a / (fn - 1.f) * k + reg, m2.b / (fn - 1.f) * k + reg};
              ch.st(mrow, m);
            }
            mean = F2{0.f, 0.f}; m2 = F2{0.f, 0.f};
            s.wf_count = 0;
            window += 1;
            s.mu = logf(10.f * eps);
            cnt = 0; hbar = 0.f; leb = 0.f;
          }
          ch.put(VEC_WMEAN, mean);
          ch.put(VEC_WM2, m2);
        }
        if (t + 1 == W) eps = expf(leb);      // after warmup: the averaged step size (no window ends at W: pfn_nuts_init refuses one, dual averaging needs transitions after its restart)
        s.window = window; s.da_count = cnt; s.hbar = hbar; s.log_eps_bar = leb;
      }
      t += 1;
      if (t >= W + N) {
        ch.st(a.trial + (long)c * a.ld, kept);      // a finished chain rests at its last sample and is never written again
        if (lane == 0) {
          s.phase = PH_DONE; s.t = t; s.eps = eps;
          *sp = s;
          atomicAdd(a.done_count, 1);
        }
        return;
      }
      new_transition = true;
    }
  }

  if (new_transition) {
    // ---- momentum z / sqrt(m), coordinate k from Philox block k >> 2 of this transition
    float z0[4], z1[4];
    normal4(philox4x32_10(((unsigned long long)t << 12) | (unsigned)(lane >> 2), id, seed), z0);
    normal4(philox4x32_10(((unsigned long long)t << 12) | (unsigned)(16 + (lane >> 2)), id, seed), z1);
    const int e = lane & 3;
    const float za = e == 0 ? z0[0] : e == 1 ? z0[1] : e == 2 ? z0[2] : z0[3];
    const float zb = e == 0 ? z1[0] : e == 1 ? z1[1] : e == 2 ? z1[2] : z1[3];
    const F2 r0 = {ch.v0 ? za / sqrtf(m.a) : 0.f, ch.v1 ? zb / sqrtf(m.b) : 0.f};
    const F2 p = ch.get(VEC_PROP), pg = ch.get(VEC_PROPG);
    s.H0 = uni_f(s.propU) + 0.5f * dot3(m, r0, r0);
    ch.put(VEC_TL, p); ch.put(VEC_TR, p);
    ch.put(VEC_RL, r0); ch.put(VEC_RR, r0);
    ch.put(VEC_GL, pg); ch.put(VEC_GR, pg);
    ch.put(VEC_RSUM, r0);
    s.logW = 0.f; s.accept_sum = 0.f;
    depth = 0; leaves = 0; diverging = 0;
    start_subtree = true;
  }
  if (start_subtree) {
    const U4 qd = philox4x32_10(((unsigned long long)t << 12) | (unsigned)(32 + depth), id, seed);
    dir = u01(qd.x) < 0.5f ? 1 : -1;
    n = 0;
    s.s_logW = -INFINITY;
    step = true;
  }
  if (step) {
    // ---- first half of the next leapfrog from the moving edge: r -= v eps g / 2, theta += v eps m r; the trial point goes out for evaluation
    const int edge = dir > 0 ? VEC_TR : VEC_TL;
    const F2 te = ch.get(edge), re = ch.get(edge + 1), ge = ch.get(edge + 2);
    const float ve = (float)dir * eps;
    const F2 rh = {re.a - 0.5f * ve * ge.a, re.b - 0.5f * ve * ge.b};
    const F2 tn = {te.a + ve * m.a * rh.a, te.b + ve * m.b * rh.b};
    ch.put(edge, tn);
    ch.put(edge + 1, rh);
    ch.st(a.trial + (long)c * a.ld, tn);
  }
  if (lane == 0) {
    s.phase = PH_RUN; s.t = t; s.depth = depth; s.n = n; s.leaves = leaves; s.diverging = diverging; s.dir = dir; s.eps = eps;
    *sp = s;
  }
}

int64_t nuts_workspace_bytes(int C, int D, int depth) {
  return (int64_t)sizeof(NutsHeader) + nuts_inv_mass_bytes(C, D) + sizeof(NutsScalars) * (int64_t)C + sizeof(float) * nuts_vec_count(depth) * C * D;
}

int launch_nuts_init(const NutsInitArgs& a, hipStream_t s) {
  nuts_init_kernel<<<dim3((a.C + NUTS_WAVES - 1) / NUTS_WAVES), dim3(64 * NUTS_WAVES), 0, s>>>(a);
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

int launch_nuts_advance(const NutsAdvanceArgs& a, hipStream_t s) {
  nuts_advance_kernel<<<dim3((a.C + NUTS_WAVES - 1) / NUTS_WAVES), dim3(64 * NUTS_WAVES), 0, s>>>(a);
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

int nuts_check(void* ws, int64_t ws_bytes, int C, int D, int64_t ld, int depth) {
  if (C < 1 || D < 1 || D > 128 || depth < 1 || depth > 10 || ld < D || !ws) return fail(PFN_ERR_ARGUMENT, "bad nuts arguments (C %d, D %d in 1..128, ld %lld >= D, max_tree_depth %d in 1..10)", C, D, (long long)ld, depth);
  if (ws_bytes < nuts_workspace_bytes(C, D, depth)) return fail(PFN_ERR_ARGUMENT, "ws_bytes %lld < pfn_nuts_workspace_bytes = %lld", (long long)ws_bytes, (long long)nuts_workspace_bytes(C, D, depth));
  return PFN_OK;
}

}  // namespace
}  // namespace pfn

using namespace pfn;

extern "C" {
int64_t pfn_nuts_workspace_bytes(int C, int D, int max_tree_depth) {
  if (C < 1 || D < 1 || D > 128 || max_tree_depth < 1 || max_tree_depth > 10) return -1;
  return nuts_workspace_bytes(C, D, max_tree_depth);
}
// window_ends: a HOST array [n_windows]; chain_ids [C] or null (the chain's index); inv_mass0 [C, D] or null (ones)
int pfn_nuts_init(void* ws, int64_t ws_bytes, int C, int D, int64_t ld, int max_tree_depth, int num_warmup, int num_samples, int flags, const int32_t* window_ends,
                  int n_windows, int window_start, float step_size, float target_accept, uint64_t seed, const int64_t* chain_ids, const float* theta0,
                  const float* inv_mass0, float* trial, int32_t* done_count, void* stream) {
  if (int rc = nuts_check(ws, ws_bytes, C, D, ld, max_tree_depth)) return rc;
  if (!theta0 || !trial || !done_count || num_warmup < 0 || num_samples < 1 || !(step_size > 0.f) || !(target_accept > 0.f && target_accept < 1.f))
    return fail(PFN_ERR_ARGUMENT, "bad nuts_init arguments");
  if (flags & ~(PFN_NUTS_ADAPT_MASS | PFN_NUTS_KEEP_WARMUP)) return fail(PFN_ERR_ARGUMENT, "unknown nuts flags 0x%x", flags);
  if (n_windows < 0 || n_windows > PFN_NUTS_MAX_WINDOWS || (n_windows > 0 && !window_ends) || window_start < 0) return fail(PFN_ERR_ARGUMENT, "bad adaptation windows");
  for (int i = 0; i < n_windows; ++i)
    if (window_ends[i] <= (i ? window_ends[i - 1] : window_start) || window_ends[i] >= num_warmup)
      return fail(PFN_ERR_ARGUMENT, "adaptation window ends must increase and lie below num_warmup (dual averaging restarts at a window end and needs transitions after it)");
  NutsInitArgs a{};
  a.ws = ws; a.C = C; a.D = D; a.depth = max_tree_depth; a.ld = ld; a.W = num_warmup; a.N = num_samples; a.flags = flags; a.n_windows = n_windows;
  a.window_start = window_start;
  for (int k = 0; k < n_windows; ++k) a.window_ends[k] = window_ends[k];
  a.step_size = step_size; a.target = target_accept; a.seed = seed; a.chain_ids = (const long long*)chain_ids; a.theta0 = theta0; a.inv_mass0 = inv_mass0;
  a.trial = trial; a.done_count = done_count;
  PFN_TRY(launch_nuts_init(a, (hipStream_t)stream));
  return PFN_OK;
}
int pfn_nuts_advance(void* ws, int64_t ws_bytes, int C, int D, int64_t ld, int max_tree_depth, int num_warmup, int num_samples, const float* value, const float* grad,
                     const int32_t* info, const float* scale, const float* shift, float* trial, float* samples, float* stats, float* warm, int32_t* done_count, void* stream) {
  if (int rc = nuts_check(ws, ws_bytes, C, D, ld, max_tree_depth)) return rc;
  if (!value || !grad || !trial || !samples || !stats || !done_count || num_warmup < 0 || num_samples < 1) return fail(PFN_ERR_ARGUMENT, "bad nuts_advance arguments");
  NutsAdvanceArgs a{};
  a.ws = ws; a.C = C; a.D = D; a.depth = max_tree_depth; a.W = num_warmup; a.N = num_samples; a.ld = ld; a.value = value; a.grad = grad; a.info = info; a.scale = scale; a.shift = shift;
  a.trial = trial; a.samples = samples; a.stats = stats; a.warm = warm; a.done_count = done_count;
  PFN_TRY(launch_nuts_advance(a, (hipStream_t)stream));
  return PFN_OK;
}
}  // extern "C"
