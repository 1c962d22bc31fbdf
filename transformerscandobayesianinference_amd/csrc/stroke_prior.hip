// The stroke prior of the few-shot study (reference priors/stroke.py:9-63): every class of a dataset is one to a few straight strokes, every image of a class
// is those strokes shifted and jittered, drawn with a random width, filled with noise bytes and blurred.  The reference draws each size x size glyph with
// Pillow on the host -- 26,000 images per step at the notebook's shape; here one launch draws a batch, bit for bit what Pillow draws.
//
// One wave per image, four waves per block.  Lane y rasterises row y of every stroke into a 64-bit mask (hence size <= 64); after that the wave works on
// "items" of four horizontally adjacent pixels packed into one dword, item i = y * W + xq with W = ceil(size / 4), at dword i of a 4 KB LDS image: a blur
// pass reads the dwords i - 1, i + 1 (rows) or i - W, i + W (columns) of one buffer and writes dword i of the other, so consecutive lanes touch consecutive
// banks.  The output is 4 size^2 bytes per image; at size % 4 == 0 with 16-byte aligned images an item is one 16-byte store.
//
// ---- What Pillow does, restated (tests/stroke_ref.py is the same in numpy; tools/make_stroke_golden.py checks that against Pillow itself) ----
// RU(f) = floor(f + 1/2) for f >= 0, else -floor(|f| + 1/2);  RD(f) = ceil(f - 1/2) for f >= 0, else -ceil(|f| - 1/2).
// Width <= 1: Bresenham from p0, then p1; points off the canvas are skipped one by one.  Width > 1 with p0 == p1: that pixel.  Otherwise, in f64,
// h = hypot(dx, dy), s = (w - 1) / 2, rmax = RU(s) / h, rmin = RD(s) / h, dxmin = RD(rmin dy), dxmax = RD(rmax dy), dymin = RU(rmin dx), dymax = RU(rmax dx) and
// the polygon (x0 - dxmin, y0 + dymax), (x1 - dxmin, y1 + dymax), (x1 + dxmax, y1 - dymin), (x0 + dxmax, y0 - dymin) is filled: a horizontal edge is the closed
// span of its row; on row y every other edge with ymin <= y <= ymax gives x = f32(f32(f32(y - y0) m) + f32(x0)), m = f32(x1 - x0) / f32(y1 - y0), entered twice
// when y is that edge's ymax and below the polygon's; the values are sorted and each pair (a, b) at positions (0,1), (2,3), ... lights RU(a) .. RD(b) (in f32).
// THE TRAP: hipcc contracts a multiply and an add into one FMA by default, and the FMA's x differs from Pillow's on about 1 stroke in 400 -- a pixel at a span's
// end appears or vanishes.  edge_x() below rounds the product and the sum separately (and says why the _rn intrinsics do not).
//
// GaussianBlur(0.2) is three box passes along rows, then three along columns.  Pillow's box radius per pass is l + a with
//   sigma^2 = 0.2^2 / 3,  L = sqrt(12 sigma^2 + 1) = 1.077,  l = floor((L - 1) / 2) = 0,
//   a = (2l + 1) (l (l + 1) - 3 sigma^2) / (6 (sigma^2 - (l + 1)^2)) = -0.04 / -5.92 = 0.00675676 (in f32),
// and on bytes a pass is out = (c ww + (l + r) fw + 2^23) >> 24 with ww = floor(2^24 / (2a + 1)) = 16553519 and fw = (2^24 - ww) / 2 = 111848, the missing
// neighbour at a border replaced by the border pixel.  The largest sum is 255 (ww + 2 fw) + 2^23 = 4,286,578,433: it fits uint32_t and not int.
#include "pfn_device.h"
#include "pfn_host.h"

namespace pfn {

struct StrokeRenderArgs {
  const int32_t* segs;       // [N,8,4] = (x0, y0, x1, y1)
  const int32_t* n_strokes;  // [N]
  const int32_t* width;      // [N]
  const uint8_t* noise;      // [N,size^2] or null (Philox)
  long N;
  int size, normalize, vec16;      // vec16: size % 4 == 0 and every image of x 16-byte aligned
  long image_stride;         // floats between two images of x
  unsigned long long seed, offset;
  float* x;
  uint8_t* raw;              // [N,size^2] or null: before the blur
  uint8_t* img;              // [N,size^2] or null: after the blur
};
struct StrokePriorArgs {
  const int32_t* labels;     // [B,T]
  int B, T, C, size, normalize, vec16;
  int strokes_lo, strokes_hi, len_lo, len_hi, start_lo, start_hi, width_lo, width_hi, max_off, max_toff;
  unsigned long long seed, offset, first_dataset;
  float* x;                  // [T,B,size^2]
  int32_t* cls_n;            // [B,C]
  int32_t* cls_len;          // [B,C,8]
  int32_t* cls_start;        // [B,C,8,2]
  double* cls_dir;           // [B,C,8]
  int32_t* segs;             // [B,T,8,4]
  int32_t* width;            // [B,T]
  uint8_t* raw;              // [B,T,size^2] or null
  uint8_t* img;              // [B,T,size^2] or null
  int32_t* status;           // [B]
};

#define STROKE_HD __host__ __device__ inline

constexpr unsigned STROKE_WW = 16553519u, STROKE_FW = 111848u;
constexpr int STROKE_WAVES = 4;                  // images per block
constexpr int STROKE_ITEMS = 64 * 16;            // dwords of one LDS image: 64 rows of 16 packed dwords
enum { STROKE_STREAM_CLASS_N = 0, STROKE_STREAM_CLASS_PASS = 1, STROKE_STREAM_IMAGE = 2, STROKE_STREAM_JITTER = 3, STROKE_STREAM_NOISE = 4 };   // stream word = offset * 8 + purpose

// ---- the rasteriser: row y of one stroke as a bit mask (bit x = pixel x).  Host-callable so that it can be checked without a device. ----
STROKE_HD int ru64(double f) { return f >= 0. ? (int)floor(f + 0.5) : -(int)floor(fabs(f) + 0.5); }
STROKE_HD int rd64(double f) { return f >= 0. ? (int)ceil(f - 0.5) : -(int)ceil(fabs(f) - 0.5); }
STROKE_HD int ru32(float f) { return f >= 0.f ? (int)floorf(f + 0.5f) : -(int)floorf(fabsf(f) + 0.5f); }
STROKE_HD int rd32(float f) { return f >= 0.f ? (int)ceilf(f - 0.5f) : -(int)ceilf(fabsf(f) - 0.5f); }

// The product rounds, then the sum rounds: never one FMA.  __fmul_rn / __fadd_rn do NOT give that under hipcc: they are inline functions of a header compiled
// with contraction allowed, so once inlined their multiply and add fuse like any others (seen in the ISA: v_fmac_f32).  What holds is the pragma on the
// statements themselves (hipcc's default -ffp-contract=fast-honor-pragmas), and on the device an empty asm that the product has to pass through.
STROKE_HD float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  float p = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(p));
#endif
  return p;
}
STROKE_HD double mul_rn(double a, double b) {
#pragma clang fp contract(off)
  double p = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(p));
#endif
  return p;
}
STROKE_HD float edge_x(int y, int x0, int y0, float m) {
#pragma clang fp contract(off)
  const float p = mul_rn((float)(y - y0), m);
  return p + (float)x0;
}

STROKE_HD uint64_t span_bits(int xa, int xb, int size) {
  if (xa >= size || xb < 0) return 0;
  xa = xa < 0 ? 0 : xa;
  xb = xb > size - 1 ? size - 1 : xb;
  if (xa > xb) return 0;
  const int n = xb - xa + 1;
  return (n >= 64 ? ~0ull : ((1ull << n) - 1ull)) << xa;      // (1ull << 64 is undefined: a full row at size 64)
}
STROKE_HD uint64_t point_bit(int x, int py, int y, int size) { return (py == y && x >= 0 && x < size) ? 1ull << x : 0ull; }

STROKE_HD void cswap(float& a, float& b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo; b = hi;
}

STROKE_HD uint64_t stroke_row_mask(int x0, int y0, int x1, int y1, int width, int y, int size) {
  const int L = PFN_STROKE_COORD_LIMIT;
  if (x0 < -L || x0 > L || y0 < -L || y0 > L || x1 < -L || x1 > L || y1 < -L || y1 > L) return 0;
  uint64_t mask = 0;
  if (width <= 1) {
    int dx = x1 - x0, dy = y1 - y0;
    const int xs = dx < 0 ? -1 : 1, ys = dy < 0 ? -1 : 1;
    dx = dx < 0 ? -dx : dx; dy = dy < 0 ? -dy : dy;
    int x = x0, py = y0;
    if (dx == 0) {
      for (int i = 0; i < dy; ++i) { mask |= point_bit(x, py, y, size); py += ys; }
    } else if (dy == 0) {
      for (int i = 0; i < dx; ++i) { mask |= point_bit(x, py, y, size); x += xs; }
    } else if (dx > dy) {
      int e = 2 * dy - dx;
      for (int i = 0; i < dx; ++i) {
        mask |= point_bit(x, py, y, size);
        if (e >= 0) { py += ys; e -= 2 * dx; }
        e += 2 * dy; x += xs;
      }
    } else {
      int e = 2 * dx - dy;
      for (int i = 0; i < dy; ++i) {
        mask |= point_bit(x, py, y, size);
        if (e >= 0) { x += xs; e -= 2 * dy; }
        e += 2 * dx; py += ys;
      }
    }
    return mask | point_bit(x1, y1, y, size);
  }
  if (x0 == x1 && y0 == y1) return point_bit(x0, y0, y, size);
  const int dx = x1 - x0, dy = y1 - y0;
  const double h = sqrt((double)(dx * dx + dy * dy));      // hypot of two integers below 2^14: the sum of squares is exact
  const double s = (width - 1) / 2.0;
  const double rmax = ru64(s) / h, rmin = rd64(s) / h;
  const int dxmin = rd64(mul_rn(rmin, (double)dy)), dxmax = rd64(mul_rn(rmax, (double)dy)), dymin = ru64(mul_rn(rmin, (double)dx)), dymax = ru64(mul_rn(rmax, (double)dx));
  const int vx[4] = {x0 - dxmin, x1 - dxmin, x1 + dxmax, x0 + dxmax};
  const int vy[4] = {y0 + dymax, y1 + dymax, y1 - dymin, y0 - dymin};
  int pymax = vy[0];
#pragma unroll
  for (int e = 1; e < 4; ++e) pymax = vy[e] > pymax ? vy[e] : pymax;
  const float INF = __builtin_huge_valf();
  float xs[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int ex0 = vx[e], ey0 = vy[e], ex1 = vx[(e + 1) & 3], ey1 = vy[(e + 1) & 3];
    xs[2 * e] = INF; xs[2 * e + 1] = INF;
    if (ey0 == ey1) {
      if (y == ey0) mask |= span_bits(ex0 < ex1 ? ex0 : ex1, ex0 < ex1 ? ex1 : ex0, size);
    } else {
      const int emin = ey0 < ey1 ? ey0 : ey1, emax = ey0 < ey1 ? ey1 : ey0;
      if (y >= emin && y <= emax) {
        const float m = (float)(ex1 - ex0) / (float)(ey1 - ey0);
        const float x = edge_x(y, ex0, ey0, m);
        xs[2 * e] = x;
        if (y == emax && y < pymax) xs[2 * e + 1] = x;
      }
    }
  }
  // ascending, the empty slots (+inf) last: Batcher's 19-comparator network on 8 values
  cswap(xs[0], xs[1]); cswap(xs[2], xs[3]); cswap(xs[4], xs[5]); cswap(xs[6], xs[7]);
  cswap(xs[0], xs[2]); cswap(xs[1], xs[3]); cswap(xs[4], xs[6]); cswap(xs[5], xs[7]);
  cswap(xs[1], xs[2]); cswap(xs[5], xs[6]);
  cswap(xs[0], xs[4]); cswap(xs[1], xs[5]); cswap(xs[2], xs[6]); cswap(xs[3], xs[7]);
  cswap(xs[2], xs[4]); cswap(xs[3], xs[5]);
  cswap(xs[1], xs[2]); cswap(xs[3], xs[4]); cswap(xs[5], xs[6]);
#pragma unroll
  for (int p = 0; p < 4; ++p)
    if (xs[2 * p + 1] < INF) mask |= span_bits(ru32(xs[2 * p]), rd32(xs[2 * p + 1]), size);
  return mask;
}

// ---- one blur pass on four packed pixels -------------------------------------------------------------------------------------------------------------------
STROKE_HD unsigned blur_byte(unsigned c, unsigned l, unsigned r) { return (c * STROKE_WW + (l + r) * STROKE_FW + (1u << 23)) >> 24; }
STROKE_HD unsigned byte_of(unsigned w, int k) { return (w >> (8 * k)) & 255u; }

// along the row: prev / next are the neighbouring dwords (unused where has_prev / has_next is false), `last` the index (0..3) of pixel size - 1 when it lies in
// this dword, else 4
STROKE_HD unsigned blur_row_item(unsigned prev, unsigned cur, unsigned next, bool has_prev, int last) {
  unsigned out = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned c = byte_of(cur, k);
    const unsigned l = k > 0 ? byte_of(cur, k - 1) : (has_prev ? byte_of(prev, 3) : c);
    const unsigned r = k == last ? c : (k < 3 ? byte_of(cur, k + 1) : byte_of(next, 0));
    out |= blur_byte(c, l, r) << (8 * k);
  }
  return out;
}
STROKE_HD unsigned blur_col_item(unsigned up, unsigned cur, unsigned down) {
  unsigned out = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) out |= blur_byte(byte_of(cur, k), byte_of(up, k), byte_of(down, k)) << (8 * k);
  return out;
}

PFN_DEV unsigned draw_int(unsigned u, int lo, int hi) { return (unsigned)lo + __umulhi(u, (unsigned)(hi - lo + 1)); }      // bias < (hi - lo + 1) 2^-32
PFN_DEV double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct StrokeJob {
  int4 seg;                  // lane s < 8: stroke s
  int n_strokes, width;      // wave-uniform
  const uint8_t* noise;      // this image's noise bytes, or null: Philox at counter (noise_image * 64 + y) * 16 + xq
  unsigned long long noise_image, stream, seed;
  float* x;                  // this image's output, or null (an idle wave)
  uint8_t* raw;              // nullable
  uint8_t* img;              // nullable
};

// Draws one image.  Called by every wave of the block (it synchronises the block); buf: this wave's two LDS images; tab: byte / 255.
__device__ __forceinline__ void stroke_draw_image(const StrokeJob& j, unsigned* buf, const float* tab, int size, int normalize, bool vec16) {
  const int lane = lane_id();
  const int W = (size + 3) >> 2, nitems = size * W, rounds = (nitems + 63) >> 6;
  unsigned* b0 = buf;
  unsigned* b1 = buf + STROKE_ITEMS;
  uint64_t mask = 0;
  for (int s = 0; s < j.n_strokes; ++s) {
    const int x0 = __shfl(j.seg.x, s), y0 = __shfl(j.seg.y, s), x1 = __shfl(j.seg.z, s), y1 = __shfl(j.seg.w, s);
    if (lane < size) mask |= stroke_row_mask(x0, y0, x1, y1, j.width, lane, size);
  }
  // the noise byte under every lit pixel
  for (int r = 0; r < rounds; ++r) {
    const int i = r * 64 + lane;
    const bool valid = i < nitems;
    const int y = valid ? i / W : 0, xq = valid ? i - y * W : 0;
    const uint64_t m = __shfl((unsigned long long)mask, y);
    const unsigned nib = valid ? (unsigned)(m >> (4 * xq)) & 15u : 0u;
    unsigned word = 0;
    if (nib) {
      unsigned nz[4];
      if (j.noise) {
#pragma unroll
        for (int k = 0; k < 4; ++k) nz[k] = 4 * xq + k < size ? j.noise[y * size + 4 * xq + k] : 0u;
      } else {
        const U4 u = philox4x32_10((j.noise_image * 64ull + (unsigned)y) * 16ull + (unsigned)xq, j.stream, j.seed);
        nz[0] = 200u + __umulhi(u.x, 55u); nz[1] = 200u + __umulhi(u.y, 55u); nz[2] = 200u + __umulhi(u.z, 55u); nz[3] = 200u + __umulhi(u.w, 55u);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((nib >> k) & 1u) word |= nz[k] << (8 * k);
    }
    if (valid) {
      b0[i] = word;
      if (j.raw) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (4 * xq + k < size) j.raw[y * size + 4 * xq + k] = (uint8_t)byte_of(word, k);
      }
    }
  }
  // three passes along the rows: b0 -> b1 -> b0 -> b1
  for (int pass = 0; pass < 3; ++pass) {
    __syncthreads();
    for (int r = 0; r < rounds; ++r) {
      const int i = r * 64 + lane;
      if (i < nitems) {
        const int y = i / W, xq = i - y * W;
        const bool has_prev = xq > 0, has_next = xq < W - 1;
        const int last = has_next ? 4 : size - 1 - 4 * xq;
        b1[i] = blur_row_item(has_prev ? b0[i - 1] : 0u, b0[i], has_next ? b0[i + 1] : 0u, has_prev, last);
      }
    }
    unsigned* t = b0; b0 = b1; b1 = t;
  }
  // three along the columns
  for (int pass = 0; pass < 3; ++pass) {
    __syncthreads();
    for (int r = 0; r < rounds; ++r) {
      const int i = r * 64 + lane;
      if (i < nitems) {
        const unsigned cur = b0[i];
        b1[i] = blur_col_item(i >= W ? b0[i - W] : cur, cur, i + W < nitems ? b0[i + W] : cur);
      }
    }
    unsigned* t = b0; b0 = b1; b1 = t;
  }
  __syncthreads();
  // b0 holds the blurred image
  double mean = 0., inv = 1.;
  if (normalize) {      // (x - mean) / (std + 1e-6), std the unbiased one: two passes in f64 over the f32 values
    double s1 = 0.;
    for (int r = 0; r < rounds; ++r) {
      const int i = r * 64 + lane;
      if (i < nitems) {
        const unsigned w = b0[i];
        const int xq = i % W;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (4 * xq + k < size) s1 += (double)tab[byte_of(w, k)];
      }
    }
    mean = wave_sum(s1) / (double)(size * size);
    double s2 = 0.;
    for (int r = 0; r < rounds; ++r) {
      const int i = r * 64 + lane;
      if (i < nitems) {
        const unsigned w = b0[i];
        const int xq = i % W;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (4 * xq + k < size) { const double d = (double)tab[byte_of(w, k)] - mean; s2 += d * d; }
      }
    }
    inv = 1. / (sqrt(wave_sum(s2) / (double)(size * size - 1)) + 1e-6);
  }
  if (!j.x) return;
  for (int r = 0; r < rounds; ++r) {
    const int i = r * 64 + lane;
    if (i < nitems) {
      const unsigned w = b0[i];
      const int y = i / W, xq = i - y * W;
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float f = tab[byte_of(w, k)];
        v[k] = normalize ? (float)(((double)f - mean) * inv) : f;
      }
      if (vec16) {      // size % 4 == 0 and a 16-byte aligned image: pixel y * size + 4 xq is float 4 i
        *reinterpret_cast<f32x4*>(j.x + 4 * i) = f32x4{v[0], v[1], v[2], v[3]};
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (4 * xq + k < size) j.x[y * size + 4 * xq + k] = v[k];
      }
      if (j.img) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (4 * xq + k < size) j.img[y * size + 4 * xq + k] = (uint8_t)byte_of(w, k);
      }
    }
  }
}

__global__ __launch_bounds__(256) void stroke_render_kernel(StrokeRenderArgs a) {
  __shared__ unsigned buf[STROKE_WAVES][2 * STROKE_ITEMS];
  __shared__ float tab[256];
  tab[threadIdx.x] = (float)threadIdx.x / 255.f;      // correctly rounded (byte * (1 / 255.f) is not, for every byte)
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const long n = (long)blockIdx.x * STROKE_WAVES + wave;
  const bool active = n < a.N;
  const long px = (long)a.size * a.size;
  StrokeJob j{};
  if (active) {
    if (lane < PFN_STROKE_MAX_STROKES) j.seg = reinterpret_cast<const int4*>(a.segs)[n * PFN_STROKE_MAX_STROKES + lane];
    const int ns = a.n_strokes[n], w = a.width[n];
    j.n_strokes = ns < 0 ? 0 : (ns > PFN_STROKE_MAX_STROKES ? PFN_STROKE_MAX_STROKES : ns);
    j.width = w < 0 ? 0 : (w > PFN_STROKE_MAX_WIDTH ? PFN_STROKE_MAX_WIDTH : w);
    j.noise = a.noise ? a.noise + n * px : nullptr;
    j.noise_image = (unsigned long long)n; j.stream = a.offset * 8ull + STROKE_STREAM_NOISE; j.seed = a.seed;
    j.x = a.x + n * a.image_stride;
    j.raw = a.raw ? a.raw + n * px : nullptr;
    j.img = a.img ? a.img + n * px : nullptr;
  }
  stroke_draw_image(j, buf[wave], tab, a.size, a.normalize, a.vec16 != 0);
}

// One block per dataset, thread c < C draws class c: the stroke count, then per stroke the reference's retry loop.  One Philox block per pass: (length, start x,
// start y, angle); the first three are used on every third pass only, as the reference redraws them.
__global__ __launch_bounds__(64) void stroke_classes_kernel(StrokePriorArgs a) {
  const int b = blockIdx.x, c = threadIdx.x;
  const unsigned long long d = a.first_dataset + (unsigned long long)b;
  int capped = 0;
  if (c < a.C) {
    const long bc = (long)b * a.C + c;
    const int n = (int)draw_int(philox4x32_10(d * (unsigned)a.C + (unsigned)c, a.offset * 8ull + STROKE_STREAM_CLASS_N, a.seed).x, a.strokes_lo, a.strokes_hi);
    a.cls_n[bc] = n;
    for (int s = 0; s < PFN_STROKE_MAX_STROKES; ++s) {
      int len = 0, sx = 0, sy = 0;
      double theta = 0.;
      if (s < n) {
        const unsigned long long base = ((d * PFN_STROKE_MAX_CLASSES + (unsigned)c) * PFN_STROKE_MAX_STROKES + (unsigned)s) * PFN_STROKE_MAX_PASSES;
        bool ok = false;
        for (int p = 0; p < PFN_STROKE_MAX_PASSES && !ok; ++p) {
          const U4 u = philox4x32_10(base + (unsigned)p, a.offset * 8ull + STROKE_STREAM_CLASS_PASS, a.seed);
          if (p % 3 == 0) {
            len = (int)draw_int(u.x, a.len_lo, a.len_hi);
            sx = (int)draw_int(u.y, a.start_lo, a.start_hi);
            sy = (int)draw_int(u.z, a.start_lo, a.start_hi);
          }
          theta = (double)u.w * (6.283185307179586 / 4294967296.0);      // [0, 2 pi)
          double sn, cs;
          sincos(theta, &sn, &cs);
          const double ex = (double)sx + mul_rn(cs, (double)len), ey = (double)sy + mul_rn(sn, (double)len);
          ok = ex >= 0. && ex <= (double)(a.size - 1) && ey >= 0. && ey <= (double)(a.size - 1);
        }
        capped += ok ? 0 : 1;
      }
      a.cls_len[bc * PFN_STROKE_MAX_STROKES + s] = len;
      a.cls_start[(bc * PFN_STROKE_MAX_STROKES + s) * 2] = sx;
      a.cls_start[(bc * PFN_STROKE_MAX_STROKES + s) * 2 + 1] = sy;
      a.cls_dir[bc * PFN_STROKE_MAX_STROKES + s] = theta;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) capped += __shfl_xor(capped, o);
  if (c == 0) a.status[b] = capped;
}

// One wave per image (b, t): its class's strokes shifted by the image's offset, every end point jittered, then drawn.
__global__ __launch_bounds__(256) void stroke_images_kernel(StrokePriorArgs a) {
  __shared__ unsigned buf[STROKE_WAVES][2 * STROKE_ITEMS];
  __shared__ float tab[256];
  tab[threadIdx.x] = (float)threadIdx.x / 255.f;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const long g = (long)blockIdx.x * STROKE_WAVES + wave;      // b * T + t
  const bool active = g < (long)a.B * a.T;
  const long px = (long)a.size * a.size;
  StrokeJob j{};
  if (active) {
    const int b = (int)(g / a.T), t = (int)(g - (long)b * a.T);
    int c = a.labels[g];
    c = c < 0 ? 0 : (c >= a.C ? a.C - 1 : c);
    const long bc = (long)b * a.C + c;
    const unsigned long long image = (a.first_dataset + (unsigned long long)b) * (unsigned)a.T + (unsigned)t;
    const U4 u = philox4x32_10(image, a.offset * 8ull + STROKE_STREAM_IMAGE, a.seed);
    const int ns = a.cls_n[bc];
    j.n_strokes = ns < 0 ? 0 : (ns > PFN_STROKE_MAX_STROKES ? PFN_STROKE_MAX_STROKES : ns);
    j.width = (int)draw_int(u.x, a.width_lo, a.width_hi);
    const int ox = (int)draw_int(u.y, -a.max_off, a.max_off), oy = (int)draw_int(u.z, -a.max_off, a.max_off);
    if (lane < PFN_STROKE_MAX_STROKES) {
      int4 seg = {0, 0, 0, 0};
      if (lane < j.n_strokes) {
        const long cs = bc * PFN_STROKE_MAX_STROKES + lane;
        const U4 ju = philox4x32_10(image * 4ull + (unsigned)(lane >> 1), a.offset * 8ull + STROKE_STREAM_JITTER, a.seed);
        const int jx = (int)draw_int((lane & 1) ? ju.z : ju.x, -a.max_toff, a.max_toff), jy = (int)draw_int((lane & 1) ? ju.w : ju.y, -a.max_toff, a.max_toff);
        const double len = (double)a.cls_len[cs];
        double sn, co;
        sincos(a.cls_dir[cs], &sn, &co);
        seg.x = a.cls_start[cs * 2] + ox;
        seg.y = a.cls_start[cs * 2 + 1] + oy;
        // the reference's order: p0 + (len cos + jitter), every step rounded; rint = Python's round (half to even)
        seg.z = (int)rint((double)seg.x + (mul_rn(co, len) + (double)jx));
        seg.w = (int)rint((double)seg.y + (mul_rn(sn, len) + (double)jy));
      }
      j.seg = seg;
      reinterpret_cast<int4*>(a.segs)[g * PFN_STROKE_MAX_STROKES + lane] = seg;
    }
    if (lane == 0) a.width[g] = j.width;
    j.noise = nullptr;
    j.noise_image = image; j.stream = a.offset * 8ull + STROKE_STREAM_NOISE; j.seed = a.seed;
    j.x = a.x + ((long)t * a.B + b) * px;
    j.raw = a.raw ? a.raw + g * px : nullptr;
    j.img = a.img ? a.img + g * px : nullptr;
  }
  stroke_draw_image(j, buf[wave], tab, a.size, a.normalize, a.vec16 != 0);
}

static int launch_stroke_render(const StrokeRenderArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(stroke_render_kernel, dim3((unsigned)((a.N + STROKE_WAVES - 1) / STROKE_WAVES)), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

static int launch_stroke_prior(const StrokePriorArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(stroke_classes_kernel, dim3(a.B), dim3(64), 0, s, a);
  if (hipGetLastError() != hipSuccess) return PFN_ERR_LAUNCH;
  hipLaunchKernelGGL(stroke_images_kernel, dim3((unsigned)(((long)a.B * a.T + STROKE_WAVES - 1) / STROKE_WAVES)), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

static int stroke_size(const char* what, int size) {
  if (size < 8 || size > 64) return fail(PFN_ERR_UNSUPPORTED, "%s: size %d outside 8 .. 64 (one lane per row, a row's mask in 64 bits)", what, size);
  return PFN_OK;
}

}  // namespace pfn

using namespace pfn;

extern "C" {
int pfn_stroke_render(const int32_t* segs, const int32_t* n_strokes, const int32_t* width, const uint8_t* noise, int64_t N, int size, int normalize,
                      int64_t image_stride, uint64_t seed, uint64_t offset, float* x, uint8_t* raw, uint8_t* img, void* stream) {
  if (const int rc = stroke_size("stroke_render", size)) return rc;
  if (N < 0 || N > (int64_t)1 << 32 || image_stride < (int64_t)size * size)
    return fail(PFN_ERR_ARGUMENT, "bad stroke_render arguments (0 <= N %lld <= 2^32, image_stride %lld >= size^2)", (long long)N, (long long)image_stride);
  if (!segs || !n_strokes || !width || !x || (uintptr_t)segs % 16 || (uintptr_t)n_strokes % 4 || (uintptr_t)width % 4 || (uintptr_t)x % 4)
    return fail(PFN_ERR_ARGUMENT, "bad stroke_render arguments (segs, n_strokes, width, x not NULL; segs 16-byte, the others 4-byte aligned)");
  if (N == 0) return PFN_OK;
  StrokeRenderArgs a{};
  a.segs = segs; a.n_strokes = n_strokes; a.width = width; a.noise = noise; a.N = N; a.size = size; a.normalize = normalize ? 1 : 0; a.image_stride = image_stride;
  a.vec16 = (size % 4 == 0 && image_stride % 4 == 0 && (uintptr_t)x % 16 == 0) ? 1 : 0;
  a.seed = seed; a.offset = offset; a.x = x; a.raw = raw; a.img = img;
  PFN_TRY(launch_stroke_render(a, (hipStream_t)stream));
  return PFN_OK;
}
int pfn_stroke_prior_sample(const int32_t* labels, int B, int T, int num_classes, int size, int normalize, int strokes_lo, int strokes_hi, int len_lo, int len_hi,
                            int start_lo, int start_hi, int width_lo, int width_hi, int max_offset, int max_target_offset, uint64_t seed, uint64_t offset,
                            uint64_t first_dataset, float* x, int32_t* cls_n, int32_t* cls_len, int32_t* cls_start, double* cls_dir, int32_t* segs, int32_t* width,
                            uint8_t* raw, uint8_t* img, int32_t* status, void* stream) {
  if (const int rc = stroke_size("stroke_prior_sample", size)) return rc;
  if (num_classes < 1 || num_classes > PFN_STROKE_MAX_CLASSES || strokes_hi > PFN_STROKE_MAX_STROKES || width_hi > PFN_STROKE_MAX_WIDTH || len_hi > 1024 ||
      start_hi > 1024 || max_offset > 1024 || max_target_offset > 1024)
    return fail(PFN_ERR_UNSUPPORTED, "stroke_prior_sample: num_classes %d outside 1 .. %d, strokes_hi %d above %d, width_hi %d above %d, or len_hi %d, start_hi %d, "
                "max_offset %d, max_target_offset %d above 1024", num_classes, PFN_STROKE_MAX_CLASSES, strokes_hi, PFN_STROKE_MAX_STROKES, width_hi, PFN_STROKE_MAX_WIDTH,
                len_hi, start_hi, max_offset, max_target_offset);
  if (B < 1 || T < 1 || (int64_t)B * T > 0x7fffffffll || strokes_lo < 0 || strokes_lo > strokes_hi || len_lo < 0 || len_lo > len_hi || start_lo < 0 || start_lo > start_hi ||
      width_lo < 0 || width_lo > width_hi || max_offset < 0 || max_target_offset < 0)
    return fail(PFN_ERR_ARGUMENT, "bad stroke_prior_sample arguments (B %d, T %d >= 1, B T < 2^31, 0 <= lo <= hi for strokes %d .. %d, len %d .. %d, start %d .. %d, "
                "width %d .. %d, max_offset %d, max_target_offset %d >= 0)", B, T, strokes_lo, strokes_hi, len_lo, len_hi, start_lo, start_hi, width_lo, width_hi, max_offset,
                max_target_offset);
  if (!labels || !x || !cls_n || !cls_len || !cls_start || !cls_dir || !segs || !width || !status || (uintptr_t)segs % 16 || (uintptr_t)cls_dir % 8 ||
      (uintptr_t)labels % 4 || (uintptr_t)x % 4 || (uintptr_t)cls_n % 4 || (uintptr_t)cls_len % 4 || (uintptr_t)cls_start % 4 || (uintptr_t)width % 4 || (uintptr_t)status % 4)
    return fail(PFN_ERR_ARGUMENT, "bad stroke_prior_sample arguments (only raw and img may be NULL; segs 16-byte, cls_dir 8-byte, the others 4-byte aligned)");
  StrokePriorArgs a{};
  a.labels = labels; a.B = B; a.T = T; a.C = num_classes; a.size = size; a.normalize = normalize ? 1 : 0; a.vec16 = (size % 4 == 0 && (uintptr_t)x % 16 == 0) ? 1 : 0;
  a.strokes_lo = strokes_lo; a.strokes_hi = strokes_hi; a.len_lo = len_lo; a.len_hi = len_hi; a.start_lo = start_lo; a.start_hi = start_hi; a.width_lo = width_lo;
  a.width_hi = width_hi; a.max_off = max_offset; a.max_toff = max_target_offset; a.seed = seed; a.offset = offset; a.first_dataset = first_dataset;
  a.x = x; a.cls_n = cls_n; a.cls_len = cls_len; a.cls_start = cls_start; a.cls_dir = cls_dir; a.segs = segs; a.width = width; a.raw = raw; a.img = img; a.status = status;
  PFN_TRY(launch_stroke_prior(a, (hipStream_t)stream));
  return PFN_OK;
}
}  // extern "C"
