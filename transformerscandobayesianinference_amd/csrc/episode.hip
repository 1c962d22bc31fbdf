// The Omniglot episode loader of the few-shot study (reference priors/omniglot.py:13-35, :58-72; datasets/omniglotNshot.py:31-77, :172-230) over an image bank
// that lives on the device: per step it picks classes and images without replacement, rotates each class by a multiple of 90 degrees, shuffles, measures each
// image's bounding box, draws a shift that keeps the glyph in frame and shifts the image.  The reference does that in a numpy loop over datasets, classes and
// images with one torchvision affine() per image; here one call draws a batch.  The kernels move data and do no arithmetic on pixels.
//
// ---- the image kernel: one wave per image, four waves per block ----
// The source image is read once, coalesced, into the wave's LDS image as f32 values (the uint8 bank through its 256-entry table), rows padded to the odd
// stride P = size | 1 so that a walk along a row AND along a column touches distinct banks -- a rotated read is a column walk.  While it loads, every lane
// collects two 64-bit masks from its own pixels: the source rows and the source columns in which one of them is not 0 (bit y = 1ull << y, the four column bits of
// an item at 4 xq .. 4 xq + 3 <= 63: no mask is built by a shift by `size`, so size 64 needs no special case).  An OR-reduction of each over the wave is the
// source's row and column occupancy; the bounding box of the ROTATED image follows from those by index arithmetic, as rotation and shift do on the way out:
//     rot90 k = 1: rot[i][j] = src[j][n-1-i];   k = 2: src[n-1-i][n-1-j];   k = 3: src[n-1-j][i]      (np.rot90(a, k, axes=(-2, -1)), n = size)
//     out[y][x] = rot[y - ty][x - tx] inside the frame, else 0.0f                                       (affine(translate=[tx, ty], NEAREST, fill=0), restated)
// Output: items of four horizontally adjacent pixels, one 16-byte store per lane when size % 4 == 0 and the image is 16-byte aligned, dword stores otherwise.
//
// ---- the draw kernel: one block of 64 threads per dataset, every array in LDS (no scratch) ----
// Words of Philox4x32-10 blocks, counter = a global index, stream word = offset * 8 + purpose, key = seed; word m of a run is component m % 4 of the block at
// base + m / 4.  An integer in [lo, hi] is lo + mulhi(u32, hi - lo + 1) (bias below (hi - lo + 1) 2^-32 per value).
//   k-SUBSET of n (ordered, without replacement), the "rank rule": draw j = 0 .. k-1 takes r = mulhi(word j, n - j), the rank of the pick among the n - j values
//   not yet taken; walking the taken values in ascending order, r += 1 for each one <= r.  Every ordered selection has probability prod 1 / (n - j), each factor
//   with the mulhi bias below (n - j) 2^-32.
//   PERMUTATION of n: Fisher-Yates, for i = n-1 .. 1: swap(a[i], a[mulhi(word n-1-i, i + 1)]).
// With d = first_dataset + b, T = n_way k_shot + 1, S = T - 1:
//   purpose 0 (classes)   base d * 4:             standard: the n_way-subset of the pool;  jonas: the permutation of range(n_way)
//   purpose 1 (images)    base (d * 16 + j) * 16:  class j (selection position j): the k_shot-subset of n_img, and for the query class one more draw of the same
//                                                   run (draw k_shot);  jonas test: the permutation of range(k_shot), then word k_shot - 1 -> query in k_shot .. n_img-1
//   purpose 2 (misc)      counter d:               .x the query class in [0, n_way), .y the alphabet in [0, A)
//   purpose 3 (rotation)  base d * 4:              word j: quarter turns of class j (standard mode)
//   purpose 4 (shuffle)   base d * 256:            the permutation of the S support positions (standard mode)
//   purpose 5 (shift)     counter g = d * T + t (pfn_episode_gather: first_image + n):  .x -> tx in [-c0, size-1-c1], .y -> ty in [-r0, size-1-r1]
//
// standard mode (OmniglotNShot.load_data_cache): :190 classes without replacement from the pool, :192 label j = position in the selection, :194 k_shot + 1 images
// without replacement (here k_shot for every class and the one more only for the class whose query is used), :196-202 one rotation per class for support and
// query alike, :207-209 one permutation of the class-major support list, :210-212 with priors/omniglot.py:61 x_q[:, :1]: of the permuted n_way queries the first
// is kept = one class uniformly.  The cache of ten batches (:184) only amortises the loop: draws here are fresh.
// jonas mode (OmniglotNShotJonas.next): :38 alphabet uniformly with replacement, :43 classes = permutation(n_way) -- the FIRST n_way classes of the alphabet, the
// reference permutes range(n_way), not the alphabet's classes --, :49-51 train: k_shot + 1 of n_img without replacement, :53-54 test: support = permutation of
// images 0 .. k_shot-1, query uniform in k_shot .. n_img-1, :68 labels = position, support class-major and unshuffled, :72-75 with :61 one query uniformly.
#include "pfn_device.h"
#include "pfn_host.h"

namespace pfn {

struct EpisodeImageArgs {
  const void* bank;            // [n_src, size, size] f32, or uint8 with table
  const float* table;          // [256] or null
  const int32_t* src;          // [N] flat class * n_img + image
  const int32_t* rot;          // [N], or with labels: [N / T, n_way] indexed through labels; null: no rotation
  const int32_t* labels;       // [N] or null
  const int32_t* shift_in;     // [N,2] or null
  long N;
  int n_src, size, translate, vec_in, vec_out, n_way;
  int T, B;                    // T > 0: image n = b T + t is written at x + (t B + b) size^2; T == 0: at x + n image_stride
  long image_stride;
  unsigned long long seed, offset, first_image;
  float* x;
  int32_t* bbox;               // [N,4] = (c0, c1, r0, r1); no content: (0, -1, 0, -1)
  int32_t* shift;              // [N,2] = (tx, ty)
};
struct EpisodeDrawArgs {
  int B, T, n_way, k_shot, n_img, n_classes, mode, train, pool_lo, pool_hi, n_alphabets;
  const int32_t* alphabet_offsets;      // [A + 1] (jonas)
  unsigned long long seed, offset, first_dataset;
  int32_t* labels;             // [B,T]
  int32_t* targets;            // [B,T]
  int32_t* classes;            // [B,n_way]
  int32_t* rotations;          // [B,n_way]
  int32_t* src;                // [B,T]
};

constexpr int EP_WAVES = 4;
enum { EP_STREAM_CLASS = 0, EP_STREAM_IMAGE = 1, EP_STREAM_MISC = 2, EP_STREAM_ROT = 3, EP_STREAM_SHUFFLE = 4, EP_STREAM_SHIFT = 5 };      // stream word = offset * 8 + purpose

PFN_DEV int ep_int(unsigned u, int lo, int hi) { return lo + (int)__umulhi(u, (unsigned)(hi - lo + 1)); }
PFN_DEV int ep_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// floats of dynamic LDS: the table, then one padded image per wave
static size_t episode_lds_bytes(int size) { return (256 + (size_t)EP_WAVES * size * (size | 1)) * sizeof(float); }

template <typename PIX>
__global__ __launch_bounds__(256) void episode_image_kernel(EpisodeImageArgs a) {
  extern __shared__ float ep_lds[];
  constexpr bool BYTES = sizeof(PIX) == 1;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int size = a.size, P = size | 1, px = size * size;
  float* tab = ep_lds;
  float* img = ep_lds + 256 + wave * (size * P);
  const long n = (long)blockIdx.x * EP_WAVES + wave;
  const bool active = n < a.N;
  const int W = (size + 3) >> 2, nitems = size * W, rounds = (nitems + 63) >> 6;
  if constexpr (BYTES) {
    tab[threadIdx.x] = a.table[threadIdx.x];
    __syncthreads();
  }
  int k = 0, c0 = 0, c1 = -1, r0 = 0, r1 = -1, tx = 0, ty = 0;
  bool empty = true;
  if (active) {
    const int s = ep_clamp(a.src[n], 0, a.n_src - 1);
    if (a.rot) k = ep_clamp(a.labels ? a.rot[(n / a.T) * a.n_way + ep_clamp(a.labels[n], 0, a.n_way - 1)] : a.rot[n], 0, 3);
    const PIX* im = reinterpret_cast<const PIX*>(a.bank) + (long)s * px;
    uint64_t rows = 0, cols = 0;      // this lane's share: bit y / bit x set where one of its pixels of source row y / column x is not 0
    for (int r = 0; r < rounds; ++r) {
      const int i = r * 64 + lane;
      if (i < nitems) {
        const int y = i / W, xq = i - y * W;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (a.vec_in) {      // size % 4 == 0: pixel y * size + 4 xq is element 4 i
          if constexpr (BYTES) {
            const unsigned w = *reinterpret_cast<const unsigned*>(im + 4 * i);
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = tab[(w >> (8 * c)) & 255u];
          } else {
            const f32x4 w = *reinterpret_cast<const f32x4*>(im + 4 * i);
            v[0] = w[0]; v[1] = w[1]; v[2] = w[2]; v[3] = w[3];
          }
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (4 * xq + c < size) {
              if constexpr (BYTES) v[c] = tab[im[y * size + 4 * xq + c]];
              else v[c] = im[y * size + 4 * xq + c];
            }
        }
        unsigned nib = 0;      // (a pixel beyond the row's end stayed 0.f)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (4 * xq + c < size) img[y * P + 4 * xq + c] = v[c];
          nib |= (v[c] != 0.f ? 1u : 0u) << c;
        }
        cols |= (uint64_t)nib << (4 * xq);      // 4 xq + 3 <= 63: at size 64 the last item's bits are 60 .. 63
        rows |= (uint64_t)(nib ? 1u : 0u) << y;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      rows |= (uint64_t)__shfl_xor((unsigned long long)rows, o);
      cols |= (uint64_t)__shfl_xor((unsigned long long)cols, o);
    }
    empty = rows == 0;
    if (!empty) {
      const int sr0 = __builtin_ctzll(rows), sr1 = 63 - __builtin_clzll(rows), sc0 = __builtin_ctzll(cols), sc1 = 63 - __builtin_clzll(cols);
      const int m = size - 1;
      // rot row i <- k 1: source column m - i, k 2: source row m - i, k 3: source column i;  rot column j <- k 1: source row j, k 2: source column m - j, k 3: source row m - j
      r0 = k == 0 ? sr0 : k == 1 ? m - sc1 : k == 2 ? m - sr1 : sc0;
      r1 = k == 0 ? sr1 : k == 1 ? m - sc0 : k == 2 ? m - sr0 : sc1;
      c0 = k == 0 ? sc0 : k == 1 ? sr0 : k == 2 ? m - sc1 : m - sr1;
      c1 = k == 0 ? sc1 : k == 1 ? sr1 : k == 2 ? m - sc0 : m - sr0;
    }
  }
  __syncthreads();      // the LDS images are complete (a wave reads only its own, but columns written by other lanes)
  if (!active) return;
  if (a.shift_in) {      // from device memory: beyond +-size every shift empties the frame alike
    tx = ep_clamp(a.shift_in[2 * n], -size, size);
    ty = ep_clamp(a.shift_in[2 * n + 1], -size, size);
  } else if (a.translate && !empty) {
    const U4 u = philox4x32_10(a.first_image + (unsigned long long)n, a.offset * 8ull + EP_STREAM_SHIFT, a.seed);
    tx = ep_int(u.x, -c0, size - 1 - c1);
    ty = ep_int(u.y, -r0, size - 1 - r1);
  }
  if (lane < 4) a.bbox[4 * n + lane] = lane == 0 ? c0 : lane == 1 ? c1 : lane == 2 ? r0 : r1;
  if (lane < 2) a.shift[2 * n + lane] = lane == 0 ? tx : ty;
  // LDS index of rot[ry][rx] = base + ry cy + rx cx
  const int m = size - 1;
  const int cy = k == 0 ? P : k == 1 ? -1 : k == 2 ? -P : 1;
  const int cx = k == 0 ? 1 : k == 1 ? P : k == 2 ? -1 : -P;
  const int base = k == 0 ? 0 : k == 1 ? m : k == 2 ? m * (P + 1) : m * P;
  float* out = a.T > 0 ? a.x + ((n % a.T) * a.B + n / a.T) * px : a.x + n * a.image_stride;
  for (int r = 0; r < rounds; ++r) {
    const int i = r * 64 + lane;
    if (i < nitems) {
      const int y = i / W, xq = i - y * W, ry = y - ty;
      float v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int rx = 4 * xq + c - tx;
        const bool inside = (unsigned)ry < (unsigned)size && (unsigned)rx < (unsigned)size;
        v[c] = img[inside ? base + ry * cy + rx * cx : 0];
        v[c] = inside ? v[c] : 0.f;
      }
      if (a.vec_out) {
        *reinterpret_cast<f32x4*>(out + 4 * i) = f32x4{v[0], v[1], v[2], v[3]};
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (4 * xq + c < size) out[y * size + 4 * xq + c] = v[c];
      }
    }
  }
}

// status[g] = images without content among images g L .. (g + 1) L - 1: one block of up to 1024 threads per group, no atomics
__global__ __launch_bounds__(1024) void episode_count_kernel(const int32_t* bbox, long L, int32_t* status) {
  __shared__ int part[16];
  const long g = blockIdx.x;
  int count = 0;
  for (long i = threadIdx.x; i < L; i += blockDim.x) {
    const int32_t* b = bbox + (g * L + i) * 4;
    count += b[1] < b[0] ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o);
  if (lane_id() == 0) part[threadIdx.x >> 6] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) total += part[w];
    status[g] = total;
  }
}

// a run of Philox words: word m is component m % 4 of the block at base + m / 4
struct EpWords {
  unsigned long long base, stream, seed;
  U4 u;
  int m;
  PFN_DEV unsigned next() {
    if ((m & 3) == 0) u = philox4x32_10(base + (unsigned)(m >> 2), stream, seed);
    const unsigned w = (m & 3) == 0 ? u.x : (m & 3) == 1 ? u.y : (m & 3) == 2 ? u.z : u.w;
    ++m;
    return w;
  }
};

// draw j of the rank rule: `taken` holds the j values taken so far in ascending order
template <typename E> PFN_DEV int ep_take(E* taken, int j, int n, unsigned word) {
  int r = (int)__umulhi(word, (unsigned)(n - j)), pos = 0;
  while (pos < j && r >= (int)taken[pos]) { ++r; ++pos; }
  for (int q = j; q > pos; --q) taken[q] = taken[q - 1];
  taken[pos] = (E)r;
  return r;
}
template <typename E> PFN_DEV void ep_permute(E* v, int n, EpWords& w) {
  for (int i = 0; i < n; ++i) v[i] = (E)i;
  for (int i = n - 1; i >= 1; --i) {
    const int j = (int)__umulhi(w.next(), (unsigned)(i + 1));
    const E t = v[i]; v[i] = v[j]; v[j] = t;
  }
}

__global__ __launch_bounds__(64) void episode_draw_kernel(EpisodeDrawArgs a) {
  __shared__ int cls[PFN_EPISODE_MAX_WAY], cls_taken[PFN_EPISODE_MAX_WAY], rots[PFN_EPISODE_MAX_WAY];
  __shared__ unsigned char img[PFN_EPISODE_MAX_WAY][PFN_EPISODE_MAX_IMAGES], img_taken[PFN_EPISODE_MAX_WAY][PFN_EPISODE_MAX_IMAGES];
  __shared__ unsigned short perm[PFN_EPISODE_MAX_WAY * PFN_EPISODE_MAX_IMAGES];
  const int b = blockIdx.x, lane = threadIdx.x;
  const unsigned long long d = a.first_dataset + (unsigned long long)b;
  const int S = a.n_way * a.k_shot;
  const bool jonas = a.mode == PFN_EPISODE_JONAS;
  const U4 misc = philox4x32_10(d, a.offset * 8ull + EP_STREAM_MISC, a.seed);
  const int q = (int)__umulhi(misc.x, (unsigned)a.n_way);
  if (lane == 0) {
    EpWords w{d * 4ull, a.offset * 8ull + EP_STREAM_CLASS, a.seed, U4{0, 0, 0, 0}, 0};
    if (jonas) {
      const int first = a.alphabet_offsets[__umulhi(misc.y, (unsigned)a.n_alphabets)];
      ep_permute(cls, a.n_way, w);
      for (int j = 0; j < a.n_way; ++j) cls[j] = ep_clamp(first + cls[j], 0, a.n_classes - 1);
    } else {
      for (int j = 0; j < a.n_way; ++j) cls[j] = a.pool_lo + ep_take(cls_taken, j, a.pool_hi - a.pool_lo, w.next());
    }
    if (jonas) {
      for (int p = 0; p < S; ++p) perm[p] = (unsigned short)p;
    } else {
      EpWords ws{d * 256ull, a.offset * 8ull + EP_STREAM_SHUFFLE, a.seed, U4{0, 0, 0, 0}, 0};
      ep_permute(perm, S, ws);
    }
  }
  if (lane < a.n_way) {
    const int j = lane;
    EpWords w{(d * 16ull + (unsigned)j) * 16ull, a.offset * 8ull + EP_STREAM_IMAGE, a.seed, U4{0, 0, 0, 0}, 0};
    if (jonas && !a.train) {
      ep_permute(img[j], a.k_shot, w);      // k_shot - 1 words
      const unsigned word = w.next();
      if (j == q) img[j][a.k_shot] = (unsigned char)(a.k_shot + (int)__umulhi(word, (unsigned)(a.n_img - a.k_shot)));
    } else {
      const int draws = a.k_shot + (j == q ? 1 : 0);
      for (int i = 0; i < draws; ++i) img[j][i] = (unsigned char)ep_take(img_taken[j], i, a.n_img, w.next());
    }
    int rot = 0;
    if (!jonas) {
      EpWords wr{d * 4ull, a.offset * 8ull + EP_STREAM_ROT, a.seed, U4{0, 0, 0, 0}, j};
      if (j & 3) wr.u = philox4x32_10(wr.base + (unsigned)(j >> 2), wr.stream, wr.seed);
      rot = (int)__umulhi(wr.next(), 4u);
    }
    rots[j] = rot;
  }
  __syncthreads();
  if (lane < a.n_way) {
    a.classes[(long)b * a.n_way + lane] = cls[lane];
    a.rotations[(long)b * a.n_way + lane] = rots[lane];
  }
  for (int p = lane; p < a.T; p += 64) {
    int j = q, i = a.k_shot;
    if (p < S) {
      const int e = perm[p];
      j = e / a.k_shot;
      i = e - j * a.k_shot;
    }
    const long g = (long)b * a.T + p;
    a.labels[g] = j;
    a.targets[g] = p < S ? -100 : j;
    a.src[g] = cls[j] * a.n_img + (int)img[j][i];
  }
}

static int launch_episode_images(const EpisodeImageArgs& a, hipStream_t s) {
  static LdsAllowance allow_f32, allow_u8;
  const dim3 grid((unsigned)((a.N + EP_WAVES - 1) / EP_WAVES));
  if (a.table) return launch_lds(episode_image_kernel<uint8_t>, allow_u8, grid, dim3(256), episode_lds_bytes(a.size), s, a);
  return launch_lds(episode_image_kernel<float>, allow_f32, grid, dim3(256), episode_lds_bytes(a.size), s, a);
}

static int launch_episode_count(const int32_t* bbox, long groups, long L, int32_t* status, hipStream_t s) {
  const long threads = L >= 1024 ? 1024 : (L + 63) / 64 * 64;
  hipLaunchKernelGGL(episode_count_kernel, dim3((unsigned)groups), dim3((unsigned)threads), 0, s, bbox, L, status);
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

static int launch_episode_draw(const EpisodeDrawArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(episode_draw_kernel, dim3(a.B), dim3(64), 0, s, a);
  return hipGetLastError() == hipSuccess ? PFN_OK : PFN_ERR_LAUNCH;
}

// what both entry points ask of the bank
static int episode_bank(const char* what, const void* bank, const float* table, int n_classes, int n_img, int size) {
  if (size < PFN_EPISODE_MIN_SIZE || size > PFN_EPISODE_MAX_SIZE)
    return fail(PFN_ERR_UNSUPPORTED, "%s: size %d outside 8 .. 64 (one lane per row, a row's mask in 64 bits)", what, size);
  if (n_img < 1 || n_img > PFN_EPISODE_MAX_IMAGES) return fail(PFN_ERR_UNSUPPORTED, "%s: n_img %d outside 1 .. %d", what, n_img, PFN_EPISODE_MAX_IMAGES);
  if (n_classes < 1 || (int64_t)n_classes * n_img > 0x7fffffffll)
    return fail(PFN_ERR_ARGUMENT, "bad %s arguments (n_classes %d >= 1, n_classes n_img < 2^31)", what, n_classes);
  if (!bank || (uintptr_t)table % 4 || (!table && (uintptr_t)bank % 4))
    return fail(PFN_ERR_ARGUMENT, "bad %s arguments (bank not NULL; an f32 bank and the table 4-byte aligned)", what);
  return PFN_OK;
}
static int episode_vec_in(const void* bank, const float* table, int size) { return (size % 4 == 0 && (uintptr_t)bank % (table ? 4 : 16) == 0) ? 1 : 0; }

}  // namespace pfn

using namespace pfn;

extern "C" {
int pfn_episode_gather(const void* bank, const float* table, int n_classes, int n_img, int size, const int32_t* src, const int32_t* rot, const int32_t* shift_in,
                       int64_t N, int translate, int64_t image_stride, uint64_t seed, uint64_t offset, uint64_t first_image, float* x, int32_t* bbox, int32_t* shift,
                       int32_t* status, void* stream) {
  if (const int rc = episode_bank("episode_gather", bank, table, n_classes, n_img, size)) return rc;
  if (N < 0 || N > 0x7fffffffll || image_stride < (int64_t)size * size)
    return fail(PFN_ERR_ARGUMENT, "bad episode_gather arguments (0 <= N %lld < 2^31, image_stride %lld >= size^2)", (long long)N, (long long)image_stride);
  if (!src || !x || !bbox || !shift || (uintptr_t)src % 4 || (uintptr_t)rot % 4 || (uintptr_t)shift_in % 4 || (uintptr_t)x % 4 || (uintptr_t)bbox % 4 ||
      (uintptr_t)shift % 4 || (uintptr_t)status % 4)
    return fail(PFN_ERR_ARGUMENT, "bad episode_gather arguments (src, x, bbox, shift not NULL; every buffer 4-byte aligned)");
  if (N == 0) return PFN_OK;
  EpisodeImageArgs a{};
  a.bank = bank; a.table = table; a.src = src; a.rot = rot; a.labels = nullptr; a.shift_in = shift_in; a.N = N; a.n_src = n_classes * n_img; a.size = size;
  a.translate = translate ? 1 : 0; a.vec_in = episode_vec_in(bank, table, size);
  a.vec_out = (size % 4 == 0 && image_stride % 4 == 0 && (uintptr_t)x % 16 == 0) ? 1 : 0;
  a.n_way = 1; a.T = 0; a.B = 0; a.image_stride = image_stride; a.seed = seed; a.offset = offset; a.first_image = first_image; a.x = x; a.bbox = bbox; a.shift = shift;
  PFN_TRY(launch_episode_images(a, (hipStream_t)stream));
  if (status) PFN_TRY(launch_episode_count(bbox, 1, N, status, (hipStream_t)stream));
  return PFN_OK;
}

int pfn_episode_sample(const void* bank, const float* table, int n_classes, int n_img, int size, int B, int n_way, int k_shot, int mode, int train, int translate,
                       int pool_lo, int pool_hi, const int32_t* alphabet_offsets, int n_alphabets, uint64_t seed, uint64_t offset, uint64_t first_dataset, float* x,
                       int32_t* labels, int32_t* targets, int32_t* classes, int32_t* rotations, int32_t* src, int32_t* shift, int32_t* bbox, int32_t* status,
                       void* stream) {
  if (const int rc = episode_bank("episode_sample", bank, table, n_classes, n_img, size)) return rc;
  if (n_way < 1 || n_way > PFN_EPISODE_MAX_WAY) return fail(PFN_ERR_UNSUPPORTED, "episode_sample: n_way %d outside 1 .. %d", n_way, PFN_EPISODE_MAX_WAY);
  if (mode != PFN_EPISODE_STANDARD && mode != PFN_EPISODE_JONAS) return fail(PFN_ERR_UNSUPPORTED, "episode_sample: mode %d is neither standard (0) nor jonas (1)", mode);
  if (k_shot < 1 || k_shot >= n_img) return fail(PFN_ERR_ARGUMENT, "bad episode_sample arguments (1 <= k_shot %d < n_img %d)", k_shot, n_img);
  const int64_t T = (int64_t)n_way * k_shot + 1;
  if (B < 0 || (int64_t)B * T > 0x7fffffffll) return fail(PFN_ERR_ARGUMENT, "bad episode_sample arguments (B %d >= 0, B T < 2^31)", B);
  if (mode == PFN_EPISODE_STANDARD && (pool_lo < 0 || pool_hi > n_classes || pool_hi - pool_lo < n_way))
    return fail(PFN_ERR_ARGUMENT, "bad episode_sample arguments (the pool [%d, %d) inside [0, %d) holds at least n_way %d classes)", pool_lo, pool_hi, n_classes, n_way);
  if (mode == PFN_EPISODE_JONAS && (!alphabet_offsets || n_alphabets < 1 || (uintptr_t)alphabet_offsets % 4))
    return fail(PFN_ERR_ARGUMENT, "bad episode_sample arguments (jonas mode: alphabet_offsets [n_alphabets + 1] not NULL, 4-byte aligned, n_alphabets %d >= 1)", n_alphabets);
  if (!x || !labels || !targets || !classes || !rotations || !src || !shift || !bbox || !status || (uintptr_t)x % 4 || (uintptr_t)labels % 4 ||
      (uintptr_t)targets % 4 || (uintptr_t)classes % 4 || (uintptr_t)rotations % 4 || (uintptr_t)src % 4 || (uintptr_t)shift % 4 || (uintptr_t)bbox % 4 ||
      (uintptr_t)status % 4)
    return fail(PFN_ERR_ARGUMENT, "bad episode_sample arguments (no output may be NULL; every buffer 4-byte aligned)");
  if (B == 0) return PFN_OK;
  EpisodeDrawArgs dr{};
  dr.B = B; dr.T = (int)T; dr.n_way = n_way; dr.k_shot = k_shot; dr.n_img = n_img; dr.n_classes = n_classes; dr.mode = mode; dr.train = train ? 1 : 0;
  dr.pool_lo = pool_lo; dr.pool_hi = pool_hi; dr.n_alphabets = n_alphabets; dr.alphabet_offsets = alphabet_offsets; dr.seed = seed; dr.offset = offset;
  dr.first_dataset = first_dataset; dr.labels = labels; dr.targets = targets; dr.classes = classes; dr.rotations = rotations; dr.src = src;
  EpisodeImageArgs a{};
  a.bank = bank; a.table = table; a.src = src; a.rot = mode == PFN_EPISODE_STANDARD ? rotations : nullptr; a.labels = labels; a.shift_in = nullptr; a.N = (long)B * T;
  a.n_src = n_classes * n_img; a.size = size; a.translate = translate ? 1 : 0; a.vec_in = episode_vec_in(bank, table, size);
  a.vec_out = (size % 4 == 0 && (uintptr_t)x % 16 == 0) ? 1 : 0;
  a.n_way = n_way; a.T = (int)T; a.B = B; a.image_stride = (long)size * size; a.seed = seed; a.offset = offset; a.first_image = first_dataset * (uint64_t)T;
  a.x = x; a.bbox = bbox; a.shift = shift;
  PFN_TRY(launch_episode_draw(dr, (hipStream_t)stream));
  PFN_TRY(launch_episode_images(a, (hipStream_t)stream));
  PFN_TRY(launch_episode_count(bbox, B, T, status, (hipStream_t)stream));
  return PFN_OK;
}
}  // extern "C"
