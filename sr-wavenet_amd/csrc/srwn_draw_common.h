// What the draw launches share (csrc/srwn_data.hip, csrc/srwn_draw.hip, csrc/srwn_augment.hip): the order function that
// dataset.draw_plan states in Python -- the splitmix64 finaliser, the keyed permutation of an epoch, a position's record
// and crop offset -- and the row writer, so that a position has one record and a row one store pattern wherever it is drawn.
#pragma once
#include <cmath>
#include "srwn_common.h"
#include "srwn_host.h"
#include "../../include/srwn.h"

namespace srwn {

constexpr int kDrawThreads = 256;
constexpr int kDrawPerThread = 16;                                // samples per thread and pass: 4096 per workgroup
constexpr int kDrawSpan = kDrawThreads * kDrawPerThread;
constexpr int kFeistelRounds = 4;
constexpr unsigned long long kGolden = 0x9E3779B97F4A7C15ull;
constexpr unsigned long long kCropSalt = 0x63726F706F666673ull;  // dataset._CROP_SALT: keeps the offsets' stream apart from the permutations'
constexpr unsigned long long kPairSalt = 0x70616972636F696Eull;       // dataset.PAIR_SALT: the coin
constexpr unsigned long long kPairPickSalt = 0x706169727069636Bull;   // dataset.PAIR_PICK_SALT: the right record
constexpr unsigned long long kPairCropSalt = 0x7061697263726F70ull;   // dataset.PAIR_CROP_SALT: the right crop offset

// the splitmix64 finaliser gen_uniform (srwn_gen_ring.h) keys its draws with
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
  return x;
}

// perm(seed, e)(i): a keyed bijection on [0, N).  kFeistelRounds alternating Feistel rounds on the k = ceil(log2 N) bits of
// the next power of two (the halves have k / 2 and k - k / 2 bits and swap widths every round, so any k works), walked
// until the value is back inside [0, N).  The walk follows one cycle of a permutation of 2^k points that starts inside
// [0, N), so it returns there within 2^k steps: the loop is bounded by the domain size.
__device__ __forceinline__ unsigned feistel_perm(unsigned long long seed, unsigned long long e, unsigned i, unsigned N) {
  if (N <= 1u) return 0u;
  const int k = 32 - __clz((int)(N - 1u));
  const unsigned long long ekey = mix64(seed + kGolden * (e + 1ull));
  unsigned x = i;
  for (unsigned long long walk = 0; walk < (1ull << k); ++walk) {
    int a = k / 2, b = k - a;                                     // x = (L : a bits, R : b bits)
#pragma unroll
    for (int r = 0; r < kFeistelRounds; ++r) {
      const unsigned L = x >> b, R = x & ((1u << b) - 1u);
      const unsigned f = (unsigned)mix64(ekey + kGolden * ((unsigned long long)R * kFeistelRounds + r + 1ull));
      x = (R << a) | (L ^ (f & ((1u << a) - 1u)));
      const int t = a; a = b; b = t;
    }
    if (x < N) return x;
  }
  return i;                                                       // (not reached; inside [0, N) whatever happens)
}

// position p of the sample sequence -> its record and crop offset (dataset.draw_plan)
struct Pick { unsigned rec; int64_t off; };
__device__ __forceinline__ Pick draw_pick(unsigned long long seed, unsigned long long p, int N, int shuffle, int crop,
                                          int64_t clip_len, int T) {
  const unsigned long long e = p / (unsigned long long)N;
  const unsigned i = (unsigned)(p % (unsigned long long)N);
  Pick k;
  k.rec = shuffle ? feistel_perm(seed, e, i, (unsigned)N) : i;
  k.off = 0;
  if (crop) {                                                     // uniform on [0, clip_len - T]
    const unsigned long long h = mix64((seed ^ kCropSalt) + kGolden * (p + 1ull));
    k.off = (int64_t)(((h >> 32) * (unsigned long long)(clip_len - T + 1)) >> 32);
  }
  return k;
}

// one row of T four-byte outputs dst[j] = f(src[j]), this workgroup's share [j0, j1): head, 16-byte body, tail
template <typename Out, typename F>
__device__ __forceinline__ void draw_row(Out* __restrict__ dst, const float* __restrict__ src, int j0, int j1, F f) {
  typedef Out out4 __attribute__((ext_vector_type(4)));
  static_assert(sizeof(Out) == 4, "four-byte outputs");
  // first element of the share whose destination sits on a 16-byte boundary (dst is 4-byte aligned: an fp32 / int32 buffer)
  const int mis = (int)(((uintptr_t)(dst + j0) >> 2) & 3);
  int jb = j0 + ((4 - mis) & 3);
  if (jb > j1) jb = j1;
  const int nvec = (j1 - jb) / 4;
  const int je = jb + 4 * nvec;
  const int tid = (int)threadIdx.x;
  if (tid < jb - j0) dst[j0 + tid] = f(src[j0 + tid]);                          // head: at most 3 elements
  const bool src_aligned = (((uintptr_t)(src + jb)) & 15) == 0;
  for (int v = tid; v < nvec; v += kDrawThreads) {
    const int j = jb + 4 * v;
    f32x4 x;
    if (src_aligned) x = *reinterpret_cast<const f32x4*>(src + j);
    else x = f32x4{src[j], src[j + 1], src[j + 2], src[j + 3]};
    *reinterpret_cast<out4*>(dst + j) = out4{f(x[0]), f(x[1]), f(x[2]), f(x[3])};
  }
  if (tid < j1 - je) dst[je + tid] = f(src[je + tid]);                          // tail: at most 3 elements
}

// row b's one-hot rows (tf.one_hot: a label outside [0, num_classes) gives zeros), by the row's first workgroup
__device__ __forceinline__ void draw_onehot(void* onehot, int dtype, int32_t lab, int b, int rows, int num_classes,
                                            int64_t ld, int col0) {
  const int n = rows * num_classes;
  for (int q = (int)threadIdx.x; q < n; q += kDrawThreads) {
    const int row = q / num_classes, c = q - row * num_classes;
    const int64_t o = ((int64_t)b * rows + row) * ld + col0 + c;
    const float v = (c == lab) ? 1.0f : 0.0f;
    if (dtype == SRWN_BF16) reinterpret_cast<bf16_t*>(onehot)[o] = (bf16_t)v;
    else reinterpret_cast<float*>(onehot)[o] = v;
  }
}

// what srwn_batch_draw and srwn_batch_draw_aug hand their kernels
struct DrawArgs {
  const float* clips; const int32_t* labels; const int64_t* state;
  float* audio0; float* audio1; int32_t* codes; void* onehot; int32_t* indices;
  int64_t clip_len, onehot_ld;
  int32_t N, B, T, shuffle, crop, rank, world, Q, onehot_rows, onehot_col0, num_classes, onehot_dtype;
  float mu, log1p_mu;
};

// ... and srwn_pair_draw and srwn_pair_draw_aug theirs
struct PairArgs {
  const float* clips; const int32_t* labels; const int32_t* order; const int32_t* place; const int32_t* start;
  const int64_t* state;
  float* audio; float* y; int32_t* left; int32_t* right; float* y_log;
  int64_t clip_len; unsigned long long threshold;
  int32_t N, P, T, shuffle, crop, rank, world, num_classes;
};

// ---- the entries' argument checks, host side: everything is refused before any launch (`who` names the entry) ----------
inline int check_draw(const char* who, const float* clips, int32_t num_clips, int64_t clip_len, const int64_t* state, int32_t B,
                      int32_t T, int32_t crop, int32_t rank, int32_t world) {
  if (num_clips < 1 || clip_len < 1 || B < 0 || T < 0 || (int64_t)T > clip_len || clip_len - T >= (1ll << 32))
    return set_error(SRWN_E_SHAPE, "%s: %d clips of %lld samples, B=%d T=%d", who, num_clips, (long long)clip_len, B, T);
  if (world < 1 || rank < 0 || rank >= world) return set_error(SRWN_E_SHAPE, "%s: rank %d of %d", who, rank, world);
  if (crop != 0 && crop != 1) return set_error(SRWN_E_SHAPE, "%s: crop %d (0 head, 1 random)", who, crop);
  if (!clips || !state) return set_error(SRWN_E_NULL, "%s: null pointer", who);
  return 0;
}

// srwn_batch_draw's arguments (and srwn_batch_draw_aug's in front of its augmentation block) into `a`
inline int check_batch_draw(const char* who, const float* clips, const int32_t* labels, int32_t num_clips, int64_t clip_len,
                            const int64_t* state, int32_t B, int32_t T, int32_t shuffle, int32_t crop, int32_t rank,
                            int32_t world, float* audio0, float* audio1, int32_t* codes, int32_t quantization_channels,
                            void* onehot, int64_t onehot_ld, int32_t onehot_rows, int32_t onehot_col0, int32_t num_classes,
                            int32_t onehot_dtype, int32_t* indices, DrawArgs* out) {
  if (num_clips < 1 || clip_len < 1 || B < 0 || T < 0 || (int64_t)T > clip_len || clip_len - T >= (1ll << 32))
    return set_error(SRWN_E_SHAPE, "%s: %d clips of %lld samples, B=%d T=%d", who, num_clips, (long long)clip_len, B, T);
  if (B > 65535) return set_error(SRWN_E_SHAPE, "%s: B=%d (at most 65535 rows per draw)", who, B);
  if (world < 1 || rank < 0 || rank >= world) return set_error(SRWN_E_SHAPE, "%s: rank %d of %d", who, rank, world);
  if (crop != 0 && crop != 1) return set_error(SRWN_E_SHAPE, "%s: crop %d (0 head, 1 random)", who, crop);
  if (!clips || !state || !audio0 || !indices) return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if (codes && quantization_channels < 2) return set_error(SRWN_E_SHAPE, "%s: Q=%d", who, quantization_channels);
  if (onehot) {
    if (!labels) return set_error(SRWN_E_NULL, "%s: one-hot rows need the labels", who);
    if (onehot_dtype != SRWN_F32 && onehot_dtype != SRWN_BF16) return set_error(SRWN_E_DTYPE, "%s: one-hot dtype %d", who, onehot_dtype);
    if (num_classes < 1 || onehot_rows < 1 || onehot_col0 < 0 || onehot_ld < (int64_t)onehot_col0 + num_classes ||
        (int64_t)onehot_rows * num_classes > (1ll << 30))
      return set_error(SRWN_E_SHAPE, "%s: one-hot %d rows x %d classes at column %d, ld %lld", who, onehot_rows,
                       num_classes, onehot_col0, (long long)onehot_ld);
  }
  if (((uintptr_t)clips | (uintptr_t)audio0 | (uintptr_t)audio1 | (uintptr_t)codes) & 3)
    return set_error(SRWN_E_SHAPE, "%s: the fp32 / int32 buffers must be 4-byte aligned", who);
  DrawArgs& a = *out;
  a.clips = clips; a.labels = labels; a.state = state;
  a.audio0 = audio0; a.audio1 = audio1; a.codes = codes; a.onehot = onehot; a.indices = indices;
  a.clip_len = clip_len; a.onehot_ld = onehot_ld;
  a.N = num_clips; a.B = B; a.T = T; a.shuffle = shuffle != 0; a.crop = crop; a.rank = rank; a.world = world;
  a.Q = quantization_channels; a.onehot_rows = onehot_rows; a.onehot_col0 = onehot_col0; a.num_classes = num_classes;
  a.onehot_dtype = onehot_dtype;
  a.mu = codes ? (float)(quantization_channels - 1) : 0.0f;                // (srwn_mu_law_encode's constants)
  a.log1p_mu = codes ? (float)log1p((double)a.mu) : 0.0f;
  return 0;
}

// srwn_pair_draw's arguments (and srwn_pair_draw_aug's in front of its augmentation block) into `a`
inline int check_pair_draw(const char* who, const float* clips, const int32_t* labels, const int32_t* order,
                           const int32_t* place, const int32_t* class_start, int32_t num_classes, int32_t num_clips,
                           int64_t clip_len, const int64_t* state, int32_t P, int32_t T, int64_t same_threshold,
                           int32_t shuffle, int32_t crop, int32_t rank, int32_t world, float* audio, float* y, int32_t* left,
                           int32_t* right, float* y_log, PairArgs* out) {
  if (int rc = check_draw(who, clips, num_clips, clip_len, state, P, T, crop, rank, world)) return rc;
  if (num_classes < 1) return set_error(SRWN_E_SHAPE, "%s: %d classes", who, num_classes);
  if (P > 32767) return set_error(SRWN_E_SHAPE, "%s: P=%d (at most 32767 pairs per draw)", who, P);
  if (same_threshold < 0 || same_threshold > (1ll << 32))
    return set_error(SRWN_E_SHAPE, "%s: same_threshold %lld outside [0, 2^32]", who, (long long)same_threshold);
  if (!labels || !order || !place || !class_start || !audio || !y || !left || !right || !y_log)
    return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if (((uintptr_t)clips | (uintptr_t)audio) & 3)
    return set_error(SRWN_E_SHAPE, "%s: the fp32 buffers must be 4-byte aligned", who);
  PairArgs& a = *out;
  a.clips = clips; a.labels = labels; a.order = order; a.place = place; a.start = class_start; a.state = state;
  a.audio = audio; a.y = y; a.left = left; a.right = right; a.y_log = y_log;
  a.clip_len = clip_len; a.threshold = (unsigned long long)same_threshold;
  a.N = num_clips; a.P = P; a.T = T; a.shuffle = shuffle != 0; a.crop = crop; a.rank = rank; a.world = world;
  a.num_classes = num_classes;
  return 0;
}

}  // namespace srwn
