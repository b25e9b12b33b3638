// Device-resident datasets (srwn.h, srwn_version() 122): the two launches that ride in the training step's graph when a
// BatchSampler (sr-wavenet_amd/dataset.py) feeds it.
//
//   srwn_batch_draw   reads {seed, step} from device memory, computes the step's B records and crop offsets -- the order
//                     function dataset.draw_plan states in Python -- and writes, in that one launch, everything the
//                     engines' set_inputs writes from a host batch: the cropped fp32 rows (into one or two audio buffers),
//                     the mu-law targets (mu_law_encode_one of srwn_mulaw.h: the bits of srwn_mu_law_encode), the one-hot
//                     label rows and the drawn record indices.
//   srwn_step_log     the step's last launch: log[step % capacity] = loss, then step += 1.  The tick lives here and not in
//                     the draw, whose workgroups all read `step`: no workgroup of a launch may change what the others read.
//
// A draw moves B * T * 4 bytes in and 4 (one audio buffer) to 12 (two audio buffers and the codes) bytes per sample out; the
// second and third passes over a row read it from the caches.  Rows start at any element -- the clip length, the crop offset
// and T are arbitrary -- so each row is written as a scalar head up to the destination's 16-byte boundary, 16-byte stores
// (16-byte loads where the source happens to share the alignment, four scalar loads elsewhere) and a scalar tail.
#include "srwn_common.h"
#include "srwn_host.h"
#include "srwn_mulaw.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

constexpr int kDrawThreads = 256;
constexpr int kDrawPerThread = 16;                                // samples per thread and pass: 4096 per workgroup
constexpr int kDrawSpan = kDrawThreads * kDrawPerThread;
constexpr int kFeistelRounds = 4;
constexpr unsigned long long kGolden = 0x9E3779B97F4A7C15ull;
constexpr unsigned long long kCropSalt = 0x63726F706F666673ull;  // keeps the offsets' stream apart from the permutations'

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

struct DrawArgs {
  const float* clips; const int32_t* labels; const int64_t* state;
  float* audio0; float* audio1; int32_t* codes; void* onehot; int32_t* indices;
  int64_t clip_len, onehot_ld;
  int32_t N, B, T, shuffle, crop, rank, world, Q, onehot_rows, onehot_col0, num_classes, onehot_dtype;
  float mu, log1p_mu;
};

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

__global__ __launch_bounds__(kDrawThreads) void batch_draw_kernel(const DrawArgs a) {
  const int b = (int)blockIdx.y;
  // the order function (dataset.draw_plan): position p, epoch e, place i, record perm(seed, e)(i), crop offset
  const unsigned long long seed = (unsigned long long)a.state[0], step = (unsigned long long)a.state[1];
  const unsigned long long p = (step * (unsigned long long)a.world + (unsigned long long)a.rank) * (unsigned long long)a.B + (unsigned long long)b;
  const unsigned long long e = p / (unsigned long long)a.N;
  const unsigned i = (unsigned)(p % (unsigned long long)a.N);
  const unsigned rec = a.shuffle ? feistel_perm(seed, e, i, (unsigned)a.N) : i;
  int64_t off = 0;
  if (a.crop) {                                                   // uniform on [0, clip_len - T]
    const unsigned long long h = mix64((seed ^ kCropSalt) + kGolden * (p + 1ull));
    off = (int64_t)(((h >> 32) * (unsigned long long)(a.clip_len - a.T + 1)) >> 32);
  }
  const float* src = a.clips + (int64_t)rec * a.clip_len + off;
  const int j0 = (int)blockIdx.x * kDrawSpan;
  const int j1 = min(a.T, j0 + kDrawSpan);
  draw_row(a.audio0 + (int64_t)b * a.T, src, j0, j1, [](float x) { return x; });
  if (a.audio1) draw_row(a.audio1 + (int64_t)b * a.T, src, j0, j1, [](float x) { return x; });
  if (a.codes) {
    const float mu = a.mu, l1p = a.log1p_mu;
    draw_row(a.codes + (int64_t)b * a.T, src, j0, j1, [mu, l1p](float x) { return mu_law_encode_one(x, mu, l1p); });
  }
  if (blockIdx.x != 0) return;
  if (threadIdx.x == 0) a.indices[b] = (int32_t)rec;
  if (a.onehot) {                                                 // tf.one_hot: a label outside [0, num_classes) gives zeros
    const int32_t lab = a.labels[rec];
    const int n = a.onehot_rows * a.num_classes;
    for (int q = (int)threadIdx.x; q < n; q += kDrawThreads) {
      const int row = q / a.num_classes, c = q - row * a.num_classes;
      const int64_t o = ((int64_t)b * a.onehot_rows + row) * a.onehot_ld + a.onehot_col0 + c;
      const float v = (c == lab) ? 1.0f : 0.0f;
      if (a.onehot_dtype == SRWN_BF16) reinterpret_cast<bf16_t*>(a.onehot)[o] = (bf16_t)v;
      else reinterpret_cast<float*>(a.onehot)[o] = v;
    }
  }
}

__global__ void step_log_kernel(const float* __restrict__ loss, float* __restrict__ log, int32_t capacity,
                                int64_t* __restrict__ state) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const unsigned long long step = (unsigned long long)state[1];
  log[step % (unsigned long long)capacity] = loss[0];
  state[1] = (int64_t)(step + 1ull);
}

}  // namespace

extern "C" int srwn_batch_draw(const float* clips, const int32_t* labels, int32_t num_clips, int64_t clip_len,
                               const int64_t* state, int32_t B, int32_t T, int32_t shuffle, int32_t crop, int32_t rank,
                               int32_t world, float* audio0, float* audio1, int32_t* codes, int32_t quantization_channels,
                               void* onehot, int64_t onehot_ld, int32_t onehot_rows, int32_t onehot_col0,
                               int32_t num_classes, int32_t onehot_dtype, int32_t* indices, void* stream) {
  if (B == 0 || T == 0) return 0;
  if (num_clips < 1 || clip_len < 1 || B < 0 || T < 0 || (int64_t)T > clip_len || clip_len - T >= (1ll << 32))
    return set_error(SRWN_E_SHAPE, "batch_draw: %d clips of %lld samples, B=%d T=%d", num_clips, (long long)clip_len, B, T);
  if (B > 65535) return set_error(SRWN_E_SHAPE, "batch_draw: B=%d (at most 65535 rows per draw)", B);
  if (world < 1 || rank < 0 || rank >= world) return set_error(SRWN_E_SHAPE, "batch_draw: rank %d of %d", rank, world);
  if (crop != 0 && crop != 1) return set_error(SRWN_E_SHAPE, "batch_draw: crop %d (0 head, 1 random)", crop);
  if (!clips || !state || !audio0 || !indices) return set_error(SRWN_E_NULL, "batch_draw: null pointer");
  if (codes && quantization_channels < 2) return set_error(SRWN_E_SHAPE, "batch_draw: Q=%d", quantization_channels);
  if (onehot) {
    if (!labels) return set_error(SRWN_E_NULL, "batch_draw: one-hot rows need the labels");
    if (onehot_dtype != SRWN_F32 && onehot_dtype != SRWN_BF16) return set_error(SRWN_E_DTYPE, "batch_draw: one-hot dtype %d", onehot_dtype);
    if (num_classes < 1 || onehot_rows < 1 || onehot_col0 < 0 || onehot_ld < (int64_t)onehot_col0 + num_classes ||
        (int64_t)onehot_rows * num_classes > (1ll << 30))
      return set_error(SRWN_E_SHAPE, "batch_draw: one-hot %d rows x %d classes at column %d, ld %lld", onehot_rows,
                       num_classes, onehot_col0, (long long)onehot_ld);
  }
  if (((uintptr_t)clips | (uintptr_t)audio0 | (uintptr_t)audio1 | (uintptr_t)codes) & 3)
    return set_error(SRWN_E_SHAPE, "batch_draw: the fp32 / int32 buffers must be 4-byte aligned");
  DrawArgs a;
  a.clips = clips; a.labels = labels; a.state = state;
  a.audio0 = audio0; a.audio1 = audio1; a.codes = codes; a.onehot = onehot; a.indices = indices;
  a.clip_len = clip_len; a.onehot_ld = onehot_ld;
  a.N = num_clips; a.B = B; a.T = T; a.shuffle = shuffle != 0; a.crop = crop; a.rank = rank; a.world = world;
  a.Q = quantization_channels; a.onehot_rows = onehot_rows; a.onehot_col0 = onehot_col0; a.num_classes = num_classes;
  a.onehot_dtype = onehot_dtype;
  a.mu = codes ? (float)(quantization_channels - 1) : 0.0f;                // (srwn_mu_law_encode's constants)
  a.log1p_mu = codes ? (float)log1p((double)a.mu) : 0.0f;
  dim3 grid((unsigned)((T + kDrawSpan - 1) / kDrawSpan), (unsigned)B);
  hipLaunchKernelGGL(batch_draw_kernel, grid, dim3(kDrawThreads), 0, (hipStream_t)stream, a);
  return check_launch("batch_draw");
}

extern "C" int srwn_step_log(const float* loss, float* log, int32_t capacity, int64_t* state, void* stream) {
  if (!loss || !log || !state) return set_error(SRWN_E_NULL, "step_log: null pointer");
  if (capacity < 1) return set_error(SRWN_E_SHAPE, "step_log: capacity %d", capacity);
  hipLaunchKernelGGL(step_log_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, loss, log, capacity, state);
  return check_launch("step_log");
}
