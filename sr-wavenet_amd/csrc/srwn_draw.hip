// Device-resident training for the student and the twin towers (srwn.h, srwn_version() 123): the launches a DistillSampler
// and a PairSampler (sr-wavenet_amd/dataset.py) put around a training step, inside its hipGraph.
//
//   srwn_distill_draw   the student step's first launch: the draw of srwn_batch_draw (csrc/srwn_data.hip; the same order
//                       function, dataset.draw_plan) into up to three fp32 buffers, the step's logistic noise
//                       (dataset.noise_plan: the bits srwn_logistic_noise draws for the rows' seeds at clock 0) and the
//                       labels' one-hot rows into every conditioning input of the step.
//   srwn_cond_scatter   after the teacher encoder's forward pass: its fp32 encoding into the latent columns of the same
//                       conditioning inputs, in their dtype.
//   srwn_distill_log    the student step's last launch: the loss from the three device scalars in double, by
//                       StudentEngine.losses()'s operations, into three rings; then step += 1.
//   srwn_pair_draw      the twins' first launch: dataset.pair_plan -- the left clips as srwn_batch_draw picks them, for each a
//                       right clip of the same class or of another one -- into the two halves of the engine's batch.
//   srwn_pair_log       the twins' last launch: the loss and the P distances into two rings; then step += 1.
//
// The ticks live in the log launches: every workgroup of a draw reads `step`, and no workgroup of a launch may change what
// the others read.  Rows are written as srwn_batch_draw writes them: a scalar head up to the destination's 16-byte
// boundary, 16-byte stores and a scalar tail, a row longer than kDrawSpan split over several workgroups.
#include "srwn_common.h"
#include "srwn_draw_common.h"
#include "srwn_host.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

constexpr unsigned long long kNoiseSalt = 0x6E6F697365726F77ull;      // dataset.NOISE_SALT

// log u - log(1 - u) at u = (k + 1/2) / 2^23: the evaluation of csrc/srwn_stream.hip's logistic_of_bits23, operation for
// operation (srwn_logistic_noise and srwn_logistic_from_bits give these bits)
__device__ __forceinline__ float logistic_of_bits23(uint32_t k) {
  const float u = ((float)(k & 0x7fffffu) + 0.5f) * (1.0f / 8388608.0f);
  const float v = 1.0f - u;
  const float d = u - v;                                   // 2u - 1, exact
  const float l = log1pf(fabsf(d) / fminf(u, v));
  return d < 0.0f ? -l : l;
}

// one row of T fp32 values dst[j] = src[j], this workgroup's share [j0, j1): the row writer of srwn_draw_common.h
__device__ __forceinline__ void copy_row(float* __restrict__ dst, const float* __restrict__ src, int j0, int j1) {
  draw_row(dst, src, j0, j1, [](float x) { return x; });
}

__device__ __forceinline__ void put(void* table, int dtype, int64_t o, float v) {
  if (dtype == SRWN_BF16) reinterpret_cast<bf16_t*>(table)[o] = (bf16_t)v;      // round to nearest even
  else reinterpret_cast<float*>(table)[o] = v;
}

struct DistillArgs {
  const float* clips; const int32_t* labels; const int64_t* state;
  float* audio0; float* audio1; float* audio2; float* noise; const int64_t* tables; int32_t* indices;
  int64_t clip_len, cond_ld;
  int32_t N, B, T, shuffle, crop, rank, world, num_tables, cond_rows, cond_col0, num_classes, cond_dtype;
  float temperature;
};

__global__ __launch_bounds__(kDrawThreads) void distill_draw_kernel(const DistillArgs a) {
  const int b = (int)blockIdx.y;
  const unsigned long long seed = (unsigned long long)a.state[0], step = (unsigned long long)a.state[1];
  const unsigned long long p = (step * (unsigned long long)a.world + (unsigned long long)a.rank) * (unsigned long long)a.B + (unsigned long long)b;
  const Pick k = draw_pick(seed, p, a.N, a.shuffle, a.crop, a.clip_len, a.T);
  const float* src = a.clips + (int64_t)k.rec * a.clip_len + k.off;
  const int j0 = (int)blockIdx.x * kDrawSpan;
  const int j1 = min(a.T, j0 + kDrawSpan);
  copy_row(a.audio0 + (int64_t)b * a.T, src, j0, j1);
  if (a.audio1) copy_row(a.audio1 + (int64_t)b * a.T, src, j0, j1);
  if (a.audio2) copy_row(a.audio2 + (int64_t)b * a.T, src, j0, j1);
  if (a.noise) {                                                  // dataset.noise_plan: row seed s_b, counter j
    const unsigned long long sb = mix64((seed ^ kNoiseSalt) + kGolden * (p + 1ull));
    const float tmp = a.temperature;
    float* nz = a.noise + (int64_t)b * a.T;
    for (int j = j0 + (int)threadIdx.x; j < j1; j += kDrawThreads) {
      const uint32_t bits = (uint32_t)(mix64(sb + kGolden * ((unsigned long long)j + 1ull)) >> 41);
      const float l = logistic_of_bits23(bits);
      nz[j] = tmp == 0.0f ? 0.0f : tmp * l;                       // (srwn_logistic_noise's rule)
    }
  }
  if (blockIdx.x != 0) return;
  if (threadIdx.x == 0) a.indices[b] = (int32_t)k.rec;
  if (a.num_tables > 0) {                                         // tf.one_hot: a label outside [0, num_classes) gives zeros
    const int32_t lab = a.labels[k.rec];
    const int per = a.cond_rows * a.num_classes;
    const int n = a.num_tables * per;
    for (int q = (int)threadIdx.x; q < n; q += kDrawThreads) {
      const int t = q / per, r = q - t * per;
      const int row = r / a.num_classes, c = r - row * a.num_classes;
      const int64_t o = ((int64_t)b * a.cond_rows + row) * a.cond_ld + a.cond_col0 + c;
      put(reinterpret_cast<void*>(a.tables[t]), a.cond_dtype, o, (c == lab) ? 1.0f : 0.0f);
    }
  }
}

__global__ __launch_bounds__(256) void cond_scatter_kernel(const float* __restrict__ enc, int64_t rows, int32_t latent,
                                                           const int64_t* __restrict__ tables, int32_t num_tables,
                                                           int64_t ld, int32_t dtype) {
  const int64_t per = rows * latent;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= per * num_tables) return;
  const int t = (int)(i / per);
  const int64_t r = i - (int64_t)t * per;
  const int64_t row = r / latent;
  const int c = (int)(r - row * latent);
  put(reinterpret_cast<void*>(tables[t]), dtype, row * ld + c, enc[r]);
}

// StudentEngine.losses() in its own order, every operation rounded once (no contraction into a multiply-add):
// entropy = logs + 2 N;  loss = (beta ce - alpha entropy + power) / loss_div
__global__ void distill_log_kernel(const float* __restrict__ ce, const float* __restrict__ power,
                                   const float* __restrict__ logs, double alpha, double beta, double two_n, double loss_div,
                                   float* __restrict__ loss_log, float* __restrict__ power_log, float* __restrict__ entropy_log,
                                   int32_t capacity, int64_t* __restrict__ state) {
#pragma clang fp contract(off)
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const unsigned long long step = (unsigned long long)state[1];
  const unsigned long long slot = step % (unsigned long long)capacity;
  const double entropy = __dadd_rn((double)logs[0], two_n);
  const double num = __dadd_rn(__dadd_rn(__dmul_rn(beta, (double)ce[0]), -__dmul_rn(alpha, entropy)), (double)power[0]);
  loss_log[slot] = (float)__ddiv_rn(num, loss_div);
  power_log[slot] = power[0];
  entropy_log[slot] = (float)entropy;
  state[1] = (int64_t)(step + 1ull);
}

__global__ __launch_bounds__(kDrawThreads) void pair_draw_kernel(const PairArgs a) {
  const int row = (int)blockIdx.y;                                // [0, P): the left clips; [P, 2P): the right ones
  const int b = row < a.P ? row : row - a.P;
  const unsigned long long seed = (unsigned long long)a.state[0], step = (unsigned long long)a.state[1];
  const unsigned long long p = (step * (unsigned long long)a.world + (unsigned long long)a.rank) * (unsigned long long)a.P + (unsigned long long)b;
  const Pick k = draw_pick(seed, p, a.N, a.shuffle, a.crop, a.clip_len, a.T);
  // dataset.pair_plan: the class block of the left record in `order`, the coin, the right record
  const int32_t c = a.labels[k.rec];
  const bool known = (unsigned)c < (unsigned)a.num_classes;       // (a PairSampler refuses labels outside the classes)
  const unsigned long long s0 = known ? (unsigned long long)a.start[c] : 0ull;
  const unsigned long long m = known ? (unsigned long long)a.start[c + 1] - s0 : 1ull;
  const unsigned long long q = known ? (unsigned long long)a.place[k.rec] - s0 : 0ull;
  const unsigned long long N = known ? (unsigned long long)a.N : 1ull;   // ... such a record is paired with itself
  const unsigned long long h1 = mix64((seed ^ kPairSalt) + kGolden * (p + 1ull));
  const unsigned long long h2 = mix64((seed ^ kPairPickSalt) + kGolden * (p + 1ull)) >> 32;
  bool same = (h1 >> 32) < a.threshold;
  if (m == 1ull) same = false;                                    // a singleton has no partner in its class
  if (N == m) same = true;                                        // one class only
  unsigned rrec;
  if (N == 1ull) {
    rrec = k.rec;                                                 // the only record, paired with itself
  } else if (same) {
    unsigned long long kk = (h2 * (m - 1ull)) >> 32;
    kk += (kk >= q) ? 1ull : 0ull;                                // never the left clip itself
    rrec = (unsigned)a.order[s0 + kk];
  } else {
    const unsigned long long kk = (h2 * (N - m)) >> 32;
    rrec = (unsigned)a.order[kk < s0 ? kk : kk + m];
  }
  int64_t roff = 0;
  if (a.crop) {
    const unsigned long long h3 = mix64((seed ^ kPairCropSalt) + kGolden * (p + 1ull));
    roff = (int64_t)(((h3 >> 32) * (unsigned long long)(a.clip_len - a.T + 1)) >> 32);
  }
  const float* src = row < a.P ? a.clips + (int64_t)k.rec * a.clip_len + k.off
                               : a.clips + (int64_t)rrec * a.clip_len + roff;
  const int j0 = (int)blockIdx.x * kDrawSpan;
  const int j1 = min(a.T, j0 + kDrawSpan);
  copy_row(a.audio + (int64_t)row * a.T, src, j0, j1);
  if (blockIdx.x == 0 && row < a.P && threadIdx.x == 0) {
    const float y = (a.labels[rrec] == c) ? 1.0f : 0.0f;          // model.py:747-749: 1 = "same"
    a.y[b] = y;
    a.y_log[b] = y;
    a.left[b] = (int32_t)k.rec;
    a.right[b] = (int32_t)rrec;
  }
}

__global__ __launch_bounds__(256) void pair_log_kernel(const float* __restrict__ loss, const float* __restrict__ dist,
                                                       int32_t P, float* __restrict__ loss_log, float* __restrict__ dist_log,
                                                       int32_t capacity, int64_t* __restrict__ state) {
  if (blockIdx.x != 0) return;
  const unsigned long long step = (unsigned long long)state[1];   // every thread reads it before the barrier
  __syncthreads();
  const unsigned long long slot = step % (unsigned long long)capacity;
  for (int i = (int)threadIdx.x; i < P; i += 256) dist_log[(int64_t)slot * P + i] = dist[i];
  if (threadIdx.x == 0) {
    loss_log[slot] = loss[0];
    state[1] = (int64_t)(step + 1ull);                            // ... and one writes it after
  }
}

}  // namespace

extern "C" int srwn_distill_draw(const float* clips, const int32_t* labels, int32_t num_clips, int64_t clip_len,
                                 const int64_t* state, int32_t B, int32_t T, int32_t shuffle, int32_t crop, int32_t rank,
                                 int32_t world, float* audio0, float* audio1, float* audio2, float* noise, float temperature,
                                 const int64_t* cond_tables, int32_t num_tables, int64_t cond_ld, int32_t cond_rows,
                                 int32_t cond_col0, int32_t num_classes, int32_t cond_dtype, int32_t* indices, void* stream) {
  if (B == 0 || T == 0) return 0;
  if (int rc = check_draw("distill_draw", clips, num_clips, clip_len, state, B, T, crop, rank, world)) return rc;
  if (B > 65535) return set_error(SRWN_E_SHAPE, "distill_draw: B=%d (at most 65535 rows per draw)", B);
  if (!audio0 || !indices) return set_error(SRWN_E_NULL, "distill_draw: null pointer");
  if (num_tables < 0 || num_tables > 64) return set_error(SRWN_E_SHAPE, "distill_draw: %d conditioning tables (0..64)", num_tables);
  if (num_tables) {
    if (!labels || !cond_tables) return set_error(SRWN_E_NULL, "distill_draw: one-hot rows need the labels and the tables");
    if (cond_dtype != SRWN_F32 && cond_dtype != SRWN_BF16) return set_error(SRWN_E_DTYPE, "distill_draw: one-hot dtype %d", cond_dtype);
    if (num_classes < 1 || cond_rows < 1 || cond_col0 < 0 || cond_ld < (int64_t)cond_col0 + num_classes ||
        (int64_t)cond_rows * num_classes > (1ll << 24))
      return set_error(SRWN_E_SHAPE, "distill_draw: one-hot %d rows x %d classes at column %d, ld %lld", cond_rows,
                       num_classes, cond_col0, (long long)cond_ld);
  }
  if (((uintptr_t)clips | (uintptr_t)audio0 | (uintptr_t)audio1 | (uintptr_t)audio2 | (uintptr_t)noise) & 3)
    return set_error(SRWN_E_SHAPE, "distill_draw: the fp32 buffers must be 4-byte aligned");
  DistillArgs a;
  a.clips = clips; a.labels = labels; a.state = state;
  a.audio0 = audio0; a.audio1 = audio1; a.audio2 = audio2; a.noise = noise; a.tables = cond_tables; a.indices = indices;
  a.clip_len = clip_len; a.cond_ld = cond_ld;
  a.N = num_clips; a.B = B; a.T = T; a.shuffle = shuffle != 0; a.crop = crop; a.rank = rank; a.world = world;
  a.num_tables = num_tables; a.cond_rows = cond_rows; a.cond_col0 = cond_col0; a.num_classes = num_classes;
  a.cond_dtype = cond_dtype; a.temperature = temperature;
  dim3 grid((unsigned)((T + kDrawSpan - 1) / kDrawSpan), (unsigned)B);
  hipLaunchKernelGGL(distill_draw_kernel, grid, dim3(kDrawThreads), 0, (hipStream_t)stream, a);
  return check_launch("distill_draw");
}

extern "C" int srwn_cond_scatter(const float* enc, int64_t rows, int32_t latent, const int64_t* cond_tables,
                                 int32_t num_tables, int64_t cond_ld, int32_t cond_dtype, void* stream) {
  if (rows == 0 || latent == 0 || num_tables == 0) return 0;
  if (rows < 0 || latent < 0 || cond_ld < latent || num_tables < 0 || num_tables > 64 ||
      rows * (int64_t)latent > (1ll << 31))
    return set_error(SRWN_E_SHAPE, "cond_scatter: %lld rows x %d columns into %d tables of ld %lld", (long long)rows, latent,
                     num_tables, (long long)cond_ld);
  if (cond_dtype != SRWN_F32 && cond_dtype != SRWN_BF16) return set_error(SRWN_E_DTYPE, "cond_scatter: dtype %d", cond_dtype);
  if (!enc || !cond_tables) return set_error(SRWN_E_NULL, "cond_scatter: null pointer");
  const int64_t n = rows * latent * num_tables;
  hipLaunchKernelGGL(cond_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, enc, rows,
                     latent, cond_tables, num_tables, cond_ld, cond_dtype);
  return check_launch("cond_scatter");
}

extern "C" int srwn_distill_log(const float* ce, const float* power, const float* logs, double alpha, double beta,
                                int64_t n, double loss_div, float* loss_log, float* power_log, float* entropy_log,
                                int32_t capacity, int64_t* state, void* stream) {
  if (!ce || !power || !logs || !loss_log || !power_log || !entropy_log || !state)
    return set_error(SRWN_E_NULL, "distill_log: null pointer");
  if (capacity < 1 || n < 0 || n > (1ll << 52)) return set_error(SRWN_E_SHAPE, "distill_log: capacity %d, n %lld", capacity, (long long)n);
  if (!(loss_div != 0.0)) return set_error(SRWN_E_SHAPE, "distill_log: loss_div %g", loss_div);
  hipLaunchKernelGGL(distill_log_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, ce, power, logs, alpha, beta,
                     2.0 * (double)n, loss_div, loss_log, power_log, entropy_log, capacity, state);
  return check_launch("distill_log");
}

extern "C" int srwn_pair_draw(const float* clips, const int32_t* labels, const int32_t* order, const int32_t* place,
                              const int32_t* class_start, int32_t num_classes, int32_t num_clips, int64_t clip_len, const int64_t* state,
                              int32_t P,
                              int32_t T, int64_t same_threshold, int32_t shuffle, int32_t crop, int32_t rank, int32_t world,
                              float* audio, float* y, int32_t* left, int32_t* right, float* y_log, void* stream) {
  if (P == 0 || T == 0) return 0;
  PairArgs a;
  if (int rc = check_pair_draw("pair_draw", clips, labels, order, place, class_start, num_classes, num_clips, clip_len, state, P,
                               T, same_threshold, shuffle, crop, rank, world, audio, y, left, right, y_log, &a))
    return rc;
  dim3 grid((unsigned)((T + kDrawSpan - 1) / kDrawSpan), (unsigned)(2 * P));
  hipLaunchKernelGGL(pair_draw_kernel, grid, dim3(kDrawThreads), 0, (hipStream_t)stream, a);
  return check_launch("pair_draw");
}

extern "C" int srwn_pair_log(const float* loss, const float* dist, int32_t P, float* loss_log, float* dist_log,
                             int32_t capacity, int64_t* state, void* stream) {
  if (!loss || !dist || !loss_log || !dist_log || !state) return set_error(SRWN_E_NULL, "pair_log: null pointer");
  if (capacity < 1 || P < 1) return set_error(SRWN_E_SHAPE, "pair_log: capacity %d, P %d", capacity, P);
  hipLaunchKernelGGL(pair_log_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, loss, dist, P, loss_log, dist_log,
                     capacity, state);
  return check_launch("pair_log");
}
