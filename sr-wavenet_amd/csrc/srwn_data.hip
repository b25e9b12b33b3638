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
#include "srwn_draw_common.h"
#include "srwn_host.h"
#include "srwn_mulaw.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

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
  if (a.onehot)
    draw_onehot(a.onehot, a.onehot_dtype, a.labels[rec], b, a.onehot_rows, a.num_classes, a.onehot_ld, a.onehot_col0);
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
  DrawArgs a;
  if (int rc = check_batch_draw("batch_draw", clips, labels, num_clips, clip_len, state, B, T, shuffle, crop, rank, world, audio0,
                                audio1, codes, quantization_channels, onehot, onehot_ld, onehot_rows, onehot_col0, num_classes,
                                onehot_dtype, indices, &a))
    return rc;
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
