// Device-resident evaluation (srwn.h, srwn_version() 124): the launch that sits behind the classifier's forward pass when an
// EvalSampler (sr-wavenet_amd/dataset.py) sweeps a held-out set.
//
//   srwn_eval_classes   reads {seed, step, sweep} from device memory and, for every row of the step whose position
//                       p = (step * world + rank) * B + b lies inside the set, writes the predicted class, the rank of the
//                       label's class and the row's negative log-likelihood at the row's record of result slot
//                       sweep % sweep_capacity, and counts the row in the slot's confusion matrix.  Rows past the end of
//                       the set (the ragged tail of a sweep's last step) write nothing.  Then it ticks the state: the draw
//                       in front (srwn_batch_draw) only reads it.
//
// One workgroup of 256 threads: a wave per row, four classes per lane (C <= 256).  Everything that is counted is counted
// with integer atomic adds, so the results do not depend on the order in which the waves reach their rows.
#include "srwn_common.h"
#include "srwn_host.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

constexpr int kEvalThreads = 256;
constexpr int kEvalWave = 64;
constexpr int kEvalPerLane = 4;                                   // 64 lanes x 4 classes = the 256 classes of a row

struct EvalArgs {
  const float* probs; const int32_t* indices; const int32_t* labels; int64_t* state;
  int32_t* pred; int32_t* rank_out; float* nll; int32_t* confusion; int32_t* seen;
  int32_t N, B, C, rank, world, capacity;
};

// (v, i) before (w, j) in the order of the generators' argmax: the greater value, on equal values the lower index
__device__ __forceinline__ bool eval_beats(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

__global__ __launch_bounds__(kEvalThreads) void eval_classes_kernel(const EvalArgs a) {
  const int tid = (int)threadIdx.x, lane = tid & (kEvalWave - 1), wave = tid / kEvalWave;
  // every thread reads the state here; thread 0 writes it behind the last barrier
  const unsigned long long step = (unsigned long long)a.state[1], sweep = (unsigned long long)a.state[2];
  const int64_t slot = (int64_t)(sweep % (unsigned long long)a.capacity);
  const int C = a.C;
  int32_t* const conf = a.confusion + slot * C * C;
  int32_t* const seen = a.seen + slot;
  if (step == 0ull) {                                             // a sweep's first step clears what the slot counted before
    for (int q = tid; q < C * C; q += kEvalThreads) conf[q] = 0;
    if (tid == 0) *seen = 0;
    __threadfence();                                              // the zeros are in memory before any wave adds to them
  }
  __syncthreads();
  const unsigned long long p0 = (step * (unsigned long long)a.world + (unsigned long long)a.rank) * (unsigned long long)a.B;
  for (int b = wave; b < a.B; b += kEvalThreads / kEvalWave) {    // (wave-uniform: b, p, rec and lab are)
    if (p0 + (unsigned long long)b >= (unsigned long long)a.N) break;      // the ragged tail: later rows lie further out
    const int32_t rec = a.indices[b];
    if ((uint32_t)rec >= (uint32_t)a.N) continue;                 // (the draw's records are p % N: never taken)
    const int32_t lab = a.labels[rec];
    if ((uint32_t)lab >= (uint32_t)C) continue;                   // (the sampler refuses such a set: never taken)
    const float* row = a.probs + (int64_t)b * C;
    const float pl = row[lab];
    float bv = 0.0f;
    int bi = 0x7fffffff, above = 0;
#pragma unroll
    for (int k = 0; k < kEvalPerLane; ++k) {
      const int c = lane * kEvalPerLane + k;
      if (c < C) {
        const float v = row[c];
        if (bi == 0x7fffffff || eval_beats(v, c, bv, bi)) { bv = v; bi = c; }
        above += eval_beats(v, c, pl, lab) ? 1 : 0;
      }
    }
#pragma unroll
    for (int m = kEvalWave / 2; m >= 1; m >>= 1) {
      const float ov = __shfl_xor(bv, m, kEvalWave);
      const int oi = __shfl_xor(bi, m, kEvalWave);
      above += __shfl_xor(above, m, kEvalWave);
      if (oi != 0x7fffffff && (bi == 0x7fffffff || eval_beats(ov, oi, bv, bi))) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
      const int pr = min(max(bi, 0), C - 1);                      // (class 0 always exists: inside [0, C) already)
      const int64_t o = slot * (int64_t)a.N + rec;
      a.pred[o] = pr;
      a.rank_out[o] = above;
      a.nll[o] = (float)(-log((double)pl));
      atomicAdd(conf + (int64_t)lab * C + pr, 1);
      atomicAdd(seen, 1);
    }
  }
  __syncthreads();
  if (tid == 0) {                                                 // the tick: the last step of a sweep starts the next one
    const unsigned long long per = (unsigned long long)a.B * (unsigned long long)a.world;
    const unsigned long long steps = ((unsigned long long)a.N + per - 1ull) / per;
    if (step + 1ull >= steps) { a.state[1] = 0; a.state[2] = (int64_t)(sweep + 1ull); }
    else a.state[1] = (int64_t)(step + 1ull);
  }
}

}  // namespace

extern "C" int srwn_eval_classes(const float* probs, const int32_t* indices, const int32_t* labels, int64_t* state,
                                 int32_t num_clips, int32_t B, int32_t C, int32_t rank, int32_t world,
                                 int32_t sweep_capacity, int32_t* pred, int32_t* rank_out, float* nll, int32_t* confusion,
                                 int32_t* seen, void* stream) {
  if (!probs || !indices || !labels || !state || !pred || !rank_out || !nll || !confusion || !seen)
    return set_error(SRWN_E_NULL, "eval_classes: null pointer");
  if (C < 1 || C > kEvalWave * kEvalPerLane) return set_error(SRWN_E_SHAPE, "eval_classes: C=%d (1 to 256 classes)", C);
  if (B < 1 || num_clips < 1) return set_error(SRWN_E_SHAPE, "eval_classes: %d clips, B=%d", num_clips, B);
  if (world < 1 || rank < 0 || rank >= world) return set_error(SRWN_E_SHAPE, "eval_classes: rank %d of %d", rank, world);
  if (sweep_capacity < 1) return set_error(SRWN_E_SHAPE, "eval_classes: sweep_capacity %d", sweep_capacity);
  EvalArgs a;
  a.probs = probs; a.indices = indices; a.labels = labels; a.state = state;
  a.pred = pred; a.rank_out = rank_out; a.nll = nll; a.confusion = confusion; a.seen = seen;
  a.N = num_clips; a.B = B; a.C = C; a.rank = rank; a.world = world; a.capacity = sweep_capacity;
  hipLaunchKernelGGL(eval_classes_kernel, dim3(1), dim3(kEvalThreads), 0, (hipStream_t)stream, a);
  return check_launch("eval_classes");
}
