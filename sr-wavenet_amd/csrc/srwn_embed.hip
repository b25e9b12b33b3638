// Streaming embedder: the last launch of a tower of class SiameseWaveNet (model.py:660-797) run as a stream.  A tower is
// class WaveNet's network up to the last 1x1, so everything below is the streaming classifier's (srwn_recog.hip): the
// stream entry, the stack with stored z and the hop sums of r1 in the per-stream ring.  Here is what turns a window of the
// ring into an embedding and scores it against an enrolled gallery, one launch, one workgroup per (stream, hop):
//   window mean   the mean over the nW = window / hop ring rows that end at the hop, oldest first, then / window -- the
//                 statements of window_mean_kernel (srwn_recog.hip), so that the bits are srwn_window_mean's
//   embedding     emb[d] = b2[d] + sum_s mean[s] w2[s][d], one fmaf per s in order: the statements of window_mean_kernel's
//                 `logits`, so that the bits are its logits'
//   distances     dist[n] = sqrt(1e-8 + sum_d (emb[d] - g[n][d])^2) for the N = *n_gallery enrolled rows (model.py:736 as
//                 srwn_contrastive_head computes it: lanes stride over d, one fmaf each, a 64-lane xor butterfly)
//   nearest       the argmin over n < N with its distance, the lowest index on ties; -1 and +inf for N = 0
// The two routines are restated here rather than moved into a header: srwn_recog.hip stays byte for byte what it was, and
// the GPU tests hold the two files to each other bit for bit.  N is read from device memory by every workgroup, so a
// captured graph keeps serving after the gallery has changed.  The mean and the embedding live in LDS; no scratch, no
// atomics.  srwn_gallery_match is the last two steps alone (the same device body) on embeddings that are already there:
// the last step of the parity twin, and a scorer of stored embeddings.
#include <cmath>
#include "srwn_common.h"
#include "srwn_host.h"
#include "srwn_slots.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

constexpr int kEmThreads = 256;      // four wave64s
constexpr int kEmWaves = kEmThreads / 64;
constexpr int kEmMaxS = 256, kEmMaxD = 256, kEmMaxGallery = 1024;

__device__ __forceinline__ float wave_sum64(float v) {      // butterfly over all 64 lanes: every lane ends with the sum
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Distances of the embedding e [D] (LDS, complete: the caller has put a barrier behind its last write) to the first
// N = clamp(*n_gallery, 0, max_gallery) rows of gallery [max_gallery][D], and the nearest row.  Wave w takes the rows w,
// w + 4, ...: lane l adds the squares of d = l, l + 64, ... in order, the butterfly adds the lanes.  A row's bits depend on
// e, g[n] and D alone -- not on N, on which wave took it or on the row of the grid.  Each wave keeps the first minimum of
// its ascending rows (strict <), thread 0 merges the four in wave order preferring the lower index on equal distances.
__device__ __forceinline__ void match_body(const float* e, int D, const float* __restrict__ gallery,
                                           const int* __restrict__ n_gallery, int max_gallery, float* __restrict__ dist,
                                           int* __restrict__ nearest, float* __restrict__ dmin, float* wd, int* wi) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  int N = *n_gallery;
  N = N < 0 ? 0 : (N > max_gallery ? max_gallery : N);
  float best = INFINITY;
  int bi = -1;
  for (int n = wave; n < N; n += kEmWaves) {
    const float* g = gallery + (int64_t)n * D;
    float ss = 0.0f;
    for (int d = lane; d < D; d += 64) {
      const float df = e[d] - g[d];
      ss = fmaf(df, df, ss);
    }
    ss = wave_sum64(ss);
    const float dn = sqrtf(1e-8f + ss);
    if (lane == 0) dist[n] = dn;
    if (bi < 0 || dn < best) {
      best = dn;
      bi = n;
    }
  }
  if (lane == 0) {
    wd[wave] = best;
    wi[wave] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    best = wd[0];
    bi = wi[0];
    for (int w = 1; w < kEmWaves; ++w)
      if (wi[w] >= 0 && (bi < 0 || wd[w] < best || (wd[w] == best && wi[w] < bi))) {
        best = wd[w];
        bi = wi[w];
      }
    *nearest = bi;
    *dmin = bi < 0 ? INFINITY : best;
  }
}

// One workgroup per row = (stream b, hop i of the step).  SLOTS: `clock` is the pool's table, j from the slot's own time,
// and the row's mean is zero too where the hop lies beyond ran(u) (an idle slot's rows); such rows read no ring row.
template <bool SLOTS>
__global__ __launch_bounds__(kEmThreads) void window_embed_match_kernel(
    const float* __restrict__ ring, int ring_rows, typename ClockArg<SLOTS>::in clock, int k, int hop, int nW, float window,
    int S, const float* __restrict__ w2, const float* __restrict__ b2, int D, int ldw, const float* __restrict__ gallery,
    const int* __restrict__ n_gallery, int max_gallery, float* __restrict__ emb, float* __restrict__ dist,
    int* __restrict__ nearest, float* __restrict__ dmin) {
  __shared__ float m[kEmMaxS];
  __shared__ float e[kEmMaxD];
  __shared__ float wd[kEmWaves];
  __shared__ int wi[kEmWaves];
  const int b = (int)blockIdx.x / k, i = (int)blockIdx.x % k;
  long long j_;
  bool due = true;
  if constexpr (SLOTS) {
    const SrwnSynthSlot sl = clock[b];
    due = sl.t >= 0 && (i + 1) * hop <= slot_rows(sl, k * hop);
    j_ = due ? sl.t / hop + i : 0;
  } else j_ = *clock / hop + i;
  const long long j = j_;
  const float* rb = ring + (int64_t)b * ring_rows * S;
  for (int s = threadIdx.x; s < S; s += kEmThreads) {
    float acc = 0.0f;
    if (due && j >= nW - 1)
      for (int w = 0; w < nW; ++w) acc += rb[(int64_t)((j - nW + 1 + w) % ring_rows) * S + s];
    acc = acc / window;
    m[s] = acc;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += kEmThreads) {
    float acc = b2[c];
    for (int s = 0; s < S; ++s) acc = fmaf(m[s], w2[(int64_t)s * ldw + c], acc);
    e[c] = acc;
    emb[(int64_t)blockIdx.x * D + c] = acc;
  }
  __syncthreads();
  match_body(e, D, gallery, n_gallery, max_gallery, dist + (int64_t)blockIdx.x * max_gallery, nearest + blockIdx.x,
             dmin + blockIdx.x, wd, wi);
}

__global__ __launch_bounds__(kEmThreads) void gallery_match_kernel(const float* __restrict__ emb, int D,
                                                                   const float* __restrict__ gallery,
                                                                   const int* __restrict__ n_gallery, int max_gallery,
                                                                   float* __restrict__ dist, int* __restrict__ nearest,
                                                                   float* __restrict__ dmin) {
  __shared__ float e[kEmMaxD];
  __shared__ float wd[kEmWaves];
  __shared__ int wi[kEmWaves];
  for (int c = threadIdx.x; c < D; c += kEmThreads) e[c] = emb[(int64_t)blockIdx.x * D + c];
  __syncthreads();
  match_body(e, D, gallery, n_gallery, max_gallery, dist + (int64_t)blockIdx.x * max_gallery, nearest + blockIdx.x,
             dmin + blockIdx.x, wd, wi);
}

// what both entry points ask of an embedding and a gallery
int match_args(const char* who, int32_t D, int32_t max_gallery) {
  if (D < 1 || D > kEmMaxD || max_gallery < 1 || max_gallery > kEmMaxGallery)
    return set_error(SRWN_E_SHAPE, "%s: D=%d max_gallery=%d (1 <= D <= %d, 1 <= max_gallery <= %d)", who, D, max_gallery,
                     kEmMaxD, kEmMaxGallery);
  return 0;
}

template <bool SLOTS>
int window_embed_match_impl(const char* who, const float* ring, int32_t ring_rows, typename ClockArg<SLOTS>::in clock,
                            int32_t B, int32_t k, int32_t hop, int32_t window, int32_t S, const float* w2, const float* b2,
                            int32_t D, int32_t ldw, const float* gallery, const int32_t* n_gallery, int32_t max_gallery,
                            float* emb, float* dist, int32_t* nearest, float* dmin, void* stream) {
  if (!ring || !clock || !w2 || !b2 || !gallery || !n_gallery || !emb || !dist || !nearest || !dmin)
    return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if (const int rc = match_args(who, D, max_gallery)) return rc;
  if (B < 1 || k < 1 || hop < 1 || window < hop || window % hop || S < 1 || S > kEmMaxS || ldw < D)
    return set_error(SRWN_E_SHAPE, "%s: %s=%d hops=%d hop=%d window=%d S=%d D=%d ldw=%d (window a multiple of hop, S <= 256, "
                     "ldw >= D)", who, SLOTS ? "capacity" : "B", B, k, hop, window, S, D, ldw);
  const int nW = window / hop;
  if (ring_rows < nW + k - 1)
    return set_error(SRWN_E_SHAPE, "%s: a ring of %d rows for %d window rows + %d hops per launch - 1", who, ring_rows, nW, k);
  // (SLOTS: the kernel counts a slot's rows in a chunk of k * hop in int32)
  if ((int64_t)B * k > 0x7fffffffLL || (SLOTS && (int64_t)k * hop > 0x7fffffffLL))
    return set_error(SRWN_E_SHAPE, "%s: too many rows", who);
  hipLaunchKernelGGL(window_embed_match_kernel<SLOTS>, dim3((unsigned)(B * k)), dim3(kEmThreads), 0, (hipStream_t)stream, ring,
                     ring_rows, clock, k, hop, nW, (float)window, S, w2, b2, D, ldw, gallery, n_gallery, max_gallery, emb, dist,
                     nearest, dmin);
  return check_launch(who);
}

}  // namespace

extern "C" int srwn_window_embed_match(const float* ring, int32_t ring_rows, const int64_t* clock, int32_t B, int32_t k,
                                       int32_t hop, int32_t window, int32_t S, const float* w2, const float* b2, int32_t D,
                                       int32_t ldw, const float* gallery, const int32_t* n_gallery, int32_t max_gallery,
                                       float* emb, float* dist, int32_t* nearest, float* dmin, void* stream) {
  return window_embed_match_impl<false>("window_embed_match", ring, ring_rows, reinterpret_cast<const long long*>(clock), B, k,
                                        hop, window, S, w2, b2, D, ldw, gallery, n_gallery, max_gallery, emb, dist, nearest,
                                        dmin, stream);
}

extern "C" int srwn_window_embed_match_slots(const float* ring, int32_t ring_rows, const SrwnSynthSlot* slots,
                                             int32_t capacity, int32_t k, int32_t hop, int32_t window, int32_t S,
                                             const float* w2, const float* b2, int32_t D, int32_t ldw, const float* gallery,
                                             const int32_t* n_gallery, int32_t max_gallery, float* emb, float* dist,
                                             int32_t* nearest, float* dmin, void* stream) {
  return window_embed_match_impl<true>("window_embed_match_slots", ring, ring_rows, slots, capacity, k, hop, window, S, w2, b2,
                                       D, ldw, gallery, n_gallery, max_gallery, emb, dist, nearest, dmin, stream);
}

extern "C" int srwn_gallery_match(const float* emb, int32_t rows, int32_t D, const float* gallery, const int32_t* n_gallery,
                                  int32_t max_gallery, float* dist, int32_t* nearest, float* dmin, void* stream) {
  if (rows == 0) return 0;
  if (!emb || !gallery || !n_gallery || !dist || !nearest || !dmin) return set_error(SRWN_E_NULL, "gallery_match: null pointer");
  if (const int rc = match_args("gallery_match", D, max_gallery)) return rc;
  if (rows < 0) return set_error(SRWN_E_SHAPE, "gallery_match: rows=%d", rows);
  hipLaunchKernelGGL(gallery_match_kernel, dim3((unsigned)rows), dim3(kEmThreads), 0, (hipStream_t)stream, emb, D, gallery,
                     n_gallery, max_gallery, dist, nearest, dmin);
  return check_launch("gallery_match");
}
