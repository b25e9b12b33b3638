// Augmented draws (srwn.h, srwn_version() 127): the draws of csrc/srwn_data.hip and csrc/srwn_draw.hip with a random time
// shift, a random gain and a background recording mixed in at a random volume, made in the draw launch itself.
//
//   srwn_batch_draw_aug   srwn_batch_draw's launch: the same records and crop offsets (dataset.draw_plan), every row changed
//                         by dataset.augment_plan / dataset.augment_rows on its way into the audio buffers and the codes.
//   srwn_pair_draw_aug    srwn_pair_draw's launch (dataset.pair_plan), the left clips augmented under side 0 and the right
//                         ones under side 1: two views of one record differ.
//
// A row's six draws are mix64((seed ^ salt) + GOLDEN * (2 p + side + 1)) with a salt per quantity.  The sample rule is
//   y[j] = clamp(fadd(fmul(gain, xs[j]), fmul(v, n[j])))     xs[j] = row[j - shift] inside [0, T), else +0
// every operation rounded once: the build contracts a * b + c into a multiply-add, which has other bits, so the three
// operations are the _rn intrinsics.  Rows are written as draw_row writes them -- a scalar head up to the destination's
// 16-byte boundary, 16-byte stores, a scalar tail -- and the zeros a shift leaves at a row's head or tail go out with the
// same stores.  The shift moves the source against the destination and the noise row starts anywhere, so neither read
// stream is taken for aligned: a vector of four is one 16-byte load where its address allows it, four scalar loads elsewhere.
#include "srwn_common.h"
#include "srwn_augment.h"
#include "srwn_draw_common.h"
#include "srwn_host.h"
#include "srwn_mulaw.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

__device__ __forceinline__ float aug_at(const AugRow& r, int j, int T) {
  const int k = j - r.shift;
  const float x = (k >= 0 && k < T) ? r.src[k] : 0.0f;
  return aug_mix(r, x, r.nz ? r.nz[j] : 0.0f);
}

// four samples from j on: whole vectors inside the row are loaded at once, the ones a shift cuts go element by element
__device__ __forceinline__ f32x4 aug_at4(const AugRow& r, int j, int T, bool src_aligned, bool nz_aligned) {
  const int k = j - r.shift;
  f32x4 x, n = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  if (k >= 0 && k + 3 < T) {
    if (src_aligned) x = *reinterpret_cast<const f32x4*>(r.src + k);
    else x = f32x4{r.src[k], r.src[k + 1], r.src[k + 2], r.src[k + 3]};
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = (k + q >= 0 && k + q < T) ? r.src[k + q] : 0.0f;
  }
  if (r.nz) {
    if (nz_aligned) n = *reinterpret_cast<const f32x4*>(r.nz + j);
    else n = f32x4{r.nz[j], r.nz[j + 1], r.nz[j + 2], r.nz[j + 3]};
  }
  return f32x4{aug_mix(r, x[0], n[0]), aug_mix(r, x[1], n[1]), aug_mix(r, x[2], n[2]), aug_mix(r, x[3], n[3])};
}

// draw_row (srwn_draw_common.h) for an augmented row: dst[j] = f(y[j]) over this workgroup's share [j0, j1)
template <typename Out, typename F>
__device__ __forceinline__ void aug_draw_row(Out* __restrict__ dst, const AugRow& r, int T, int j0, int j1, F f) {
  typedef Out out4 __attribute__((ext_vector_type(4)));
  static_assert(sizeof(Out) == 4, "four-byte outputs");
  // first element of the share whose destination sits on a 16-byte boundary (dst is 4-byte aligned: an fp32 / int32 buffer)
  const int mis = (int)(((uintptr_t)(dst + j0) >> 2) & 3);
  int jb = j0 + ((4 - mis) & 3);
  if (jb > j1) jb = j1;
  const int nvec = (j1 - jb) / 4;
  const int je = jb + 4 * nvec;
  const int tid = (int)threadIdx.x;
  if (tid < jb - j0) dst[j0 + tid] = f(aug_at(r, j0 + tid, T));                 // head: at most 3 elements
  // the body's vectors step by four from jb: one test each says whether the two read streams share the alignment
  const bool src_aligned = (((uintptr_t)(r.src + (jb - r.shift))) & 15) == 0;
  const bool nz_aligned = r.nz && (((uintptr_t)(r.nz + jb)) & 15) == 0;
  for (int v = tid; v < nvec; v += kDrawThreads) {
    const int j = jb + 4 * v;
    const f32x4 y = aug_at4(r, j, T, src_aligned, nz_aligned);
    *reinterpret_cast<out4*>(dst + j) = out4{f(y[0]), f(y[1]), f(y[2]), f(y[3])};
  }
  if (tid < j1 - je) dst[je + tid] = f(aug_at(r, je + tid, T));                 // tail: at most 3 elements
}

__global__ __launch_bounds__(kDrawThreads) void batch_draw_aug_kernel(const DrawArgs a, const AugArgs g) {
  const int b = (int)blockIdx.y;
  const unsigned long long seed = (unsigned long long)a.state[0], step = (unsigned long long)a.state[1];
  const unsigned long long p = (step * (unsigned long long)a.world + (unsigned long long)a.rank) * (unsigned long long)a.B + (unsigned long long)b;
  const Pick k = draw_pick(seed, p, a.N, a.shuffle, a.crop, a.clip_len, a.T);
  const AugRow r = aug_row(g, seed, p, 0, a.clips + (int64_t)k.rec * a.clip_len + k.off, a.T);
  const int j0 = (int)blockIdx.x * kDrawSpan;
  const int j1 = min(a.T, j0 + kDrawSpan);
  aug_draw_row(a.audio0 + (int64_t)b * a.T, r, a.T, j0, j1, [](float y) { return y; });
  if (a.audio1) aug_draw_row(a.audio1 + (int64_t)b * a.T, r, a.T, j0, j1, [](float y) { return y; });
  if (a.codes) {
    const float mu = a.mu, l1p = a.log1p_mu;
    aug_draw_row(a.codes + (int64_t)b * a.T, r, a.T, j0, j1, [mu, l1p](float y) { return mu_law_encode_one(y, mu, l1p); });
  }
  if (blockIdx.x != 0) return;
  if (threadIdx.x == 0) a.indices[b] = (int32_t)k.rec;
  if (a.onehot)
    draw_onehot(a.onehot, a.onehot_dtype, a.labels[k.rec], b, a.onehot_rows, a.num_classes, a.onehot_ld, a.onehot_col0);
}

__global__ __launch_bounds__(kDrawThreads) void pair_draw_aug_kernel(const PairArgs a, const AugArgs g) {
  const int row = (int)blockIdx.y;                                // [0, P): the left clips; [P, 2P): the right ones
  const int side = row < a.P ? 0 : 1;
  const int b = side ? row - a.P : row;
  const unsigned long long seed = (unsigned long long)a.state[0], step = (unsigned long long)a.state[1];
  const unsigned long long p = (step * (unsigned long long)a.world + (unsigned long long)a.rank) * (unsigned long long)a.P + (unsigned long long)b;
  const Pick k = draw_pick(seed, p, a.N, a.shuffle, a.crop, a.clip_len, a.T);
  const PairPick rp = pair_pick(a, seed, p, k);
  const float* src = side ? a.clips + (int64_t)rp.rec * a.clip_len + rp.off
                          : a.clips + (int64_t)k.rec * a.clip_len + k.off;
  const AugRow r = aug_row(g, seed, p, side, src, a.T);
  const int j0 = (int)blockIdx.x * kDrawSpan;
  const int j1 = min(a.T, j0 + kDrawSpan);
  aug_draw_row(a.audio + (int64_t)row * a.T, r, a.T, j0, j1, [](float y) { return y; });
  if (blockIdx.x == 0 && side == 0 && threadIdx.x == 0) {
    const float y = (a.labels[rp.rec] == rp.c) ? 1.0f : 0.0f;     // model.py:747-749: 1 = "same"
    a.y[b] = y;
    a.y_log[b] = y;
    a.left[b] = (int32_t)k.rec;
    a.right[b] = (int32_t)rp.rec;
  }
}

}  // namespace

extern "C" int srwn_batch_draw_aug(const float* clips, const int32_t* labels, int32_t num_clips, int64_t clip_len,
                                   const int64_t* state, int32_t B, int32_t T, int32_t shuffle, int32_t crop, int32_t rank,
                                   int32_t world, float* audio0, float* audio1, int32_t* codes,
                                   int32_t quantization_channels, void* onehot, int64_t onehot_ld, int32_t onehot_rows,
                                   int32_t onehot_col0, int32_t num_classes, int32_t onehot_dtype, int32_t* indices,
                                   int32_t max_shift, float gain_lo, float gain_hi, const float* noise, int32_t noise_clips,
                                   int64_t noise_len, int64_t noise_threshold, float volume_lo, float volume_hi,
                                   void* stream) {
  if (B == 0 || T == 0) return 0;
  DrawArgs a;
  if (int rc = check_batch_draw("batch_draw_aug", clips, labels, num_clips, clip_len, state, B, T, shuffle, crop, rank, world,
                                audio0, audio1, codes, quantization_channels, onehot, onehot_ld, onehot_rows, onehot_col0,
                                num_classes, onehot_dtype, indices, &a))
    return rc;
  AugArgs g;
  if (int rc = check_augment("batch_draw_aug", T, max_shift, gain_lo, gain_hi, noise, noise_clips, noise_len,
                             noise_threshold, volume_lo, volume_hi, &g))
    return rc;
  dim3 grid((unsigned)((T + kDrawSpan - 1) / kDrawSpan), (unsigned)B);
  hipLaunchKernelGGL(batch_draw_aug_kernel, grid, dim3(kDrawThreads), 0, (hipStream_t)stream, a, g);
  return check_launch("batch_draw_aug");
}

extern "C" int srwn_pair_draw_aug(const float* clips, const int32_t* labels, const int32_t* order, const int32_t* place,
                                  const int32_t* class_start, int32_t num_classes, int32_t num_clips, int64_t clip_len,
                                  const int64_t* state, int32_t P, int32_t T, int64_t same_threshold, int32_t shuffle,
                                  int32_t crop, int32_t rank, int32_t world, float* audio, float* y, int32_t* left,
                                  int32_t* right, float* y_log, int32_t max_shift, float gain_lo, float gain_hi,
                                  const float* noise, int32_t noise_clips, int64_t noise_len, int64_t noise_threshold,
                                  float volume_lo, float volume_hi, void* stream) {
  if (P == 0 || T == 0) return 0;
  PairArgs a;
  if (int rc = check_pair_draw("pair_draw_aug", clips, labels, order, place, class_start, num_classes, num_clips, clip_len, state,
                               P, T, same_threshold, shuffle, crop, rank, world, audio, y, left, right, y_log, &a))
    return rc;
  AugArgs g;
  if (int rc = check_augment("pair_draw_aug", T, max_shift, gain_lo, gain_hi, noise, noise_clips, noise_len,
                             noise_threshold, volume_lo, volume_hi, &g))
    return rc;
  dim3 grid((unsigned)((T + kDrawSpan - 1) / kDrawSpan), (unsigned)(2 * P));
  hipLaunchKernelGGL(pair_draw_aug_kernel, grid, dim3(kDrawThreads), 0, (hipStream_t)stream, a, g);
  return check_launch("pair_draw_aug");
}
