// Speed perturbation in the augmented draws (srwn.h, srwn_version() 128): the launches of csrc/srwn_augment.hip with every row
// resampled by a factor of its own near 1 before shift, gain, noise and clamp act on it.
//
//   srwn_batch_draw_warp  srwn_batch_draw_aug's launch; the rows go through dataset.resample_rows at dataset.speed_plan's
//                         steps first, audio, the second audio buffer and the codes alike.
//   srwn_pair_draw_warp   srwn_pair_draw_aug's launch, the two sides of a pair at steps of their own.
//
// A row's step is its seventh draw, mix64((seed ^ kAugSpeedSalt) + GOLDEN * (2 p + side + 1)), uniform on the integers
// [step_lo, step_hi]: a speed is a fixed-point number with 24 fraction bits and positions are 64-bit integers, so no float
// decides which samples an output reads.  Output jj of the resampled row sits at q = jj * step: its source sample is
// i = q >> 24, its phase f = (q >> (24 - log2 P)) & (P - 1) (by floor) and
//   r[jj] = sum over k = 0 .. taps - 1, in that order from +0, of fmul(table[f][k], x[i - (taps / 2 - 1) + k])
// with x = +0 outside [0, T) of the row, every product and every sum rounded once (_rn intrinsics: the build would contract
// them).  The shift then moves the output index, jj = j - shift with +0 outside [0, T), and aug_mix (srwn_augment.h)
// finishes the sample.  A lane forms four neighbouring outputs at once and a row's destinations that share their position
// against the 16-byte boundaries -- audio, second buffer and codes of one allocator do -- are written in one pass.
//
// Reads go through the caches, nothing is staged in LDS: the 4096 outputs of a workgroup read a window of at most 8192 +
// taps consecutive source samples, each of them `taps` times by neighbouring lanes of one wave -- the vector cache serves
// those -- and one table row per output at a phase that jumps by step * P mod P from one output to the next, a gather
// over a table of P * taps * 4 bytes (256 KiB at 16 taps) that stays in L2 and that LDS cannot hold at 64 taps.  A draw
// is 32 workgroups at the flagship shape: latency bounds it, not bandwidth, so what counts is how many loads a lane has in
// flight (warp_samples), and a barrier between staging and use would add to the latency.
// Rows are written as draw_row writes them: a scalar head, 16-byte stores, a scalar tail.
#include "srwn_common.h"
#include "srwn_augment.h"
#include "srwn_draw_common.h"
#include "srwn_host.h"
#include "srwn_mulaw.h"
#include "srwn_resample.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

static_assert(kAugSpeedSalt == 0x6175677370656564ull, "dataset.AUG_SPEED_SALT: the seventh draw's salt (srwn_resample.h)");

// output j of the augmented row: the shift moves the output index, +0 outside the row (computed at index 0, not used)
template <int kN>
__device__ __forceinline__ void warp_at(const AugRow& r, const WarpRow& w, int j, int T, float (&y)[kN]) {
  int jj[kN];
  bool in[kN];
#pragma unroll
  for (int u = 0; u < kN; ++u) {
    const int v = j + u - r.shift;
    in[u] = v >= 0 && v < T;
    jj[u] = in[u] ? v : 0;
  }
  warp_samples<kN>(r.src, w, jj, T, y);
#pragma unroll
  for (int u = 0; u < kN; ++u) y[u] = in[u] ? y[u] : 0.0f;
}

// One pass over this workgroup's share [j0, j1) of a row for up to three destinations that share their position against
// the 16-byte boundaries (null: not written; the first one that is not null sets the pattern): every destination is
// written as draw_row writes it -- a scalar head, 16-byte stores, a scalar tail -- and the tap sums are formed once.
__device__ __forceinline__ void warp_draw_row(float* __restrict__ d0, float* __restrict__ d1, int32_t* __restrict__ dc,
                                              const AugRow& r, const WarpRow& w, int T, int j0, int j1, float mu, float l1p) {
  const void* lead = d0 ? (const void*)(d0 + j0) : d1 ? (const void*)(d1 + j0) : (const void*)(dc + j0);
  int jb = j0 + ((4 - phase16(lead)) & 3);
  if (jb > j1) jb = j1;
  const int nvec = (j1 - jb) / 4;
  const int je = jb + 4 * nvec;
  const int tid = (int)threadIdx.x;
  // head and tail: at most 3 elements each, one lane per element
  const int edge = tid < jb - j0 ? j0 + tid : (tid >= 4 && tid - 4 < j1 - je ? je + tid - 4 : -1);
  if (edge >= 0) {
    float x[1];
    warp_at<1>(r, w, edge, T, x);
    const float y = aug_mix(r, x[0], r.nz ? r.nz[edge] : 0.0f);
    if (d0) d0[edge] = y;
    if (d1) d1[edge] = y;
    if (dc) dc[edge] = mu_law_encode_one(y, mu, l1p);
  }
  const bool nz_aligned = r.nz && (((uintptr_t)(r.nz + jb)) & 15) == 0;
  for (int v = tid; v < nvec; v += kDrawThreads) {
    const int j = jb + 4 * v;
    float x[4];
    warp_at<4>(r, w, j, T, x);
    f32x4 n = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (r.nz) {
      if (nz_aligned) n = *reinterpret_cast<const f32x4*>(r.nz + j);
      else n = f32x4{r.nz[j], r.nz[j + 1], r.nz[j + 2], r.nz[j + 3]};
    }
    const f32x4 y = f32x4{aug_mix(r, x[0], n[0]), aug_mix(r, x[1], n[1]), aug_mix(r, x[2], n[2]), aug_mix(r, x[3], n[3])};
    if (d0) *reinterpret_cast<f32x4*>(d0 + j) = y;
    if (d1) *reinterpret_cast<f32x4*>(d1 + j) = y;
    if (dc) {
      typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
      *reinterpret_cast<i32x4*>(dc + j) = i32x4{mu_law_encode_one(y[0], mu, l1p), mu_law_encode_one(y[1], mu, l1p),
                                                mu_law_encode_one(y[2], mu, l1p), mu_law_encode_one(y[3], mu, l1p)};
    }
  }
}

__global__ __launch_bounds__(kDrawThreads) void batch_draw_warp_kernel(const DrawArgs a, const AugArgs g, const WarpArgs wa) {
  const int b = (int)blockIdx.y;
  const unsigned long long seed = (unsigned long long)a.state[0], step = (unsigned long long)a.state[1];
  const unsigned long long p = (step * (unsigned long long)a.world + (unsigned long long)a.rank) * (unsigned long long)a.B + (unsigned long long)b;
  const Pick k = draw_pick(seed, p, a.N, a.shuffle, a.crop, a.clip_len, a.T);
  const AugRow r = aug_row(g, seed, p, 0, a.clips + (int64_t)k.rec * a.clip_len + k.off, a.T);
  const WarpRow w = warp_row(wa, seed, p, 0);
  const int j0 = (int)blockIdx.x * kDrawSpan;
  const int j1 = min(a.T, j0 + kDrawSpan);
  // destinations that share audio0's position against the 16-byte boundaries join its pass; another one gets its own
  float* const d0 = a.audio0 + (int64_t)b * a.T;
  float* const d1 = a.audio1 ? a.audio1 + (int64_t)b * a.T : nullptr;
  int32_t* const dc = a.codes ? a.codes + (int64_t)b * a.T : nullptr;
  const bool with1 = d1 && phase16(d1) == phase16(d0), withc = dc && phase16(dc) == phase16(d0);
  for (int pass = 0; pass < 3; ++pass) {                          // (one body: passes 1 and 2 are rare)
    float* const e0 = pass == 0 ? d0 : nullptr;
    float* const e1 = (pass == 0 ? with1 : (pass == 1 && d1 && !with1)) ? d1 : nullptr;
    int32_t* const ec = (pass == 0 ? withc : (pass == 2 && dc && !withc)) ? dc : nullptr;
    if (e0 || e1 || ec) warp_draw_row(e0, e1, ec, r, w, a.T, j0, j1, a.mu, a.log1p_mu);
  }
  if (blockIdx.x != 0) return;
  if (threadIdx.x == 0) a.indices[b] = (int32_t)k.rec;
  if (a.onehot)
    draw_onehot(a.onehot, a.onehot_dtype, a.labels[k.rec], b, a.onehot_rows, a.num_classes, a.onehot_ld, a.onehot_col0);
}

__global__ __launch_bounds__(kDrawThreads) void pair_draw_warp_kernel(const PairArgs a, const AugArgs g, const WarpArgs wa) {
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
  const WarpRow w = warp_row(wa, seed, p, side);
  const int j0 = (int)blockIdx.x * kDrawSpan;
  const int j1 = min(a.T, j0 + kDrawSpan);
  warp_draw_row(a.audio + (int64_t)row * a.T, nullptr, nullptr, r, w, a.T, j0, j1, 0.0f, 0.0f);
  if (blockIdx.x == 0 && side == 0 && threadIdx.x == 0) {
    const float y = (a.labels[rp.rec] == rp.c) ? 1.0f : 0.0f;     // model.py:747-749: 1 = "same"
    a.y[b] = y;
    a.y_log[b] = y;
    a.left[b] = (int32_t)k.rec;
    a.right[b] = (int32_t)rp.rec;
  }
}

}  // namespace

extern "C" int srwn_batch_draw_warp(const float* clips, const int32_t* labels, int32_t num_clips, int64_t clip_len,
                                    const int64_t* state, int32_t B, int32_t T, int32_t shuffle, int32_t crop, int32_t rank,
                                    int32_t world, float* audio0, float* audio1, int32_t* codes,
                                    int32_t quantization_channels, void* onehot, int64_t onehot_ld, int32_t onehot_rows,
                                    int32_t onehot_col0, int32_t num_classes, int32_t onehot_dtype, int32_t* indices,
                                    int32_t max_shift, float gain_lo, float gain_hi, const float* noise, int32_t noise_clips,
                                    int64_t noise_len, int64_t noise_threshold, float volume_lo, float volume_hi,
                                    const float* table, int32_t taps, int32_t step_lo, int32_t step_hi, void* stream) {
  if (B == 0 || T == 0) return 0;
  DrawArgs a;
  if (int rc = check_batch_draw("batch_draw_warp", clips, labels, num_clips, clip_len, state, B, T, shuffle, crop, rank, world,
                                audio0, audio1, codes, quantization_channels, onehot, onehot_ld, onehot_rows, onehot_col0,
                                num_classes, onehot_dtype, indices, &a))
    return rc;
  AugArgs g;
  if (int rc = check_augment("batch_draw_warp", T, max_shift, gain_lo, gain_hi, noise, noise_clips, noise_len,
                             noise_threshold, volume_lo, volume_hi, &g))
    return rc;
  WarpArgs w;
  if (int rc = check_resample("batch_draw_warp", table, taps, step_lo, step_hi, &w)) return rc;
  dim3 grid((unsigned)((T + kDrawSpan - 1) / kDrawSpan), (unsigned)B);
  hipLaunchKernelGGL(batch_draw_warp_kernel, grid, dim3(kDrawThreads), 0, (hipStream_t)stream, a, g, w);
  return check_launch("batch_draw_warp");
}

extern "C" int srwn_pair_draw_warp(const float* clips, const int32_t* labels, const int32_t* order, const int32_t* place,
                                   const int32_t* class_start, int32_t num_classes, int32_t num_clips, int64_t clip_len,
                                   const int64_t* state, int32_t P, int32_t T, int64_t same_threshold, int32_t shuffle,
                                   int32_t crop, int32_t rank, int32_t world, float* audio, float* y, int32_t* left,
                                   int32_t* right, float* y_log, int32_t max_shift, float gain_lo, float gain_hi,
                                   const float* noise, int32_t noise_clips, int64_t noise_len, int64_t noise_threshold,
                                   float volume_lo, float volume_hi, const float* table, int32_t taps, int32_t step_lo,
                                   int32_t step_hi, void* stream) {
  if (P == 0 || T == 0) return 0;
  PairArgs a;
  if (int rc = check_pair_draw("pair_draw_warp", clips, labels, order, place, class_start, num_classes, num_clips, clip_len, state,
                               P, T, same_threshold, shuffle, crop, rank, world, audio, y, left, right, y_log, &a))
    return rc;
  AugArgs g;
  if (int rc = check_augment("pair_draw_warp", T, max_shift, gain_lo, gain_hi, noise, noise_clips, noise_len,
                             noise_threshold, volume_lo, volume_hi, &g))
    return rc;
  WarpArgs w;
  if (int rc = check_resample("pair_draw_warp", table, taps, step_lo, step_hi, &w)) return rc;
  dim3 grid((unsigned)((T + kDrawSpan - 1) / kDrawSpan), (unsigned)(2 * P));
  hipLaunchKernelGGL(pair_draw_warp_kernel, grid, dim3(kDrawThreads), 0, (hipStream_t)stream, a, g, w);
  return check_launch("pair_draw_warp");
}
