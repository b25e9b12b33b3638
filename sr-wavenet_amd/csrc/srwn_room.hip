// Room reverberation in the augmented draws (srwn.h, srwn_version() 129): the launches of csrc/srwn_resample.hip with a row
// convolved with a room impulse response of up to SRWN_ROOM_MAX_TAPS taps, between resampling and shift / gain / noise.
//
//   srwn_batch_draw_room  srwn_batch_draw_warp's launch (a null table: no resampling, the rows of srwn_batch_draw_aug);
//                         with probability rir_threshold / 2^32 a row goes through dataset.reverb_rows first.
//   srwn_pair_draw_room   srwn_pair_draw_warp's launch, the two sides of a pair with coins and responses of their own.
//
// A row's eighth and ninth draws, mix64((seed ^ salt) + GOLDEN * (2 p + side + 1)) under kAugRirCoinSalt and
// kAugRirPickSalt, say whether it is reverberated and with which response h (dataset.reverb_plan).  With r the resampled
// (or copied) row, +0 outside [0, T),
//   e[jj] = sum over k = 0 .. K - 1, in that order from +0, of fmul(h[k], r[jj - k])
// every product and every sum rounded once (_rn intrinsics: the build would contract them; an fp32 MFMA is a chain of
// fused multiply-adds and has other bits).  The shift then moves the output index and aug_mix finishes the sample.
//
// A row whose coin is off is staged -- resampled by warp_samples, or copied -- and written by the same stage C; the rule
// is the older entries', so the row has their bits (tests/test_gpu_room_entries.py draws both on the device).  The older
// units' row writers inlined beside the tap loop cost this kernel about a hundred scalar registers more than it has.
// A reverberated row is compute bound -- K multiply-add pairs per output against 16 per output of the resampler -- so
// the grid is finer than the other draws': kRoomSpan = 512 outputs per workgroup, 256 workgroups at 8 x 16 000, and every
// lane forms two neighbouring outputs.
//   stage A  the window r[jj_lo - K' .. jj_hi) of this workgroup's outputs goes into LDS (K' = K rounded up to even), by
//            warp_samples or by a copy, +0 outside the row: (kRoomSpan + K') * 4 bytes, 34 KiB at the cap.
//   stage B  the lane with outputs J, J + 1 walks the taps two at a time: it holds the pair (r[J - k], r[J - k + 1]) and
//            one 8-byte LDS read brings (r[J - k - 2], r[J - k - 1]), which serves taps k and k + 1 of both outputs --
//            half an LDS read per product, lanes at stride 8 bytes, no bank conflict.  The taps of a row are the same in
//            every lane, so they are read with scalar loads.
//   stage C  the tap sums go back into LDS (the window is dead by then) and the destinations are written from there as
//            warp_draw_row writes them: a scalar head, 16-byte stores, a scalar tail, once per destination, destinations
//            that share their position against the 16-byte boundaries in one pass.
#include "srwn_common.h"
#include "srwn_augment.h"
#include "srwn_draw_common.h"
#include "srwn_host.h"
#include "srwn_mulaw.h"
#include "srwn_resample.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

constexpr unsigned long long kAugRirCoinSalt = 0x61756772636F696Eull;  // dataset.AUG_RIR_COIN_SALT
constexpr unsigned long long kAugRirPickSalt = 0x617567727069636Bull;  // dataset.AUG_RIR_PICK_SALT
constexpr int kRoomSpan = 512;                                         // outputs per workgroup: two per lane
constexpr int kRoomBlock = 8;                                          // taps fetched ahead of their use (even)
static_assert(kRoomSpan == 2 * kDrawThreads && 4096 % kRoomSpan == 0 && kRoomSpan >= 256, "a power of two in [256, 4096]");

struct RoomArgs { const float* rir; unsigned long long threshold; int32_t n, len; };

// dataset.reverb_plan for position p and side: the row's response, null where its coin is off
__device__ __forceinline__ const float* room_row(const RoomArgs& q, unsigned long long seed, unsigned long long p, int side) {
  const unsigned long long key = kGolden * (2ull * p + (unsigned long long)side + 1ull);
  if (!((mix64((seed ^ kAugRirCoinSalt) + key) >> 32) < q.threshold)) return nullptr;
  const unsigned long long rec = ((mix64((seed ^ kAugRirPickSalt) + key) >> 32) * (unsigned long long)q.n) >> 32;
  return q.rir + (size_t)rec * (size_t)q.len;
}

// stage A: lds[i] = r[w0 + i] for i in [0, n), the resampled (or copied) row, +0 outside [0, hi) of it; hi <= T
__device__ __forceinline__ void room_stage(float* __restrict__ lds, const AugRow& r, const WarpRow& w, int T, int w0, int n,
                                           int hi) {
  const int tid = (int)threadIdx.x;
  if (w.table) {
    for (int i = 2 * tid; i < n; i += 2 * kDrawThreads) {
      int jj[2];
      bool in[2];
      float x[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int at = w0 + i + u;
        in[u] = at >= 0 && at < hi;
        jj[u] = in[u] ? at : 0;
      }
      warp_samples<2>(r.src, w, jj, T, x);
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (i + u < n) lds[i + u] = in[u] ? x[u] : 0.0f;
    }
  } else {
    for (int i = tid; i < n; i += kDrawThreads) {
      const int at = w0 + i;
      lds[i] = (at >= 0 && at < hi) ? r.src[at] : 0.0f;
    }
  }
  __syncthreads();
}

// stage B: the window r[jj_lo - Ke ..] in lds becomes the tap sums e[jj_lo ..], two per lane (Ke: K rounded up to even)
__device__ __forceinline__ void room_sums(float* __restrict__ lds, const float* __restrict__ taps, int K, int Ke) {
  // the responses are only read while the launch runs and a row's is the same in every lane: through the constant address
  // space its taps are scalar loads, sixteen to an instruction
  typedef const float __attribute__((address_space(4))) ctap;
  ctap* const h = reinterpret_cast<ctap*>(reinterpret_cast<uintptr_t>(taps));
  const int tid = (int)threadIdx.x;
  // the lane's outputs are J = jj_lo + 2 tid and J + 1; r[J] sits at lds[2 tid + Ke], an 8-byte boundary
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const float* at = lds + 2 * tid + Ke;
  f32x2 P = *reinterpret_cast<const f32x2*>(at);                  // (r[J - k], r[J - k + 1]) at k = 0
  float a0 = 0.0f, a1 = 0.0f;
  int k = 0;
  // blocks of kRoomBlock taps, the next block's taps and window pairs fetched before this block's arithmetic: a wave is
  // alone on its SIMD at the flagship shape, so nothing else hides the scalar load's and the LDS reads' latency
  if (K >= kRoomBlock) {
    float hn[kRoomBlock];
    f32x2 qn[kRoomBlock / 2];
#pragma unroll
    for (int u = 0; u < kRoomBlock; ++u) hn[u] = h[u];
#pragma unroll
    for (int m = 0; m < kRoomBlock / 2; ++m) qn[m] = *reinterpret_cast<const f32x2*>(at - 2 - 2 * m);
    for (; k + kRoomBlock <= K; k += kRoomBlock) {
      float hc[kRoomBlock];
      f32x2 qc[kRoomBlock / 2];
#pragma unroll
      for (int u = 0; u < kRoomBlock; ++u) hc[u] = hn[u];
#pragma unroll
      for (int m = 0; m < kRoomBlock / 2; ++m) qc[m] = qn[m];
      const int kn = min(k + kRoomBlock, K - kRoomBlock);         // the next block; behind the last one, itself once more
#pragma unroll
      for (int u = 0; u < kRoomBlock; ++u) hn[u] = h[kn + u];
#pragma unroll
      for (int m = 0; m < kRoomBlock / 2; ++m) qn[m] = *reinterpret_cast<const f32x2*>(at - kn - 2 - 2 * m);
#pragma unroll
      for (int m = 0; m < kRoomBlock / 2; ++m) {
        const f32x2 Q = qc[m];                                    // (r[J - k' - 2], r[J - k' - 1]) at k' = k + 2 m
        a0 = __fadd_rn(a0, __fmul_rn(hc[2 * m], P[0]));
        a1 = __fadd_rn(a1, __fmul_rn(hc[2 * m], P[1]));
        a0 = __fadd_rn(a0, __fmul_rn(hc[2 * m + 1], Q[1]));
        a1 = __fadd_rn(a1, __fmul_rn(hc[2 * m + 1], P[0]));
        P = Q;
      }
    }
  }
  for (; k + 1 < K; k += 2) {                                     // what is left of an even number of taps
    const f32x2 Q = *reinterpret_cast<const f32x2*>(at - k - 2);  // (r[J - k - 2], r[J - k - 1])
    const float h0 = h[k], h1 = h[k + 1];
    a0 = __fadd_rn(a0, __fmul_rn(h0, P[0]));
    a1 = __fadd_rn(a1, __fmul_rn(h0, P[1]));
    a0 = __fadd_rn(a0, __fmul_rn(h1, Q[1]));
    a1 = __fadd_rn(a1, __fmul_rn(h1, P[0]));
    P = Q;
  }
  if (k < K) {                                                    // an odd K's last tap
    const float h0 = h[k];
    a0 = __fadd_rn(a0, __fmul_rn(h0, P[0]));
    a1 = __fadd_rn(a1, __fmul_rn(h0, P[1]));
  }
  __syncthreads();                                                // every lane has read its window
  *reinterpret_cast<f32x2*>(lds + 2 * tid) = f32x2{a0, a1};
  __syncthreads();
}

// a row's samples in front of the shift for this workgroup's outputs [j0, j1) -- jj = j - shift inside [0, T) -- into lds:
// the tap sums of a reverberated row (h), else the resampled or copied row itself, which then has the bits the older
// entries give it (one rule, whoever evaluates it)
__device__ __forceinline__ void room_row_samples(float* __restrict__ lds, const AugRow& r, const WarpRow& w,
                                                 const float* __restrict__ h, int K, int T, int j0, int j1, int* jj_lo,
                                                 int* jj_hi) {
  const int lo = min(max(j0 - r.shift, 0), T), hi = min(max(j1 - r.shift, 0), T);
  *jj_lo = lo;
  *jj_hi = hi;
  if (hi <= lo) return;                                           // (the shift leaves this share empty: all +0)
  const int Ke = h ? (K + 1) & ~1 : 0;
  room_stage(lds, r, w, T, lo - Ke, Ke + ((hi - lo + 1) & ~1), hi);
  if (h) room_sums(lds, h, K, Ke);
}

// output j of the augmented row from the tap sums in LDS: the shift moves the output index, +0 outside the row
__device__ __forceinline__ float room_at(const float* lds, const AugRow& r, int j, int jj_lo, int jj_hi) {
  const int v = j - r.shift;
  return (v >= jj_lo && v < jj_hi) ? lds[v - jj_lo] : 0.0f;
}

// stage C: warp_draw_row's pass over [j0, j1) with the tap sums read from LDS
__device__ __forceinline__ void room_draw_row(float* __restrict__ d0, float* __restrict__ d1, int32_t* __restrict__ dc,
                                              const float* lds, const AugRow& r, int jj_lo, int jj_hi, int j0, int j1,
                                              float mu, float l1p) {
  const void* lead = d0 ? (const void*)(d0 + j0) : d1 ? (const void*)(d1 + j0) : (const void*)(dc + j0);
  int jb = j0 + ((4 - phase16(lead)) & 3);
  if (jb > j1) jb = j1;
  const int nvec = (j1 - jb) / 4;
  const int je = jb + 4 * nvec;
  const int tid = (int)threadIdx.x;
  // head and tail: at most 3 elements each, one lane per element
  const int edge = tid < jb - j0 ? j0 + tid : (tid >= 4 && tid - 4 < j1 - je ? je + tid - 4 : -1);
  if (edge >= 0) {
    const float y = aug_mix(r, room_at(lds, r, edge, jj_lo, jj_hi), r.nz ? r.nz[edge] : 0.0f);
    if (d0) d0[edge] = y;
    if (d1) d1[edge] = y;
    if (dc) dc[edge] = mu_law_encode_one(y, mu, l1p);
  }
  const bool nz_aligned = r.nz && (((uintptr_t)(r.nz + jb)) & 15) == 0;
  for (int v = tid; v < nvec; v += kDrawThreads) {
    const int j = jb + 4 * v;
    f32x4 n = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (nz_aligned) n = *reinterpret_cast<const f32x4*>(r.nz + j);
    else if (r.nz) n = f32x4{r.nz[j], r.nz[j + 1], r.nz[j + 2], r.nz[j + 3]};
    f32x4 y;
#pragma unroll
    for (int u = 0; u < 4; ++u) y[u] = aug_mix(r, room_at(lds, r, j + u, jj_lo, jj_hi), n[u]);
    if (d0) *reinterpret_cast<f32x4*>(d0 + j) = y;
    if (d1) *reinterpret_cast<f32x4*>(d1 + j) = y;
    if (dc) {
      typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
      *reinterpret_cast<i32x4*>(dc + j) = i32x4{mu_law_encode_one(y[0], mu, l1p), mu_law_encode_one(y[1], mu, l1p),
                                                mu_law_encode_one(y[2], mu, l1p), mu_law_encode_one(y[3], mu, l1p)};
    }
  }
}

__global__ __launch_bounds__(kDrawThreads) void batch_draw_room_kernel(const DrawArgs a, const AugArgs g, const WarpArgs wa,
                                                                       const RoomArgs q) {
  extern __shared__ float lds[];
  const int b = (int)blockIdx.y;
  const unsigned long long seed = (unsigned long long)a.state[0], step = (unsigned long long)a.state[1];
  const unsigned long long p = (step * (unsigned long long)a.world + (unsigned long long)a.rank) * (unsigned long long)a.B + (unsigned long long)b;
  const Pick k = draw_pick(seed, p, a.N, a.shuffle, a.crop, a.clip_len, a.T);
  const AugRow r = aug_row(g, seed, p, 0, a.clips + (int64_t)k.rec * a.clip_len + k.off, a.T);
  const WarpRow w = warp_row(wa, seed, p, 0);
  const float* const h = room_row(q, seed, p, 0);
  if (blockIdx.x == 0) {                                          // (first: the tap loop needs the scalar registers)
    if (threadIdx.x == 0) a.indices[b] = (int32_t)k.rec;
    if (a.onehot)
      draw_onehot(a.onehot, a.onehot_dtype, a.labels[k.rec], b, a.onehot_rows, a.num_classes, a.onehot_ld, a.onehot_col0);
  }
  const int j0 = (int)blockIdx.x * kRoomSpan;
  const int j1 = min(a.T, j0 + kRoomSpan);
  int jj_lo, jj_hi;
  room_row_samples(lds, r, w, h, q.len, a.T, j0, j1, &jj_lo, &jj_hi);
  // destinations that share audio0's position against the 16-byte boundaries join its pass; another one gets its own
  float* const d0 = a.audio0 + (int64_t)b * a.T;
  float* const d1 = a.audio1 ? a.audio1 + (int64_t)b * a.T : nullptr;
  int32_t* const dc = a.codes ? a.codes + (int64_t)b * a.T : nullptr;
  const bool with1 = d1 && phase16(d1) == phase16(d0), withc = dc && phase16(dc) == phase16(d0);
  for (int pass = 0; pass < 3; ++pass) {                          // (one body: passes 1 and 2 are rare)
    float* const e0 = pass == 0 ? d0 : nullptr;
    float* const e1 = (pass == 0 ? with1 : (pass == 1 && d1 && !with1)) ? d1 : nullptr;
    int32_t* const ec = (pass == 0 ? withc : (pass == 2 && dc && !withc)) ? dc : nullptr;
    if (e0 || e1 || ec) room_draw_row(e0, e1, ec, lds, r, jj_lo, jj_hi, j0, j1, a.mu, a.log1p_mu);
  }
}

__global__ __launch_bounds__(kDrawThreads) void pair_draw_room_kernel(const PairArgs a, const AugArgs g, const WarpArgs wa,
                                                                      const RoomArgs q) {
  extern __shared__ float lds[];
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
  const float* const h = room_row(q, seed, p, side);
  const int j0 = (int)blockIdx.x * kRoomSpan;
  const int j1 = min(a.T, j0 + kRoomSpan);
  if (blockIdx.x == 0 && side == 0 && threadIdx.x == 0) {
    const float y = (a.labels[rp.rec] == rp.c) ? 1.0f : 0.0f;     // model.py:747-749: 1 = "same"
    a.y[b] = y;
    a.y_log[b] = y;
    a.left[b] = (int32_t)k.rec;
    a.right[b] = (int32_t)rp.rec;
  }
  int jj_lo, jj_hi;
  room_row_samples(lds, r, w, h, q.len, a.T, j0, j1, &jj_lo, &jj_hi);
  room_draw_row(a.audio + (int64_t)row * a.T, nullptr, nullptr, lds, r, jj_lo, jj_hi, j0, j1, 0.0f, 0.0f);
}

// the resampling block of the room entries: check_resample's, or a null table with no taps at step 2^24 -- no resampling
int check_room_resample(const char* who, const float* table, int32_t taps, int32_t step_lo, int32_t step_hi, WarpArgs* w) {
  if (table) return check_resample(who, table, taps, step_lo, step_hi, w);
  if (taps != 0 || step_lo != (1 << kSpeedBits) || step_hi != (1 << kSpeedBits))
    return set_error(SRWN_E_NULL, "%s: null resampling table with %d taps at steps [%d, %d] (no resampling: 0 taps, 2^24)",
                     who, taps, step_lo, step_hi);
  w->table = nullptr; w->taps = 0; w->step_lo = step_lo; w->step_hi = step_hi;
  return 0;
}

// the room block of both entries, checked before any launch
int check_room(const char* who, const float* rir, int32_t rir_clips, int32_t rir_len, int64_t rir_threshold, RoomArgs* q) {
  if (rir_clips < 1) return set_error(SRWN_E_SHAPE, "%s: %d room responses", who, rir_clips);
  if (rir_len < 1 || rir_len > SRWN_ROOM_MAX_TAPS)
    return set_error(SRWN_E_SHAPE, "%s: responses of %d taps (1 to %d)", who, rir_len, SRWN_ROOM_MAX_TAPS);
  if (rir_threshold < 0 || rir_threshold > (1ll << 32))
    return set_error(SRWN_E_SHAPE, "%s: rir_threshold %lld outside [0, 2^32]", who, (long long)rir_threshold);
  if (!rir) return set_error(SRWN_E_NULL, "%s: null room responses", who);
  if ((uintptr_t)rir & 3) return set_error(SRWN_E_SHAPE, "%s: the fp32 buffers must be 4-byte aligned", who);
  q->rir = rir; q->threshold = (unsigned long long)rir_threshold; q->n = rir_clips; q->len = rir_len;
  return 0;
}

size_t room_lds_bytes(int32_t rir_len) { return (size_t)(kRoomSpan + ((rir_len + 1) & ~1)) * sizeof(float); }

}  // namespace

extern "C" int srwn_batch_draw_room(const float* clips, const int32_t* labels, int32_t num_clips, int64_t clip_len,
                                    const int64_t* state, int32_t B, int32_t T, int32_t shuffle, int32_t crop, int32_t rank,
                                    int32_t world, float* audio0, float* audio1, int32_t* codes,
                                    int32_t quantization_channels, void* onehot, int64_t onehot_ld, int32_t onehot_rows,
                                    int32_t onehot_col0, int32_t num_classes, int32_t onehot_dtype, int32_t* indices,
                                    int32_t max_shift, float gain_lo, float gain_hi, const float* noise, int32_t noise_clips,
                                    int64_t noise_len, int64_t noise_threshold, float volume_lo, float volume_hi,
                                    const float* table, int32_t taps, int32_t step_lo, int32_t step_hi, const float* rir,
                                    int32_t rir_clips, int32_t rir_len, int64_t rir_threshold, void* stream) {
  if (B == 0 || T == 0) return 0;
  DrawArgs a;
  if (int rc = check_batch_draw("batch_draw_room", clips, labels, num_clips, clip_len, state, B, T, shuffle, crop, rank, world,
                                audio0, audio1, codes, quantization_channels, onehot, onehot_ld, onehot_rows, onehot_col0,
                                num_classes, onehot_dtype, indices, &a))
    return rc;
  AugArgs g;
  if (int rc = check_augment("batch_draw_room", T, max_shift, gain_lo, gain_hi, noise, noise_clips, noise_len,
                             noise_threshold, volume_lo, volume_hi, &g))
    return rc;
  WarpArgs w;
  if (int rc = check_room_resample("batch_draw_room", table, taps, step_lo, step_hi, &w)) return rc;
  RoomArgs q;
  if (int rc = check_room("batch_draw_room", rir, rir_clips, rir_len, rir_threshold, &q)) return rc;
  dim3 grid((unsigned)((T + kRoomSpan - 1) / kRoomSpan), (unsigned)B);
  hipLaunchKernelGGL(batch_draw_room_kernel, grid, dim3(kDrawThreads), room_lds_bytes(rir_len), (hipStream_t)stream, a, g, w, q);
  return check_launch("batch_draw_room");
}

extern "C" int srwn_pair_draw_room(const float* clips, const int32_t* labels, const int32_t* order, const int32_t* place,
                                   const int32_t* class_start, int32_t num_classes, int32_t num_clips, int64_t clip_len,
                                   const int64_t* state, int32_t P, int32_t T, int64_t same_threshold, int32_t shuffle,
                                   int32_t crop, int32_t rank, int32_t world, float* audio, float* y, int32_t* left,
                                   int32_t* right, float* y_log, int32_t max_shift, float gain_lo, float gain_hi,
                                   const float* noise, int32_t noise_clips, int64_t noise_len, int64_t noise_threshold,
                                   float volume_lo, float volume_hi, const float* table, int32_t taps, int32_t step_lo,
                                   int32_t step_hi, const float* rir, int32_t rir_clips, int32_t rir_len,
                                   int64_t rir_threshold, void* stream) {
  if (P == 0 || T == 0) return 0;
  PairArgs a;
  if (int rc = check_pair_draw("pair_draw_room", clips, labels, order, place, class_start, num_classes, num_clips, clip_len, state,
                               P, T, same_threshold, shuffle, crop, rank, world, audio, y, left, right, y_log, &a))
    return rc;
  AugArgs g;
  if (int rc = check_augment("pair_draw_room", T, max_shift, gain_lo, gain_hi, noise, noise_clips, noise_len,
                             noise_threshold, volume_lo, volume_hi, &g))
    return rc;
  WarpArgs w;
  if (int rc = check_room_resample("pair_draw_room", table, taps, step_lo, step_hi, &w)) return rc;
  RoomArgs q;
  if (int rc = check_room("pair_draw_room", rir, rir_clips, rir_len, rir_threshold, &q)) return rc;
  dim3 grid((unsigned)((T + kRoomSpan - 1) / kRoomSpan), (unsigned)(2 * P));
  hipLaunchKernelGGL(pair_draw_room_kernel, grid, dim3(kDrawThreads), room_lds_bytes(rir_len), (hipStream_t)stream, a, g, w, q);
  return check_launch("pair_draw_room");
}
