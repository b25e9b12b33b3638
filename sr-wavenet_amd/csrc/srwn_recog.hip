// Streaming classifier: the causal stack of class WaveNet (model.py:33-62) as an inference-only stream that emits the
// pooled output of every window position it has passed.  gfx950 (MI355X) only; MFMA orientation and lane maps:
// srwn_common.h.  The stack itself runs through srwn_residual_group_fwd_stream_z (csrc/srwn_group.hip); here is what
// stands around it, one launch each:
//   stream entry   the K = 2 input conv (model.py:40, no RightShift, no conditioning) from the chunk's audio and a
//                  one-sample carry, written behind the history rows of the first boundary buffer
//   pooled head    skip sum from the stored z (gate rebuilt as the skip sum's SRWN_PRO_GATE does), relu, head 1x1, relu
//                  (model.py:50-54) and the sum of r1 over each hop, one workgroup per (stream, hop): r0, r1 and the
//                  per-step logits never reach HBM.  The hop sum lands in a per-stream ring of fp32 rows [S]
//   hop sum        the parity twin of the head's last step: the same sum from an r1 buffer that srwn_pw_linear wrote
//   window mean    (sum of the nW = window / hop ring rows that end at a hop, oldest first) / window: the pooled r1 of
//                  the window position that ends there (the AVG pool of model.py:58 commutes with the last 1x1); the
//                  existing srwn_pooled_head turns the rows into probabilities
//   roll           the history roll of the boundary buffers, the carry and the clock
// A stream only ever advances by whole hops at hop-aligned absolute times, and a hop's 32-row tiles are cut from the
// hop's first row: every ring row depends on absolute time only, so a stream has the same bits in any chunking, at any
// batch size and in any row of the batch.
//
// The slot forms (classifier pools; srwn.h, srwn_version() 115) are the same kernels on the pool's table of SrwnSynthSlot
// instead of the clock: slot u is a stream at its own absolute time slots[u].t (a multiple of hop) with ran =
// slot_rows(slots[u], n) rows in this chunk (a multiple of hop too).  The host writes the whole table before every step and
// no launch modifies it.  What the clock forms take from *clock they take from the slot; a workgroup or thread whose hop or
// row lies beyond ran returns before it reads or writes anything.  The stream entry reads the audio -- and the sample before
// the chunk -- from the pool's audio ring, so the slot forms keep no carry.
// Each pair of entry points is ONE kernel template with a SLOTS flag and ONE host body (`*_impl<SLOTS>`: the checks, the
// dtype / R / S dispatch and the launch, written once); the ten extern "C" functions at the end only name themselves and
// pass their arguments on.  ClockArg, slot_rows and RollEntry are srwn_slots.h's, shared with srwn_stream.hip.
#include <cmath>
#include <type_traits>
#include "srwn_common.h"
#include "srwn_host.h"
#include "srwn_slots.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

// ------------------------------------------------------------------------------------------
// stream entry: 8 channels per thread, one row per group of R/8 lanes
//   v = b; v = fma(x[t-1], w[0], v); v = fma(x[t], w[1], v); round to T          (srwn_causal_conv1d_fwd, shift 0)
// Clock form: x [B][x_stride] is the chunk's audio, x[-1] of the chunk the carry (zero at the stream's start: the conv's
// zero padding).  SLOTS: x is the pool's audio ring of x_stride columns per slot; row t < ran(b) of slot b is absolute
// sample s = slots[b].t + t in column s mod x_stride, x[s - 1] from the ring too (0 at s = 0), no carry.  Only the fetch
// of the two samples differs.
// ------------------------------------------------------------------------------------------
template <typename T, bool SLOTS = false>
__global__ __launch_bounds__(256) void recog_stream_in_kernel(const float* __restrict__ x, int64_t x_stride,
                                                              const float* __restrict__ carry,
                                                              const float* __restrict__ w, const float* __restrict__ bias,
                                                              T* __restrict__ out, int64_t out_clip_rows, int hist, int B,
                                                              int n, int R, const SrwnSynthSlot* __restrict__ slots) {
  // (one argument list for both forms: the clock form is launched with slots = null, the slot form with carry = null,
  // and neither instantiation reads the other's)
  const int lpr = R / 8;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = idx / lpr;
  const int sub = (int)(idx % lpr);
  if (row >= (int64_t)B * n) return;
  const int b = (int)(row / n);
  const int t = (int)(row - (int64_t)b * n);
  float x0, x1;
  if constexpr (SLOTS) {
    const SrwnSynthSlot sl = slots[b];
    if (sl.t < 0 || t >= slot_rows(sl, n)) return;
    const int ring_len = (int)x_stride;
    const float* xb = x + (int64_t)b * ring_len;
    const long long s = sl.t + t;
    const int c1 = (int)(s % ring_len);
    const int c0 = c1 > 0 ? c1 - 1 : ring_len - 1;
    x0 = s >= 1 ? xb[c0] : 0.0f;
    x1 = xb[c1];
  } else {
    const float* xb = x + (int64_t)b * x_stride;
    x0 = t >= 1 ? xb[t - 1] : carry[b];
    x1 = xb[t];
  }
  T* d = out + ((int64_t)b * out_clip_rows + hist + t) * R + 8 * sub;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = bias[8 * sub + j];
    v[j] = fmaf(x0, w[8 * sub + j], v[j]);
    v[j] = fmaf(x1, w[R + 8 * sub + j], v[j]);
  }
  store4(d, v[0], v[1], v[2], v[3]);
  store4(d + 4, v[4], v[5], v[6], v[7]);
}

// The sum of a tile's 32 rows in the order both forms of the hop sum use: neighbours first, then pairs of pairs ...
// (what an xor butterfly over the 32 lanes of a half wave leaves in every lane).
__device__ __forceinline__ float half_wave_sum(float v) {
#pragma unroll
  for (int s = 1; s < 32; s <<= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// ------------------------------------------------------------------------------------------
// pooled head of a chunk of k hops.  Workgroup = (stream b, hop i of the chunk), 4 waves; wave w owns the output
// channels [w * S/4, (w + 1) * S/4) of both products.  Per 32-row tile of the hop, in time order:
//   accS = bs_sum + sum_l Ws_l . gate(z_l)      B fragments: 8 channels of one z row per lane (natural k order), the gate
//                                               on the fragment as pw_load_b<SRWN_PRO_GATE>; A fragments from the
//                                               packed skip image in L2 (rows = skip channel, k = l * R + n)
//   r0 = relu(accS) rounded to T -> xch[32][S]  LDS, rows = time: the B operand of the head 1x1 for all four waves
//   acc1 = b1 + W1 . r0;  r1 = relu(acc1) rounded to T
//   hsum += half_wave_sum(r1 of the tile's valid rows)
// and at the end H[b][(j0 + i) mod ring][:] = hsum, j0 = *clock / hop.  The arithmetic of r0 and r1 is srwn_pw_linear's
// (accumulators start at the bias, k-steps in order).
// LDS: xch = 32 x (S + 16 / sizeof(T)) x sizeof(T) bytes -- 33 280 for S = 256 in fp32, 16 896 in bf16.
// ------------------------------------------------------------------------------------------
// SLOTS: `clock` is the pool's table; the workgroup of (slot u, hop i) works only when (i + 1) * hop <= ran(u).
template <typename T, int R, int S, bool SLOTS = false>
__global__ __launch_bounds__(256) void pooled_stream_head_kernel(const T* __restrict__ z, int64_t z_layer_stride,
                                                                  int64_t z_clip_rows, int L, const T* __restrict__ wskip,
                                                                  const float* __restrict__ bs_sum,
                                                                  const T* __restrict__ w1, const float* __restrict__ b1,
                                                                  float* __restrict__ ring, int ring_rows,
                                                                  typename ClockArg<SLOTS>::in clock, int k, int hop) {
  constexpr int MTW = S / 128;                // 32-channel output tiles per wave
  constexpr int KSL = R / 16;                 // k-steps per layer
  constexpr int KS1 = S / 16;
  constexpr int LS = RowStage<T>::stride(S);
  __shared__ __attribute__((aligned(16))) T xch[32 * LS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int col = lane & 31, half = lane >> 5;
  const int b = (int)blockIdx.x / k, i = (int)blockIdx.x % k;
  long long j0_ = 0;
  if constexpr (SLOTS) {      // (workgroup-uniform, before the first barrier)
    const SrwnSynthSlot sl = clock[b];
    if (sl.t < 0 || (i + 1) * hop > slot_rows(sl, k * hop)) return;
    j0_ = sl.t / hop;
  }
  const int ks_skip = L * KSL;
  const Frag<T>* ws = reinterpret_cast<const Frag<T>*>(wskip) + (size_t)(wave * MTW) * ks_skip * 64 + lane;
  const Frag<T>* wh = reinterpret_cast<const Frag<T>*>(w1) + (size_t)(wave * MTW) * KS1 * 64 + lane;
  float bsv[MTW][16], b1v[MTW][16], hsum[MTW][16];
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int n = 32 * (wave * MTW + mt) + crow(q, half);
      bsv[mt][q] = bs_sum[n];
      b1v[mt][q] = b1[n];
      hsum[mt][q] = 0.0f;
    }
  const T* zb = z + ((int64_t)b * z_clip_rows + (int64_t)i * hop) * R + 8 * half;
  for (int t0 = 0; t0 < hop; t0 += 32) {
    const int valid = hop - t0 < 32 ? hop - t0 : 32;
    const int trow = t0 + (col < valid ? col : valid - 1);      // (a masked column re-reads the hop's last row)
    const T* zr = zb + (int64_t)trow * R;
    f32x16 acc[MTW];
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[mt][q] = bsv[mt][q];
    for (int l = 0; l < L; ++l) {
      Frag<T> bf[KSL];
#pragma unroll
      for (int ks = 0; ks < KSL; ++ks) {
        bf[ks] = load_nat(zr + (int64_t)l * z_layer_stride + 16 * ks);
        gate_frag<T>(bf[ks]);
      }
#pragma unroll
      for (int ks = 0; ks < KSL; ++ks)
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) mma(acc[mt], ws[((size_t)mt * ks_skip + l * KSL + ks) * 64], bf[ks]);
    }
    __syncthreads();                          // the previous tile's reads of xch are done
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        store4(xch + col * LS + 32 * (wave * MTW + mt) + 8 * g + 4 * half, fmaxf(acc[mt][4 * g], 0.0f),
               fmaxf(acc[mt][4 * g + 1], 0.0f), fmaxf(acc[mt][4 * g + 2], 0.0f), fmaxf(acc[mt][4 * g + 3], 0.0f));
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[mt][q] = b1v[mt][q];
#pragma unroll 4
    for (int ks = 0; ks < KS1; ++ks) {
      const Frag<T> bf = load_nat(xch + col * LS + 16 * ks + 8 * half);
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) mma(acc[mt], wh[((size_t)mt * KS1 + ks) * 64], bf);
    }
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float r1 = (float)(T)fmaxf(acc[mt][q], 0.0f);
        hsum[mt][q] += half_wave_sum(col < valid ? r1 : 0.0f);
      }
  }
  long long j_;
  if constexpr (SLOTS) j_ = j0_ + i; else j_ = *clock / hop + i;
  const long long j = j_;
  float* dst = ring + ((int64_t)b * ring_rows + (int64_t)(j % ring_rows)) * S;
  if (col == 0) {
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
      for (int q = 0; q < 16; ++q) dst[32 * (wave * MTW + mt) + crow(q, half)] = hsum[mt][q];
  }
}

// ------------------------------------------------------------------------------------------
// hop sum (parity twin): r1 [B][r1_clip_rows][S] of the chunk -> the ring rows of its k hops.  One wave per (stream, hop,
// 2 channels): lane (col, half) reads row t0 + col of channel 2 * w + half, tiles in time order, the tile's rows summed as
// the head kernel sums them.
// ------------------------------------------------------------------------------------------
template <typename T, bool SLOTS = false>
__global__ __launch_bounds__(256) void hop_sum_kernel(const T* __restrict__ r1, int64_t r1_clip_rows,
                                                      float* __restrict__ ring, int ring_rows,
                                                      typename ClockArg<SLOTS>::in clock, int k, int hop, int S) {
  const int lane = threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int b = (int)blockIdx.x / k, i = (int)blockIdx.x % k;
  long long j_;
  if constexpr (SLOTS) {
    const SrwnSynthSlot sl = clock[b];
    if (sl.t < 0 || (i + 1) * hop > slot_rows(sl, k * hop)) return;
    j_ = sl.t / hop + i;
  } else j_ = *clock / hop + i;
  const long long j = j_;
  float* dst = ring + ((int64_t)b * ring_rows + (int64_t)(j % ring_rows)) * S;
  const T* src = r1 + ((int64_t)b * r1_clip_rows + (int64_t)i * hop) * S;
  for (int s = 2 * wave + half; s < S; s += 8) {      // (both halves of a wave run the same number of rounds: S is even)
    float h = 0.0f;
    for (int t0 = 0; t0 < hop; t0 += 32) {
      const int t = t0 + col;
      const float v = t < hop ? (float)src[(int64_t)t * S + s] : 0.0f;
      h += half_wave_sum(v);
    }
    if (col == 0) dst[s] = h;
  }
}

// ------------------------------------------------------------------------------------------
// window mean: row (b * k + i) = (sum of the nW ring rows that end at hop j = *clock / hop + i, oldest first) / window,
// zeros where no window has filled yet (j < nW - 1).  With `logits`, also mean @ w2 + b2 in srwn_pooled_head's arithmetic.
// One workgroup per row.
// ------------------------------------------------------------------------------------------
// SLOTS: j from the slot's own time; the row is zero too where the hop lies beyond ran(u) (an idle slot's rows).
template <bool SLOTS = false>
__global__ __launch_bounds__(256) void window_mean_kernel(const float* __restrict__ ring, int ring_rows,
                                                          float* __restrict__ mean, typename ClockArg<SLOTS>::in clock,
                                                          int k, int hop, int nW, float window, int S,
                                                          const float* __restrict__ w2, const float* __restrict__ b2,
                                                          float* __restrict__ logits, int C, int ldw) {
  __shared__ float m[256];
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
  for (int s = threadIdx.x; s < S; s += 256) {
    float acc = 0.0f;
    if (due && j >= nW - 1)
      for (int w = 0; w < nW; ++w) acc += rb[(int64_t)((j - nW + 1 + w) % ring_rows) * S + s];
    acc = acc / window;
    m[s] = acc;
    mean[(int64_t)blockIdx.x * S + s] = acc;
  }
  if (!logits) return;
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float acc = b2[c];
    for (int s = 0; s < S; ++s) acc = fmaf(m[s], w2[(int64_t)s * ldw + c], acc);
    logits[(int64_t)blockIdx.x * C + c] = acc;
  }
}

// ------------------------------------------------------------------------------------------
// roll.  Blocks [0, nroll * B): one per (boundary buffer, stream), rows [n, n + hist) move to [0, hist) -- for n < hist the
// ranges overlap: the block walks them front to back, each step reading all of its rows before it writes any (a barrier
// between), and a row written in one step lies in front of every row a later step reads (srwn_flow_stream_out's roll).
// The last block: carry[b] = x[b][n - 1] and *clock += n (nothing in this launch reads either).
// ------------------------------------------------------------------------------------------
// SLOTS: `clock` is the pool's table, the grid has no last block, and slot b rolls by its own ran(b) rows (none: no roll).
template <bool SLOTS> using RollClock = typename std::conditional<SLOTS, const SrwnSynthSlot*, long long*>::type;

template <typename T, int R, bool SLOTS = false>
__global__ __launch_bounds__(256) void recog_roll_kernel(const RollEntry* __restrict__ roll, int nroll,
                                                         const float* __restrict__ x, int64_t x_stride,
                                                         float* __restrict__ carry, RollClock<SLOTS> clock, int B, int n) {
  if constexpr (SLOTS) {      // (workgroup-uniform, before the first barrier)
    const SrwnSynthSlot sl = clock[(int)blockIdx.x % B];
    n = sl.t < 0 ? 0 : slot_rows(sl, n);
    if (n <= 0) return;
  } else if ((int)blockIdx.x == nroll * B) {
    for (int b = threadIdx.x; b < B; b += 256) carry[b] = x[(int64_t)b * x_stride + n - 1];
    if (threadIdx.x == 0) *clock = *clock + n;
    return;
  }
  constexpr int PPR = R * (int)sizeof(T) / 16, RPB = 256 / PPR, U = 4;
  const int kk = (int)blockIdx.x / B, b = (int)blockIdx.x % B;
  const RollEntry e = roll[kk];
  const int hist = (int)e.hist;
  f32x4* base = reinterpret_cast<f32x4*>(reinterpret_cast<T*>(e.buf) + (size_t)b * (size_t)e.clip_rows * R);
  const int piece = threadIdx.x % PPR, rloc = threadIdx.x / PPR;
  for (int i0 = 0; i0 < hist; i0 += RPB * U) {
    f32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * RPB + rloc;
      if (i < hist) v[u] = base[(size_t)(i + n) * PPR + piece];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * RPB + rloc;
      if (i < hist) base[(size_t)i * PPR + piece] = v[u];
    }
    __syncthreads();
  }
}


// ------------------------------------------------------------------------------------------
// The host bodies: one per pair of entry points.  `who` names the entry point in every message; SLOTS says which form it
// is, and the clock form's B is then the pool's capacity (named so in the messages: rows_name).
// ------------------------------------------------------------------------------------------
// x: the chunk's audio with its carry, or (SLOTS) the pool's audio ring of x_stride samples per slot, without one
template <bool SLOTS> constexpr const char* rows_name() { return SLOTS ? "capacity" : "B"; }

template <bool SLOTS>
int recog_stream_in_impl(const char* who, const float* x, int64_t x_stride, const float* carry, const float* init_w,
                         const float* init_b, void* out, int64_t out_clip_rows, int32_t out_hist, int32_t B, int32_t n,
                         int32_t max_chunk, int32_t R, int32_t dtype, const SrwnSynthSlot* slots, void* stream) {
  if (!x || !init_w || !init_b || !out || (SLOTS ? !slots : !carry)) return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if (R != 32 && R != 64) return set_error(SRWN_E_UNSUPPORTED, "%s: dilation_channels %d (built: 32, 64)", who, R);
  if (B < 1 || max_chunk < 1 || out_hist < 0)
    return set_error(SRWN_E_SHAPE, "%s: %s=%d max_chunk=%d out_hist=%d", who, rows_name<SLOTS>(), B, max_chunk, out_hist);
  if (n < 1 || n > max_chunk) return set_error(SRWN_E_SHAPE, "%s: chunk of %d rows (1..max_chunk = %d)", who, n, max_chunk);
  // (the ring also holds the sample before a whole chunk)
  if (x_stride < (int64_t)max_chunk + (SLOTS ? 1 : 0) || out_clip_rows < (int64_t)out_hist + max_chunk) {
    if (SLOTS)
      return set_error(SRWN_E_SHAPE, "%s: an audio ring of %d samples for max_chunk + 1 = %lld, %lld buffer rows per slot for %d + %d",
                       who, (int)x_stride, (long long)max_chunk + 1, (long long)out_clip_rows, out_hist, max_chunk);
    return set_error(SRWN_E_SHAPE, "%s: x stride %lld, %lld buffer rows per stream for %d + %d", who, (long long)x_stride,
                     (long long)out_clip_rows, out_hist, max_chunk);
  }
  const int64_t threads = (int64_t)B * n * (R / 8);
  dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SRWN_BF16)
    hipLaunchKernelGGL((recog_stream_in_kernel<bf16_t, SLOTS>), grid, block, 0, st, x, x_stride, carry, init_w, init_b,
                       (bf16_t*)out, out_clip_rows, out_hist, B, n, R, slots);
  else if (dtype == SRWN_F32)
    hipLaunchKernelGGL((recog_stream_in_kernel<float, SLOTS>), grid, block, 0, st, x, x_stride, carry, init_w, init_b,
                       (float*)out, out_clip_rows, out_hist, B, n, R, slots);
  else
    return set_error(SRWN_E_DTYPE, "%s: dtype %d", who, dtype);
  return check_launch(who);
}

int hop_args(const char* who, int32_t ring_rows, int32_t B, int32_t k, int32_t hop, int32_t max_chunk, int64_t clip_rows) {
  if (B < 1 || k < 1 || hop < 1 || ring_rows < 1 || max_chunk < 1)
    return set_error(SRWN_E_SHAPE, "%s: B=%d hops=%d hop=%d ring=%d max_chunk=%d", who, B, k, hop, ring_rows, max_chunk);
  if ((int64_t)k * hop > max_chunk || clip_rows < max_chunk)
    return set_error(SRWN_E_SHAPE, "%s: %d hops of %d rows in buffers of %lld rows per stream (max_chunk = %d)", who, k, hop,
                     (long long)clip_rows, max_chunk);
  if ((int64_t)B * k > 0x7fffffffLL) return set_error(SRWN_E_SHAPE, "%s: too many hops", who);
  return 0;
}

template <bool SLOTS>
int pooled_stream_head_impl(const char* who, const void* z, int64_t z_layer_stride, int64_t z_clip_rows, int32_t nlayers,
                            const void* wskip, const float* bs_sum, const void* w1, const float* b1, float* ring,
                            int32_t ring_rows, typename ClockArg<SLOTS>::in clock, int32_t B, int32_t k, int32_t hop,
                            int32_t max_chunk, int32_t R, int32_t S, int32_t dtype, void* stream) {
  if (!z || !wskip || !bs_sum || !w1 || !b1 || !ring || !clock) return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if ((R != 32 && R != 64) || (S != 128 && S != 256))
    return set_error(SRWN_E_UNSUPPORTED, "%s: dilation_channels %d, skip_channels %d (built: 32 / 64 x 128 / 256)", who, R, S);
  if (const int rc = hop_args(who, ring_rows, B, k, hop, max_chunk, z_clip_rows)) return rc;
  if (nlayers < 1 || z_layer_stride < (int64_t)B * z_clip_rows * R)
    return set_error(SRWN_E_SHAPE, "%s: %d layers at a stride of %lld", who, nlayers, (long long)z_layer_stride);
  dim3 grid((unsigned)(B * k)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define SRWN_PSH(TT, RR, SS)                                                                                             \
  hipLaunchKernelGGL((pooled_stream_head_kernel<TT, RR, SS, SLOTS>), grid, block, 0, st, (const TT*)z, z_layer_stride,    \
                     z_clip_rows, nlayers, (const TT*)wskip, bs_sum, (const TT*)w1, b1, ring, ring_rows, clock, k, hop)
#define SRWN_PSH_T(TT)                                       \
  {                                                          \
    if (R == 32 && S == 128) SRWN_PSH(TT, 32, 128);          \
    else if (R == 32) SRWN_PSH(TT, 32, 256);                 \
    else if (S == 128) SRWN_PSH(TT, 64, 128);                \
    else SRWN_PSH(TT, 64, 256);                              \
  }
  if (dtype == SRWN_BF16) SRWN_PSH_T(bf16_t)
  else if (dtype == SRWN_F32) SRWN_PSH_T(float)
  else return set_error(SRWN_E_DTYPE, "%s: dtype %d", who, dtype);
#undef SRWN_PSH_T
#undef SRWN_PSH
  return check_launch(who);
}

template <bool SLOTS>
int hop_sum_impl(const char* who, const void* r1, int64_t r1_clip_rows, float* ring, int32_t ring_rows,
                 typename ClockArg<SLOTS>::in clock, int32_t B, int32_t k, int32_t hop, int32_t max_chunk, int32_t S,
                 int32_t dtype, void* stream) {
  if (!r1 || !ring || !clock) return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if (const int rc = hop_args(who, ring_rows, B, k, hop, max_chunk, r1_clip_rows)) return rc;
  if (S < 2 || S % 2) return set_error(SRWN_E_SHAPE, "%s: S=%d", who, S);
  dim3 grid((unsigned)(B * k)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SRWN_BF16)
    hipLaunchKernelGGL((hop_sum_kernel<bf16_t, SLOTS>), grid, block, 0, st, (const bf16_t*)r1, r1_clip_rows, ring, ring_rows, clock, k, hop, S);
  else if (dtype == SRWN_F32)
    hipLaunchKernelGGL((hop_sum_kernel<float, SLOTS>), grid, block, 0, st, (const float*)r1, r1_clip_rows, ring, ring_rows, clock, k, hop, S);
  else
    return set_error(SRWN_E_DTYPE, "%s: dtype %d", who, dtype);
  return check_launch(who);
}

template <bool SLOTS>
int window_mean_impl(const char* who, const float* ring, int32_t ring_rows, float* mean, typename ClockArg<SLOTS>::in clock,
                     int32_t B, int32_t k, int32_t hop, int32_t window, int32_t S, const float* w2, const float* b2,
                     float* logits, int32_t C, int32_t ldw, void* stream) {
  if (!ring || !mean || !clock || (logits && (!w2 || !b2))) return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if (B < 1 || k < 1 || hop < 1 || window < hop || window % hop || S < 1 || S > 256)
    return set_error(SRWN_E_SHAPE, "%s: %s=%d hops=%d hop=%d window=%d S=%d (window a multiple of hop, S <= 256)", who,
                     rows_name<SLOTS>(), B, k, hop, window, S);
  const int nW = window / hop;
  if (ring_rows < nW + k - 1)
    return set_error(SRWN_E_SHAPE, "%s: a ring of %d rows for %d window rows + %d hops per launch - 1", who, ring_rows, nW, k);
  if (logits && (C < 1 || ldw < C)) return set_error(SRWN_E_SHAPE, "%s: C=%d ldw=%d", who, C, ldw);
  // (SLOTS: the kernel counts a slot's rows in a chunk of k * hop in int32)
  if ((int64_t)B * k > 0x7fffffffLL || (SLOTS && (int64_t)k * hop > 0x7fffffffLL))
    return set_error(SRWN_E_SHAPE, "%s: too many rows", who);
  hipLaunchKernelGGL(window_mean_kernel<SLOTS>, dim3((unsigned)(B * k)), dim3(256), 0, (hipStream_t)stream, ring, ring_rows,
                     mean, clock, k, hop, nW, (float)window, S, w2, b2, logits, C, ldw);
  return check_launch(who);
}

// Clock form: x, carry and the clock are renewed by one extra block at the grid's end.  SLOTS: the table in the clock's
// place, no x and no carry, no last block -- and without boundary buffers no launch at all.
template <bool SLOTS>
int recog_roll_impl(const char* who, const int64_t* roll_table, int32_t nroll, const float* x, int64_t x_stride, float* carry,
                    RollClock<SLOTS> clock, int32_t B, int32_t n, int32_t max_chunk, int32_t R, int32_t dtype, void* stream) {
  if (!clock || (nroll > 0 && !roll_table) || (!SLOTS && (!x || !carry))) return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if (R != 32 && R != 64) return set_error(SRWN_E_UNSUPPORTED, "%s: dilation_channels %d (built: 32, 64)", who, R);
  if (B < 1 || nroll < 0 || max_chunk < 1 || (!SLOTS && x_stride < max_chunk)) {
    if (SLOTS) return set_error(SRWN_E_SHAPE, "%s: capacity=%d boundaries=%d max_chunk=%d", who, B, nroll, max_chunk);
    return set_error(SRWN_E_SHAPE, "%s: B=%d boundaries=%d max_chunk=%d x stride %lld", who, B, nroll, max_chunk, (long long)x_stride);
  }
  if (n < 1 || n > max_chunk) return set_error(SRWN_E_SHAPE, "%s: chunk of %d rows (1..max_chunk = %d)", who, n, max_chunk);
  if (SLOTS && nroll == 0) return 0;
  dim3 grid((unsigned)((int64_t)nroll * B + (SLOTS ? 0 : 1))), block(256);
  hipStream_t st = (hipStream_t)stream;
  const RollEntry* rt = reinterpret_cast<const RollEntry*>(roll_table);
#define SRWN_RR(TT, RR) hipLaunchKernelGGL((recog_roll_kernel<TT, RR, SLOTS>), grid, block, 0, st, rt, nroll, x, x_stride, carry, clock, B, n)
  if (dtype == SRWN_BF16) { if (R == 32) SRWN_RR(bf16_t, 32); else SRWN_RR(bf16_t, 64); }
  else if (dtype == SRWN_F32) { if (R == 32) SRWN_RR(float, 32); else SRWN_RR(float, 64); }
  else return set_error(SRWN_E_DTYPE, "%s: dtype %d", who, dtype);
#undef SRWN_RR
  return check_launch(who);
}

const long long* ck(const int64_t* clock) { return reinterpret_cast<const long long*>(clock); }

}  // namespace

// ------------------------------------------------------------------------------------------
// The entry points (srwn.h): each names itself and says which form it is.
// ------------------------------------------------------------------------------------------
extern "C" int srwn_recog_stream_in(const float* x, int64_t x_stride, const float* carry, const float* init_w,
                                    const float* init_b, void* out, int64_t out_clip_rows, int32_t out_hist, int32_t B,
                                    int32_t n, int32_t max_chunk, int32_t R, int32_t dtype, void* stream) {
  return recog_stream_in_impl<false>("recog_stream_in", x, x_stride, carry, init_w, init_b, out, out_clip_rows, out_hist, B, n,
                                     max_chunk, R, dtype, nullptr, stream);
}

extern "C" int srwn_recog_stream_in_slots(const float* audio_ring, int32_t ring_len, const float* init_w,
                                          const float* init_b, void* out, int64_t out_clip_rows, int32_t out_hist,
                                          int32_t capacity, int32_t n, int32_t max_chunk, int32_t R, int32_t dtype,
                                          const SrwnSynthSlot* slots, void* stream) {
  return recog_stream_in_impl<true>("recog_stream_in_slots", audio_ring, ring_len, nullptr, init_w, init_b, out, out_clip_rows,
                                    out_hist, capacity, n, max_chunk, R, dtype, slots, stream);
}

extern "C" int srwn_pooled_stream_head(const void* z, int64_t z_layer_stride, int64_t z_clip_rows, int32_t nlayers,
                                       const void* wskip, const float* bs_sum, const void* w1, const float* b1,
                                       float* ring, int32_t ring_rows, const int64_t* clock, int32_t B, int32_t k,
                                       int32_t hop, int32_t max_chunk, int32_t R, int32_t S, int32_t dtype, void* stream) {
  return pooled_stream_head_impl<false>("pooled_stream_head", z, z_layer_stride, z_clip_rows, nlayers, wskip, bs_sum, w1, b1,
                                        ring, ring_rows, ck(clock), B, k, hop, max_chunk, R, S, dtype, stream);
}

extern "C" int srwn_pooled_stream_head_slots(const void* z, int64_t z_layer_stride, int64_t z_clip_rows, int32_t nlayers,
                                             const void* wskip, const float* bs_sum, const void* w1, const float* b1,
                                             float* ring, int32_t ring_rows, const SrwnSynthSlot* slots, int32_t capacity,
                                             int32_t k, int32_t hop, int32_t max_chunk, int32_t R, int32_t S, int32_t dtype,
                                             void* stream) {
  return pooled_stream_head_impl<true>("pooled_stream_head_slots", z, z_layer_stride, z_clip_rows, nlayers, wskip, bs_sum, w1,
                                       b1, ring, ring_rows, slots, capacity, k, hop, max_chunk, R, S, dtype, stream);
}

extern "C" int srwn_hop_sum(const void* r1, int64_t r1_clip_rows, float* ring, int32_t ring_rows, const int64_t* clock,
                            int32_t B, int32_t k, int32_t hop, int32_t max_chunk, int32_t S, int32_t dtype, void* stream) {
  return hop_sum_impl<false>("hop_sum", r1, r1_clip_rows, ring, ring_rows, ck(clock), B, k, hop, max_chunk, S, dtype, stream);
}

extern "C" int srwn_hop_sum_slots(const void* r1, int64_t r1_clip_rows, float* ring, int32_t ring_rows,
                                  const SrwnSynthSlot* slots, int32_t capacity, int32_t k, int32_t hop, int32_t max_chunk,
                                  int32_t S, int32_t dtype, void* stream) {
  return hop_sum_impl<true>("hop_sum_slots", r1, r1_clip_rows, ring, ring_rows, slots, capacity, k, hop, max_chunk, S, dtype,
                            stream);
}

extern "C" int srwn_window_mean(const float* ring, int32_t ring_rows, float* mean, const int64_t* clock, int32_t B,
                                int32_t k, int32_t hop, int32_t window, int32_t S, const float* w2, const float* b2,
                                float* logits, int32_t C, int32_t ldw, void* stream) {
  return window_mean_impl<false>("window_mean", ring, ring_rows, mean, ck(clock), B, k, hop, window, S, w2, b2, logits, C, ldw,
                                 stream);
}

extern "C" int srwn_window_mean_slots(const float* ring, int32_t ring_rows, float* mean, const SrwnSynthSlot* slots,
                                      int32_t capacity, int32_t k, int32_t hop, int32_t window, int32_t S, const float* w2,
                                      const float* b2, float* logits, int32_t C, int32_t ldw, void* stream) {
  return window_mean_impl<true>("window_mean_slots", ring, ring_rows, mean, slots, capacity, k, hop, window, S, w2, b2, logits,
                                C, ldw, stream);
}

extern "C" int srwn_recog_roll(const int64_t* roll_table, int32_t nroll, const float* x, int64_t x_stride, float* carry,
                               int64_t* clock, int32_t B, int32_t n, int32_t max_chunk, int32_t R, int32_t dtype,
                               void* stream) {
  return recog_roll_impl<false>("recog_roll", roll_table, nroll, x, x_stride, carry, reinterpret_cast<long long*>(clock), B, n,
                                max_chunk, R, dtype, stream);
}

extern "C" int srwn_recog_roll_slots(const int64_t* roll_table, int32_t nroll, const SrwnSynthSlot* slots, int32_t capacity,
                                     int32_t n, int32_t max_chunk, int32_t R, int32_t dtype, void* stream) {
  return recog_roll_impl<true>("recog_roll_slots", roll_table, nroll, nullptr, 0, nullptr, slots, capacity, n, max_chunk, R,
                               dtype, stream);
}
