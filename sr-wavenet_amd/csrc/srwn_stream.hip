// Chunked synthesis with the Parallel-WaveNet student (model.py:415-535 as an inference-only stream): what a flow does
// around its layer groups (csrc/srwn_group.hip, srwn_residual_group_fwd_stream), one small launch each, and the noise
// the first flow reads.  gfx950 (MI355X) only.
//   flow entry  RightShift + input conv from the two carried samples + the first layer's conditioning bias by absolute
//               time, written behind the history rows of the flow's first boundary buffer
//   flow exit   relu -> 1x1 R->2 -> x * exp(p0) + p1 (+ the clamp after the last flow), the carry of the flow's input,
//               the history roll of every boundary buffer of the flow, and (last flow) the clock
//   noise       temperature[b] * (log u - log(1 - u)), u the counter-based uniform of (seed[b], absolute sample index)
//   slot forms  the three above for a synthesis pool (every stream at a clock of its own, srwn.h SrwnSynthSlot), and the
//               reset a join runs on its slots
// Every value of a row depends on absolute time only, so a stream has the same bits in any chunking, at any batch size
// and in any row of the batch; the arithmetic is that of causal_conv_cin1_kernel + add_frame_bias_kernel and of
// flow_affine_fwd_kernel + clamp_kernel, which the training engine runs on whole clips.
#include <cmath>
#include <type_traits>
#include "srwn_common.h"
#include "srwn_flow_in.h"
#include "srwn_host.h"
#include "srwn_slots.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

// The slot forms (synthesis pools, srwn.h SrwnSynthSlot) are the same kernels with a template flag: the clock argument
// becomes the pool's table, slot b's chunk starts at slots[b].t and has ran = slot_rows(slots[b], n) rows (ClockArg,
// slot_rows and the roll's RollEntry: srwn_slots.h).  The clock instantiations keep their arguments and their code.

// ------------------------------------------------------------------------------------------
// flow entry: 8 channels per thread, one row per group of R/8 lanes
//   v = b; v = fma(x[t-2], w[0], v); v = fma(x[t-1], w[1], v); round to T        (srwn_causal_conv1d_fwd, shift 1)
//   out = round to T ((float)v + cond[b, t_abs / pool])                          (srwn_add_frame_bias)
// x[-1], x[-2] of the chunk are the carry (zeros at the stream's start: the conv's zero padding).
// ------------------------------------------------------------------------------------------
template <typename T, bool SLOTS = false>
__global__ __launch_bounds__(256) void flow_stream_in_kernel(const float* __restrict__ x, int64_t x_stride,
                                                             const float* __restrict__ carry,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             const T* __restrict__ cond, int cond_frames, int pool,
                                                             int64_t cond_stride, T* __restrict__ out,
                                                             int64_t out_clip_rows, int hist, int B, int n, int R,
                                                             typename ClockArg<SLOTS>::in __restrict__ clock) {
  const int lpr = R / 8;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = idx / lpr;
  const int sub = (int)(idx % lpr);
  if (row >= (int64_t)B * n) return;
  const int b = (int)(row / n);
  const int t = (int)(row - (int64_t)b * n);
  long long t0;
  if constexpr (SLOTS) {
    const SrwnSynthSlot s = clock[b];
    if (t >= slot_rows(s, n)) return;
    t0 = s.t;
  } else {
    t0 = *clock;
  }
  const float* xb = x + (int64_t)b * x_stride;
  const float x1 = t >= 1 ? xb[t - 1] : carry[2 * b];
  const float x0 = t >= 2 ? xb[t - 2] : carry[2 * b + (1 - t)];      // t = 1: x[-1] = carry[0]; t = 0: x[-2] = carry[1]
  // (the arithmetic, and the frame's row of the conditioning ring: flow_entry_row, shared with the scorer pool's entry)
  flow_entry_row<T>(x0, x1, w, bias, cond, cond_frames, pool, cond_stride, b, t0 + t,
                    out, (int64_t)b * out_clip_rows + hist + t, R, sub);
}

// ------------------------------------------------------------------------------------------
// flow exit.  Blocks [0, naff): the head and the affine transform in flow_affine_fwd_kernel's arithmetic, rows of the
// flow's top buffer [B][top_clip_rows][R]; the thread of a stream's last row also renews the carry of the flow's input.
// Blocks [naff, naff + nroll * B): the history roll, one block per (boundary buffer, stream): rows [n, n + hist) move to
// [0, hist) (slot form: rows [ran, ran + hist)).  For n < hist the ranges overlap: the block walks them front to back, each step reading all of its rows
// before it writes any (a barrier between), and a row written in one step lies in front of every row a later step reads.
// ------------------------------------------------------------------------------------------
// (SLOTS) slots[b].t += ran(b) for the live slots.  Every workgroup of the exit launch reads the table, so the one that
// arrives LAST -- after all of them have read -- does the writing: each counts itself in once it is done, the one that
// finds every other counted puts the counter back to zero for the next launch and advances the table, one thread per
// slot, ordinary stores.  Called by all threads of every workgroup, at its end.
__device__ __forceinline__ void slots_advance(SrwnSynthSlot* slots, int* arrive, int B, int n, int advance) {
  if (!advance) return;
  __shared__ int last;
  __syncthreads();                        // all of this workgroup's reads of the table are done
  if (threadIdx.x == 0) {
    __threadfence();
    last = atomicAdd(arrive, 1) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  if (threadIdx.x == 0) *arrive = 0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const SrwnSynthSlot s = slots[b];
    if (s.t < s.t_end) slots[b].t = s.t + slot_rows(s, n);
  }
}

template <typename T, int R, bool SLOTS = false>
__global__ __launch_bounds__(256) void flow_stream_out_kernel(const T* __restrict__ h, int64_t top_clip_rows,
                                                              const float* __restrict__ w2, const float* __restrict__ b2,
                                                              const float* __restrict__ x_in, float* __restrict__ x_out,
                                                              int64_t x_stride, float* __restrict__ carry, int clamp,
                                                              const RollEntry* __restrict__ roll, int naff, int B, int n,
                                                              typename ClockArg<SLOTS>::out clock, int advance) {
  constexpr int LPR = R / 8, RPI = 256 / LPR;
  if ((int)blockIdx.x >= naff) {
    constexpr int PPR = R * (int)sizeof(T) / 16, RPB = 256 / PPR, U = 4;
    const int k = ((int)blockIdx.x - naff) / B, b = ((int)blockIdx.x - naff) % B;
    const RollEntry e = roll[k];
    int hist = (int)e.hist;
    int nsh = n;
    if constexpr (SLOTS) {      // a slot whose chunk was cut short moves by the rows it ran: a live stream goes on from there
      nsh = slot_rows(clock.slots[b], n);
      if (nsh == 0) hist = 0;                               // a slot without rows in this chunk keeps its buffers as they are
    }
    f32x4* base = reinterpret_cast<f32x4*>(reinterpret_cast<T*>(e.buf) + (size_t)b * (size_t)e.clip_rows * R);
    const int piece = threadIdx.x % PPR, rloc = threadIdx.x / PPR;
    for (int i0 = 0; i0 < hist; i0 += RPB * U) {
      f32x4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * RPB + rloc;
        if (i < hist) v[u] = base[(size_t)(i + nsh) * PPR + piece];
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * RPB + rloc;
        if (i < hist) base[(size_t)i * PPR + piece] = v[u];
      }
      __syncthreads();
    }
    if constexpr (SLOTS) slots_advance(clock.slots, clock.arrive, B, n, advance);
    return;
  }
  const int sub = threadIdx.x % LPR, rloc = threadIdx.x / LPR;
  float w0[8], w1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { w0[j] = w2[(8 * sub + j) * 2]; w1[j] = w2[(8 * sub + j) * 2 + 1]; }
  const float b0 = b2[0], b1 = b2[1];
  const int64_t rows = (int64_t)B * n;
  const int64_t base = (int64_t)blockIdx.x * 256;
#pragma unroll 2
  for (int it = 0; it < 256 / RPI; ++it) {
    const int64_t row = base + it * RPI + rloc;
    const bool ok = row < rows;
    const int bb = ok ? (int)(row / n) : 0;
    const int t = ok ? (int)(row - (int64_t)bb * n) : 0;
    float v[8];
    Row8s<T>::load(h + ((int64_t)bb * top_clip_rows + t) * R + 8 * sub, v);
    float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a = fmaxf(v[j], 0.0f);
      p0 = fmaf(a, w0[j], p0);
      p1 = fmaf(a, w1[j], p1);
    }
#pragma unroll
    for (int s = 1; s < LPR; s <<= 1) { p0 += __shfl_xor(p0, s, 64); p1 += __shfl_xor(p1, s, 64); }
    p0 += b0;
    p1 += b1;
    if (ok && sub == 0) {
      const float* xi = x_in + (int64_t)bb * x_stride;
      if constexpr (SLOTS) {
        const int ran = slot_rows(clock.slots[bb], n);
        if (t < ran) {
          float y = fmaf(xi[t], expf(p0), p1);
          if (clamp) y = fminf(fmaxf(y, -1.0f), 1.0f);
          x_out[(int64_t)bb * x_stride + t] = y;
          if (t == ran - 1) {
            const float c1 = ran >= 2 ? xi[ran - 2] : carry[2 * bb];
            carry[2 * bb] = xi[ran - 1];
            carry[2 * bb + 1] = c1;
          }
        } else {
          x_out[(int64_t)bb * x_stride + t] = 0.0f;      // past the stream's end, and every entry of a free slot
        }
      } else {
      float y = fmaf(xi[t], expf(p0), p1);
      if (clamp) y = fminf(fmaxf(y, -1.0f), 1.0f);                // model.py:535
      x_out[(int64_t)bb * x_stride + t] = y;
      if (t == n - 1) {      // the two samples the next chunk's input conv reads behind its first row
        const float c1 = n >= 2 ? xi[n - 2] : carry[2 * bb];
        carry[2 * bb] = xi[n - 1];
        carry[2 * bb + 1] = c1;
      }
      }
    }
  }
  if constexpr (SLOTS) slots_advance(clock.slots, clock.arrive, B, n, advance);
  else if (advance && blockIdx.x == 0 && threadIdx.x == 0) *clock = *clock + n;      // (nothing in this launch reads the clock)
}

// ------------------------------------------------------------------------------------------
// logistic noise.  The counter's bits: splitmix64 of (seed, index), as uniform01 of csrc/srwn_ops.hip mixes them; the top
// 23 bits k give u = (k + 1/2) / 2^23, so that 2^-24 <= u <= 1 - 2^-24 and 1 - u is exact and > 0 in fp32 (uniform01's
// 24 bits + 1/2 round to 1.0f at the top value: log(1 - u) = -inf).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t counter_bits23(uint64_t seed, uint64_t idx) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (idx + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)(z >> 41);
}
// log u - log(1 - u) evaluated as +-log1p(|2u - 1| / min(u, 1 - u)): 2u - 1 and 1 - u are exact, so the draw carries one
// division's and one log1pf's rounding at every u.  (The difference of two logf cancels near u = 1/2: a draw of 2e-6 would
// carry the 6e-8 of each logarithm, 3 % of itself.)
__device__ __forceinline__ float logistic_of_bits23(uint32_t k) {
  const float u = ((float)(k & 0x7fffffu) + 0.5f) * (1.0f / 8388608.0f);
  const float v = 1.0f - u;
  const float d = u - v;                                   // 2u - 1, exact
  const float l = log1pf(fabsf(d) / fminf(u, v));
  return d < 0.0f ? -l : l;
}

template <bool SLOTS = false>
__global__ __launch_bounds__(256) void logistic_noise_kernel(float* __restrict__ noise, int64_t stride,
                                                             const float* __restrict__ temperature,
                                                             const uint64_t* __restrict__ seed,
                                                             typename ClockArg<SLOTS>::in __restrict__ clock, int B, int n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * n) return;
  const int b = (int)(i / n);
  const int j = (int)(i - (int64_t)b * n);
  long long t0;
  if constexpr (SLOTS) {
    const SrwnSynthSlot s = clock[b];
    if (j >= slot_rows(s, n)) return;
    t0 = s.t;
  } else {
    t0 = *clock;
  }
  const float tmp = temperature[b];
  const float l = logistic_of_bits23(counter_bits23(seed[b], (uint64_t)(t0 + j)));
  noise[(int64_t)b * stride + j] = tmp == 0.0f ? 0.0f : tmp * l;
}

__global__ __launch_bounds__(256) void logistic_from_bits_kernel(const uint32_t* __restrict__ bits, float* __restrict__ out,
                                                                 int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = logistic_of_bits23(bits[i]);
}

// ------------------------------------------------------------------------------------------
// join of a synthesis pool: zero history rows and zero carries for the named slots.  Blocks [0, nroll * nslots): one per
// (boundary buffer, named slot), rows [0, hist); the last block: the carries.
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void flow_stream_reset_kernel(const RollEntry* __restrict__ roll, int nroll,
                                                                float* __restrict__ carry, int ncarry, int64_t carry_stride,
                                                                const int* __restrict__ ids, int nslots, int capacity, int R) {
  const int blk = (int)blockIdx.x;
  if (blk == nroll * nslots) {
    for (int i = threadIdx.x; i < ncarry * nslots; i += 256) {
      const int u = ids[i % nslots];
      if (u < 0 || u >= capacity) continue;
      float* c = carry + (int64_t)(i / nslots) * carry_stride + 2 * u;
      c[0] = 0.0f;
      c[1] = 0.0f;
    }
    return;
  }
  const int u = ids[blk % nslots];
  if (u < 0 || u >= capacity) return;
  const RollEntry e = roll[blk / nslots];
  f32x4* base = reinterpret_cast<f32x4*>(reinterpret_cast<T*>(e.buf) + (size_t)u * (size_t)e.clip_rows * R);
  const long long pieces = e.hist * (long long)(R * (int)sizeof(T) / 16);
  for (long long i = threadIdx.x; i < pieces; i += 256) base[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

// the entry points' two forms: clock != null xor slots != null
int flow_stream_in_impl(const char* who, const float* x, int64_t x_stride, const float* carry, const float* init_w,
                        const float* init_b, const void* cond0, int32_t cond_frames, int32_t pool_stride,
                        int64_t cond_row_stride, void* out, int64_t out_clip_rows, int32_t out_hist, int32_t B, int32_t n,
                        int32_t max_chunk, int32_t R, int32_t dtype, const int64_t* clock, const SrwnSynthSlot* slots,
                        void* stream) {
  if (!x || !carry || !init_w || !init_b || !cond0 || !out || (!clock && !slots))
    return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if (R != 32 && R != 64) return set_error(SRWN_E_UNSUPPORTED, "%s: dilation_channels %d (built: 32, 64)", who, R);
  if (B < 1 || max_chunk < 1 || out_hist < 0 || cond_frames < 1 || pool_stride < 1 || cond_row_stride < R || cond_row_stride % 8)
    return set_error(SRWN_E_SHAPE, "%s: B=%d max_chunk=%d out_hist=%d frames=%d pool=%d cond stride %lld", who, B,
                     max_chunk, out_hist, cond_frames, pool_stride, (long long)cond_row_stride);
  if (n < 1 || n > max_chunk) return set_error(SRWN_E_SHAPE, "%s: chunk of %d rows (1..max_chunk = %d)", who, n, max_chunk);
  if (x_stride < max_chunk || out_clip_rows < (int64_t)out_hist + max_chunk)
    return set_error(SRWN_E_SHAPE, "%s: x stride %lld, %lld buffer rows per stream for %d + %d", who, (long long)x_stride,
                     (long long)out_clip_rows, out_hist, max_chunk);
  const int64_t threads = (int64_t)B * n * (R / 8);
  dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const long long* ck = reinterpret_cast<const long long*>(clock);
#define SRWN_FSI(TT)                                                                                                     \
  {                                                                                                                      \
    if (slots)                                                                                                           \
      hipLaunchKernelGGL((flow_stream_in_kernel<TT, true>), grid, block, 0, st, x, x_stride, carry, init_w, init_b,       \
                         (const TT*)cond0, cond_frames, pool_stride, cond_row_stride, (TT*)out, out_clip_rows, out_hist, B, \
                         n, R, slots);                                                                                   \
    else                                                                                                                 \
      hipLaunchKernelGGL((flow_stream_in_kernel<TT, false>), grid, block, 0, st, x, x_stride, carry, init_w, init_b,      \
                         (const TT*)cond0, cond_frames, pool_stride, cond_row_stride, (TT*)out, out_clip_rows, out_hist, B, \
                         n, R, ck);                                                                                      \
  }
  if (dtype == SRWN_BF16) SRWN_FSI(bf16_t)
  else if (dtype == SRWN_F32) SRWN_FSI(float)
  else return set_error(SRWN_E_DTYPE, "%s: dtype %d", who, dtype);
#undef SRWN_FSI
  return check_launch(who);
}

int flow_stream_out_impl(const char* who, const void* h, int64_t top_clip_rows, const float* flow_w, const float* flow_b,
                         const float* x_in, float* x_out, int64_t x_stride, float* carry, int32_t clamp,
                         const int64_t* roll_table, int32_t nroll, int32_t B, int32_t n, int32_t max_chunk, int32_t R,
                         int32_t dtype, int64_t* clock, SrwnSynthSlot* slots, int32_t* arrive, bool slot_form,
                         int32_t advance_clock, void* stream) {
  if (!h || !flow_w || !flow_b || !x_in || !x_out || !carry || (nroll > 0 && !roll_table))
    return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if (slot_form ? (!slots || (advance_clock && !arrive)) : (advance_clock && !clock))
    return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if (R != 32 && R != 64) return set_error(SRWN_E_UNSUPPORTED, "%s: dilation_channels %d (built: 32, 64)", who, R);
  if (B < 1 || max_chunk < 1 || nroll < 0)
    return set_error(SRWN_E_SHAPE, "%s: B=%d max_chunk=%d boundaries=%d", who, B, max_chunk, nroll);
  if (n < 1 || n > max_chunk) return set_error(SRWN_E_SHAPE, "%s: chunk of %d rows (1..max_chunk = %d)", who, n, max_chunk);
  if (x_stride < max_chunk || top_clip_rows < max_chunk)
    return set_error(SRWN_E_SHAPE, "%s: x stride %lld, top rows %lld < max_chunk %d", who, (long long)x_stride,
                     (long long)top_clip_rows, max_chunk);
  const int naff = (int)(((int64_t)B * n + 255) / 256);
  dim3 grid((unsigned)(naff + (int64_t)nroll * B)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const RollEntry* rt = reinterpret_cast<const RollEntry*>(roll_table);
  long long* ck = reinterpret_cast<long long*>(clock);
  const ClockArg<true>::out sk{slots, arrive};
#define SRWN_FSO(TT, RR)                                                                                                  \
  {                                                                                                                       \
    if (slot_form)                                                                                                        \
      hipLaunchKernelGGL((flow_stream_out_kernel<TT, RR, true>), grid, block, 0, st, (const TT*)h, top_clip_rows, flow_w,  \
                         flow_b, x_in, x_out, x_stride, carry, clamp ? 1 : 0, rt, naff, B, n, sk, advance_clock ? 1 : 0); \
    else                                                                                                                  \
      hipLaunchKernelGGL((flow_stream_out_kernel<TT, RR, false>), grid, block, 0, st, (const TT*)h, top_clip_rows, flow_w, \
                         flow_b, x_in, x_out, x_stride, carry, clamp ? 1 : 0, rt, naff, B, n, ck, advance_clock ? 1 : 0); \
  }
  if (dtype == SRWN_BF16) { if (R == 32) SRWN_FSO(bf16_t, 32) else SRWN_FSO(bf16_t, 64) }
  else if (dtype == SRWN_F32) { if (R == 32) SRWN_FSO(float, 32) else SRWN_FSO(float, 64) }
  else return set_error(SRWN_E_DTYPE, "%s: dtype %d", who, dtype);
#undef SRWN_FSO
  return check_launch(who);
}

int logistic_noise_impl(const char* who, float* noise, int64_t noise_stride, const float* temperature, const uint64_t* seed,
                        const int64_t* clock, const SrwnSynthSlot* slots, int32_t B, int32_t n, void* stream) {
  if (!noise || !temperature || !seed || (!clock && !slots)) return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if (B < 1 || n < 1 || noise_stride < n)
    return set_error(SRWN_E_SHAPE, "%s: B=%d n=%d stride=%lld", who, B, n, (long long)noise_stride);
  const int64_t total = (int64_t)B * n;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (slots)
    hipLaunchKernelGGL(logistic_noise_kernel<true>, grid, block, 0, (hipStream_t)stream, noise, noise_stride, temperature, seed,
                       slots, B, n);
  else
    hipLaunchKernelGGL(logistic_noise_kernel<false>, grid, block, 0, (hipStream_t)stream, noise, noise_stride, temperature, seed,
                       reinterpret_cast<const long long*>(clock), B, n);
  return check_launch(who);
}

}  // namespace

extern "C" int srwn_flow_stream_in(const float* x, int64_t x_stride, const float* carry, const float* init_w,
                                   const float* init_b, const void* cond0, int32_t cond_frames, int32_t pool_stride,
                                   int64_t cond_row_stride, void* out, int64_t out_clip_rows, int32_t out_hist, int32_t B,
                                   int32_t n, int32_t max_chunk, int32_t R, int32_t dtype, const int64_t* clock,
                                   void* stream) {
  return flow_stream_in_impl("flow_stream_in", x, x_stride, carry, init_w, init_b, cond0, cond_frames, pool_stride,
                             cond_row_stride, out, out_clip_rows, out_hist, B, n, max_chunk, R, dtype, clock, nullptr, stream);
}

extern "C" int srwn_flow_stream_in_slots(const float* x, int64_t x_stride, const float* carry, const float* init_w,
                                         const float* init_b, const void* cond0, int32_t cond_frames, int32_t pool_stride,
                                         int64_t cond_row_stride, void* out, int64_t out_clip_rows, int32_t out_hist,
                                         int32_t capacity, int32_t n, int32_t max_chunk, int32_t R, int32_t dtype,
                                         const SrwnSynthSlot* slots, void* stream) {
  return flow_stream_in_impl("flow_stream_in_slots", x, x_stride, carry, init_w, init_b, cond0, cond_frames, pool_stride,
                             cond_row_stride, out, out_clip_rows, out_hist, capacity, n, max_chunk, R, dtype, nullptr, slots,
                             stream);
}

extern "C" int srwn_flow_stream_out(const void* h, int64_t top_clip_rows, const float* flow_w, const float* flow_b,
                                    const float* x_in, float* x_out, int64_t x_stride, float* carry, int32_t clamp,
                                    const int64_t* roll_table, int32_t nroll, int32_t B, int32_t n, int32_t max_chunk,
                                    int32_t R, int32_t dtype, int64_t* clock, int32_t advance_clock, void* stream) {
  return flow_stream_out_impl("flow_stream_out", h, top_clip_rows, flow_w, flow_b, x_in, x_out, x_stride, carry, clamp,
                              roll_table, nroll, B, n, max_chunk, R, dtype, clock, nullptr, nullptr, false, advance_clock,
                              stream);
}

extern "C" int srwn_flow_stream_out_slots(const void* h, int64_t top_clip_rows, const float* flow_w, const float* flow_b,
                                          const float* x_in, float* x_out, int64_t x_stride, float* carry, int32_t clamp,
                                          const int64_t* roll_table, int32_t nroll, int32_t capacity, int32_t n,
                                          int32_t max_chunk, int32_t R, int32_t dtype, SrwnSynthSlot* slots, int32_t* arrive,
                                          int32_t advance, void* stream) {
  return flow_stream_out_impl("flow_stream_out_slots", h, top_clip_rows, flow_w, flow_b, x_in, x_out, x_stride, carry, clamp,
                              roll_table, nroll, capacity, n, max_chunk, R, dtype, nullptr, slots, arrive, true, advance,
                              stream);
}

extern "C" int srwn_logistic_noise(float* noise, int64_t noise_stride, const float* temperature, const uint64_t* seed,
                                   const int64_t* clock, int32_t B, int32_t n, void* stream) {
  return logistic_noise_impl("logistic_noise", noise, noise_stride, temperature, seed, clock, nullptr, B, n, stream);
}

extern "C" int srwn_logistic_noise_slots(float* noise, int64_t noise_stride, const float* temperature, const uint64_t* seed,
                                         const SrwnSynthSlot* slots, int32_t capacity, int32_t n, void* stream) {
  return logistic_noise_impl("logistic_noise_slots", noise, noise_stride, temperature, seed, nullptr, slots, capacity, n,
                             stream);
}

extern "C" int srwn_flow_stream_reset_slots(const int64_t* roll_table, int32_t nroll, float* carry, int32_t ncarry,
                                            int64_t carry_stride, const int32_t* slot_ids, int32_t nslots, int32_t capacity,
                                            int32_t R, int32_t dtype, void* stream) {
  if (!slot_ids || (nroll > 0 && !roll_table) || (ncarry > 0 && !carry))
    return set_error(SRWN_E_NULL, "flow_stream_reset_slots: null pointer");
  if (R != 32 && R != 64) return set_error(SRWN_E_UNSUPPORTED, "flow_stream_reset_slots: dilation_channels %d (built: 32, 64)", R);
  if (capacity < 1 || nslots < 1 || nslots > capacity || nroll < 0 || ncarry < 0 || (ncarry > 1 && carry_stride < 2LL * capacity))
    return set_error(SRWN_E_SHAPE, "flow_stream_reset_slots: capacity=%d slots=%d boundaries=%d carries=%d stride %lld", capacity,
                     nslots, nroll, ncarry, (long long)carry_stride);
  const dim3 grid((unsigned)((int64_t)nroll * nslots + 1)), block(256);
  const RollEntry* rt = reinterpret_cast<const RollEntry*>(roll_table);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SRWN_BF16)
    hipLaunchKernelGGL(flow_stream_reset_kernel<bf16_t>, grid, block, 0, st, rt, nroll, carry, ncarry, carry_stride, slot_ids,
                       nslots, capacity, R);
  else if (dtype == SRWN_F32)
    hipLaunchKernelGGL(flow_stream_reset_kernel<float>, grid, block, 0, st, rt, nroll, carry, ncarry, carry_stride, slot_ids,
                       nslots, capacity, R);
  else
    return set_error(SRWN_E_DTYPE, "flow_stream_reset_slots: dtype %d", dtype);
  return check_launch("flow_stream_reset_slots");
}

extern "C" int srwn_logistic_from_bits(const uint32_t* bits, float* out, int64_t n, void* stream) {
  if (n == 0) return 0;
  if (!bits || !out) return set_error(SRWN_E_NULL, "logistic_from_bits: null pointer");
  if (n < 0) return set_error(SRWN_E_SHAPE, "logistic_from_bits: n=%lld", (long long)n);
  hipLaunchKernelGGL(logistic_from_bits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bits, out, n);
  return check_launch("logistic_from_bits");
}
