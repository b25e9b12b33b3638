// Chunked synthesis with the Parallel-WaveNet student (model.py:415-535 as an inference-only stream): what a flow does
// around its layer groups (csrc/srwn_group.hip, srwn_residual_group_fwd_stream), one small launch each, and the noise
// the first flow reads.  gfx950 (MI355X) only.
//   flow entry  RightShift + input conv from the two carried samples + the first layer's conditioning bias by absolute
//               time, written behind the history rows of the flow's first boundary buffer
//   flow exit   relu -> 1x1 R->2 -> x * exp(p0) + p1 (+ the clamp after the last flow), the carry of the flow's input,
//               the history roll of every boundary buffer of the flow, and (last flow) the clock
//   noise       temperature[b] * (log u - log(1 - u)), u the counter-based uniform of (seed[b], absolute sample index)
// Every value of a row depends on absolute time only, so a stream has the same bits in any chunking, at any batch size
// and in any row of the batch; the arithmetic is that of causal_conv_cin1_kernel + add_frame_bias_kernel and of
// flow_affine_fwd_kernel + clamp_kernel, which the training engine runs on whole clips.
#include <cmath>
#include "srwn_common.h"
#include "srwn_host.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

template <typename T> struct Row8s;
template <> struct Row8s<bf16_t> {
  static __device__ __forceinline__ void load(const bf16_t* p, float (&v)[8]) {
    const bf16x8 r = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)r[j];
  }
};
template <> struct Row8s<float> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
  }
};

// ------------------------------------------------------------------------------------------
// flow entry: 8 channels per thread, one row per group of R/8 lanes
//   v = b; v = fma(x[t-2], w[0], v); v = fma(x[t-1], w[1], v); round to T        (srwn_causal_conv1d_fwd, shift 1)
//   out = round to T ((float)v + cond[b, t_abs / pool])                          (srwn_add_frame_bias)
// x[-1], x[-2] of the chunk are the carry (zeros at the stream's start: the conv's zero padding).
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void flow_stream_in_kernel(const float* __restrict__ x, int64_t x_stride,
                                                             const float* __restrict__ carry,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             const T* __restrict__ cond, int cond_frames, int pool,
                                                             int64_t cond_stride, T* __restrict__ out,
                                                             int64_t out_clip_rows, int hist, int B, int n, int R,
                                                             const long long* __restrict__ clock) {
  const int lpr = R / 8;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = idx / lpr;
  const int sub = (int)(idx % lpr);
  if (row >= (int64_t)B * n) return;
  const int b = (int)(row / n);
  const int t = (int)(row - (int64_t)b * n);
  const float* xb = x + (int64_t)b * x_stride;
  const float x1 = t >= 1 ? xb[t - 1] : carry[2 * b];
  const float x0 = t >= 2 ? xb[t - 2] : carry[2 * b + (1 - t)];      // t = 1: x[-1] = carry[0]; t = 0: x[-2] = carry[1]
  const long long tabs = *clock + t;
  long long f = tabs / pool;
  f = f < cond_frames ? f : cond_frames - 1;
  float c[8];
  Row8s<T>::load(cond + ((int64_t)b * cond_frames + f) * cond_stride + 8 * sub, c);
  T* d = out + ((int64_t)b * out_clip_rows + hist + t) * R + 8 * sub;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = bias[8 * sub + j];
    v = fmaf(x0, w[8 * sub + j], v);
    v = fmaf(x1, w[R + 8 * sub + j], v);
    const T vr = (T)v;
    d[j] = (T)((float)vr + c[j]);
  }
}

// ------------------------------------------------------------------------------------------
// flow exit.  Blocks [0, naff): the head and the affine transform in flow_affine_fwd_kernel's arithmetic, rows of the
// flow's top buffer [B][top_clip_rows][R]; the thread of a stream's last row also renews the carry of the flow's input.
// Blocks [naff, naff + nroll * B): the history roll, one block per (boundary buffer, stream): rows [n, n + hist) move to
// [0, hist).  For n < hist the ranges overlap: the block walks them front to back, each step reading all of its rows
// before it writes any (a barrier between), and a row written in one step lies in front of every row a later step reads.
// ------------------------------------------------------------------------------------------
struct RollEntry { void* buf; long long clip_rows; long long hist; };      // int64 triples, as the engine's table holds them

template <typename T, int R>
__global__ __launch_bounds__(256) void flow_stream_out_kernel(const T* __restrict__ h, int64_t top_clip_rows,
                                                              const float* __restrict__ w2, const float* __restrict__ b2,
                                                              const float* __restrict__ x_in, float* __restrict__ x_out,
                                                              int64_t x_stride, float* __restrict__ carry, int clamp,
                                                              const RollEntry* __restrict__ roll, int naff, int B, int n,
                                                              long long* __restrict__ clock, int advance) {
  constexpr int LPR = R / 8, RPI = 256 / LPR;
  if ((int)blockIdx.x >= naff) {
    constexpr int PPR = R * (int)sizeof(T) / 16, RPB = 256 / PPR, U = 4;
    const int k = ((int)blockIdx.x - naff) / B, b = ((int)blockIdx.x - naff) % B;
    const RollEntry e = roll[k];
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
  if (advance && blockIdx.x == 0 && threadIdx.x == 0) *clock = *clock + n;      // (nothing in this launch reads the clock)
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

__global__ __launch_bounds__(256) void logistic_noise_kernel(float* __restrict__ noise, int64_t stride,
                                                             const float* __restrict__ temperature,
                                                             const uint64_t* __restrict__ seed,
                                                             const long long* __restrict__ clock, int B, int n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * n) return;
  const int b = (int)(i / n);
  const int j = (int)(i - (int64_t)b * n);
  const float tmp = temperature[b];
  const float l = logistic_of_bits23(counter_bits23(seed[b], (uint64_t)(*clock + j)));
  noise[(int64_t)b * stride + j] = tmp == 0.0f ? 0.0f : tmp * l;
}

__global__ __launch_bounds__(256) void logistic_from_bits_kernel(const uint32_t* __restrict__ bits, float* __restrict__ out,
                                                                 int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = logistic_of_bits23(bits[i]);
}

}  // namespace

extern "C" int srwn_flow_stream_in(const float* x, int64_t x_stride, const float* carry, const float* init_w,
                                   const float* init_b, const void* cond0, int32_t cond_frames, int32_t pool_stride,
                                   int64_t cond_row_stride, void* out, int64_t out_clip_rows, int32_t out_hist, int32_t B,
                                   int32_t n, int32_t max_chunk, int32_t R, int32_t dtype, const int64_t* clock,
                                   void* stream) {
  if (!x || !carry || !init_w || !init_b || !cond0 || !out || !clock)
    return set_error(SRWN_E_NULL, "flow_stream_in: null pointer");
  if (R != 32 && R != 64) return set_error(SRWN_E_UNSUPPORTED, "flow_stream_in: dilation_channels %d (built: 32, 64)", R);
  if (B < 1 || max_chunk < 1 || out_hist < 0 || cond_frames < 1 || pool_stride < 1 || cond_row_stride < R || cond_row_stride % 8)
    return set_error(SRWN_E_SHAPE, "flow_stream_in: B=%d max_chunk=%d out_hist=%d frames=%d pool=%d cond stride %lld", B,
                     max_chunk, out_hist, cond_frames, pool_stride, (long long)cond_row_stride);
  if (n < 1 || n > max_chunk) return set_error(SRWN_E_SHAPE, "flow_stream_in: chunk of %d rows (1..max_chunk = %d)", n, max_chunk);
  if (x_stride < max_chunk || out_clip_rows < (int64_t)out_hist + max_chunk)
    return set_error(SRWN_E_SHAPE, "flow_stream_in: x stride %lld, %lld buffer rows per stream for %d + %d", (long long)x_stride,
                     (long long)out_clip_rows, out_hist, max_chunk);
  const int64_t threads = (int64_t)B * n * (R / 8);
  dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const long long* ck = reinterpret_cast<const long long*>(clock);
  if (dtype == SRWN_BF16)
    hipLaunchKernelGGL(flow_stream_in_kernel<bf16_t>, grid, block, 0, st, x, x_stride, carry, init_w, init_b, (const bf16_t*)cond0,
                       cond_frames, pool_stride, cond_row_stride, (bf16_t*)out, out_clip_rows, out_hist, B, n, R, ck);
  else if (dtype == SRWN_F32)
    hipLaunchKernelGGL(flow_stream_in_kernel<float>, grid, block, 0, st, x, x_stride, carry, init_w, init_b, (const float*)cond0,
                       cond_frames, pool_stride, cond_row_stride, (float*)out, out_clip_rows, out_hist, B, n, R, ck);
  else
    return set_error(SRWN_E_DTYPE, "flow_stream_in: dtype %d", dtype);
  return check_launch("flow_stream_in");
}

extern "C" int srwn_flow_stream_out(const void* h, int64_t top_clip_rows, const float* flow_w, const float* flow_b,
                                    const float* x_in, float* x_out, int64_t x_stride, float* carry, int32_t clamp,
                                    const int64_t* roll_table, int32_t nroll, int32_t B, int32_t n, int32_t max_chunk,
                                    int32_t R, int32_t dtype, int64_t* clock, int32_t advance_clock, void* stream) {
  if (!h || !flow_w || !flow_b || !x_in || !x_out || !carry || (nroll > 0 && !roll_table) || (advance_clock && !clock))
    return set_error(SRWN_E_NULL, "flow_stream_out: null pointer");
  if (R != 32 && R != 64) return set_error(SRWN_E_UNSUPPORTED, "flow_stream_out: dilation_channels %d (built: 32, 64)", R);
  if (B < 1 || max_chunk < 1 || nroll < 0)
    return set_error(SRWN_E_SHAPE, "flow_stream_out: B=%d max_chunk=%d boundaries=%d", B, max_chunk, nroll);
  if (n < 1 || n > max_chunk) return set_error(SRWN_E_SHAPE, "flow_stream_out: chunk of %d rows (1..max_chunk = %d)", n, max_chunk);
  if (x_stride < max_chunk || top_clip_rows < max_chunk)
    return set_error(SRWN_E_SHAPE, "flow_stream_out: x stride %lld, top rows %lld < max_chunk %d", (long long)x_stride,
                     (long long)top_clip_rows, max_chunk);
  static_assert(sizeof(RollEntry) == 24, "the roll table is int64 triples");
  const int naff = (int)(((int64_t)B * n + 255) / 256);
  dim3 grid((unsigned)(naff + (int64_t)nroll * B)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const RollEntry* rt = reinterpret_cast<const RollEntry*>(roll_table);
  long long* ck = reinterpret_cast<long long*>(clock);
#define SRWN_FSO(TT, RR)                                                                                              \
  hipLaunchKernelGGL((flow_stream_out_kernel<TT, RR>), grid, block, 0, st, (const TT*)h, top_clip_rows, flow_w, flow_b, \
                     x_in, x_out, x_stride, carry, clamp ? 1 : 0, rt, naff, B, n, ck, advance_clock ? 1 : 0)
  if (dtype == SRWN_BF16) { if (R == 32) SRWN_FSO(bf16_t, 32); else SRWN_FSO(bf16_t, 64); }
  else if (dtype == SRWN_F32) { if (R == 32) SRWN_FSO(float, 32); else SRWN_FSO(float, 64); }
  else return set_error(SRWN_E_DTYPE, "flow_stream_out: dtype %d", dtype);
#undef SRWN_FSO
  return check_launch("flow_stream_out");
}

extern "C" int srwn_logistic_noise(float* noise, int64_t noise_stride, const float* temperature, const uint64_t* seed,
                                   const int64_t* clock, int32_t B, int32_t n, void* stream) {
  if (!noise || !temperature || !seed || !clock) return set_error(SRWN_E_NULL, "logistic_noise: null pointer");
  if (B < 1 || n < 1 || noise_stride < n)
    return set_error(SRWN_E_SHAPE, "logistic_noise: B=%d n=%d stride=%lld", B, n, (long long)noise_stride);
  const int64_t total = (int64_t)B * n;
  hipLaunchKernelGGL(logistic_noise_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, noise,
                     noise_stride, temperature, seed, reinterpret_cast<const long long*>(clock), B, n);
  return check_launch("logistic_noise");
}

extern "C" int srwn_logistic_from_bits(const uint32_t* bits, float* out, int64_t n, void* stream) {
  if (n == 0) return 0;
  if (!bits || !out) return set_error(SRWN_E_NULL, "logistic_from_bits: null pointer");
  if (n < 0) return set_error(SRWN_E_SHAPE, "logistic_from_bits: n=%lld", (long long)n);
  hipLaunchKernelGGL(logistic_from_bits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bits, out, n);
  return check_launch("logistic_from_bits");
}
