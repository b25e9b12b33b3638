// The auto-encoder's encoder for inference: the whole ResidualDilationLayerNC chain (ops.py:48-58; model.py:136-156)
// of a run of frames in ONE launch, bf16, 128 channels, K = 2 taps at t and t+1.  gfx950 (MI355X) only.
//
// Every layer looks one sample ahead and none back, so frame f of a stream depends on the audio rows
// [f*P, (f+1)*P + L + 1) and nothing else.  One workgroup owns (stream, frame, segment): kSeg = 96 rows of the frame
// plus the 32 rows ahead of them, 128 rows = one 32-row tile per wave, resident in LDS for the whole chain.  The rows
// ahead lose one valid row per layer (the last tile has no neighbour to take its row t+1 from), which after L <= 32
// layers has not reached the 96 rows that count.  Per layer the two weight images stream from L2 into LDS (64 + 32 KB,
// LDS-DMA, the next image under way while the current product runs), the conv accumulator tile is the B operand of the
// residual 1x1 (nc_layer_fwd_kernel's register chaining), and the only thing that leaves the chip is the per-segment
// sum of a_{l+1} over the frame's rows: [segment][L][rows][128] fp32, summed in segment order and scaled to the frame
// mean by nc_frame_finish_kernel ([L][rows][128] bf16, what srwn_pw_linear_ksplit consumes).
//
// Segments are cut from the frame's first row and every sum runs in a fixed order (rows ascending inside a tile, tiles
// ascending, segments ascending), so a frame's bits depend on its own window only: not on its place in the launch, the
// streams beside it or the number of frames.  Rows at or beyond `valid_rows` are beyond the clip: the input of EVERY
// layer is zero there (SAME padding), so r_l is stored as zero on those rows rather than computed from zeros below.
//
// The same chain serves a LIST of frames (srwn_nc_encode_frame_list): workgroup (segment, item) takes its stream, the ring
// column of its first sample and its count of real samples from a device table instead of the grid, and reads the audio
// from a ring [capacity][ring_len] (sample s in column s mod ring_len).  One device body, two instantiations: the
// addressing of the audio and of the output row differ and nothing else does, so a frame from the list has the bits of
// the same frame from the rectangle.  Rows are counted from the frame's first sample and gated by `valid` before any
// load, so a column of the ring that holds an older sample is never read.
#include <atomic>
#include <type_traits>

#include "srwn_common.h"
#include "srwn_host.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

constexpr int kC = 128, kRT = 4, kKS = 8, kTaps = 2;
constexpr int kSeg = 96, kRows = 128, kMaxL = 32;      // frame rows per workgroup | rows it computes | layers it holds
constexpr int kLS = RowStage<bf16_t>::stride(kC);      // 136 elements: padded LDS row
constexpr int kActRows = kRows + 1;                    // + one row that stays zero: row t+1 of the last tile
constexpr int kConvBytes = kRT * kTaps * kKS * 64 * (int)sizeof(Frag<bf16_t>);   // 64 KB
constexpr int kResBytes = kRT * kKS * 64 * (int)sizeof(Frag<bf16_t>);            // 32 KB
constexpr int kActBytes = kActRows * kLS * (int)sizeof(bf16_t);
constexpr size_t kLdsBytes = (size_t)kConvBytes + kResBytes + 2 * 256 * sizeof(float) + 3 * kC * sizeof(float) + kActBytes;
static_assert(kActBytes % 16 == 0, "the activation rows are cleared 16 bytes at a time");
static_assert(kLdsBytes <= 160 * 1024, "one workgroup's LDS");

struct NcEncArgs {
  const float* x; int64_t ld;                          // audio window [B][ld], row 0 = a frame boundary
  const float* nc_w; const float* nc_b;                // 'nc_conv': [2][128], [128]
  const bf16_t* nc_wr; const float* nc_br;             // its residual 1x1 (image [4][8], permuted k), [128]
  const bf16_t* wconv; int64_t wconv_stride;           // layer images, `stride` elements apart
  const bf16_t* wres; int64_t wres_stride;
  const float* bias_c; const float* bias_r;            // [L][128] each
  float* parts;                                        // [nseg][L][B*nframes][128]
  int L, P, nframes, valid;
};

struct NcListArgs : NcEncArgs {                        // x = the ring, ld = ring_len; nframes / valid unused
  const SrwnEncFrame* items;                           // [gridDim.y], device
  int ring_len, capacity;
};

// this thread's LDS-DMA pieces are in LDS (the barrier that follows makes them every wave's)
__device__ __forceinline__ void copies_landed() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

template <class A>
__global__ __launch_bounds__(256) void nc_encode_frames_kernel(A a) {
  constexpr bool kList = std::is_same<A, NcListArgs>::value;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Frag<bf16_t>* lds_conv = reinterpret_cast<Frag<bf16_t>*>(smem);           // [RT][taps*KS][64]
  Frag<bf16_t>* lds_res = lds_conv + kRT * kTaps * kKS * 64;                  // [RT][KS][64], permuted k
  float* lds_bias = reinterpret_cast<float*>(lds_res + kRT * kKS * 64);       // [2 stages][conv 128 | res 128]
  float* lds_sum = lds_bias + 2 * 256;                                        // [3 tiles][128]
  bf16_t* act = reinterpret_cast<bf16_t*>(lds_sum + 3 * kC);                  // [129][kLS]: r_l, or a_{l+1} in passing
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, half = lane >> 5;
  const int seg = blockIdx.x, f = kList ? 0 : blockIdx.y;      // (a list item's window is the frame's own)
  const int nrows = min(kSeg, a.P - seg * kSeg);       // frame rows of this segment
  const int tr = 32 * wave + col;                      // this lane's row of the segment
  const int gt = f * a.P + seg * kSeg + tr;            // ... and of the window
  const bool active = 32 * wave < nrows + a.L;         // tiles further ahead than the chain looks are not computed
  const int64_t R = kList ? (int64_t)gridDim.y : (int64_t)gridDim.z * a.nframes;
  SrwnEncFrame it{};
  if constexpr (kList) {
    it = a.items[blockIdx.y];                          // uniform: a scalar load
    if (it.stream < 0 || it.stream >= a.capacity || it.col < 0 || it.col >= a.ring_len || it.valid < a.P ||
        it.valid > a.P + a.L + 1) {                    // a table that cannot be checked before the launch: zeros
      if (tid < kC)
        for (int l = 0; l < a.L; ++l) a.parts[(((int64_t)seg * a.L + l) * R + blockIdx.y) * kC + tid] = 0.0f;
      return;
    }
  }
  const int b = kList ? it.stream : blockIdx.z;        // the row of the audio
  const int64_t row = kList ? (int64_t)blockIdx.y : (int64_t)b * a.nframes + f;

  lds_dma_copy(a.nc_wr, lds_res, kResBytes, wave, lane, 4);
  lds_dma_copy(a.wconv, lds_conv, kConvBytes, wave, lane, 4);
  lds_bias[tid] = tid < kC ? 0.0f : a.nc_br[tid - kC];
  lds_bias[256 + tid] = tid < kC ? a.bias_c[tid] : a.bias_r[tid - kC];
  for (int i = tid; i < kActBytes / 16; i += 256) reinterpret_cast<f32x4*>(act)[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // r = relu(bias + W . cf) on the rows of the clip, zero beyond it -> this wave's rows of `act`
  auto residual = [&](const Frag<bf16_t> (&cf)[kKS], const float* bias) {
    f32x16 accR[kRT];
#pragma unroll
    for (int mt = 0; mt < kRT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + 32 * mt + 8 * g + 4 * half);
#pragma unroll
        for (int e = 0; e < 4; ++e) accR[mt][4 * g + e] = bv[e];
      }
    Frag<bf16_t> af[2][kRT];
#pragma unroll
    for (int mt = 0; mt < kRT; ++mt) af[0][mt] = lds_res[(mt * kKS) * 64 + lane];
#pragma unroll
    for (int s = 0; s < kKS; ++s) {
      if (s + 1 < kKS) {
#pragma unroll
        for (int mt = 0; mt < kRT; ++mt) af[(s + 1) & 1][mt] = lds_res[(mt * kKS + s + 1) * 64 + lane];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mt = 0; mt < kRT; ++mt) mma(accR[mt], af[s & 1][mt], cf[s]);
      __builtin_amdgcn_sched_barrier(0);
    }
    bool in_clip;      // (the count is read from the arguments here: through a local copy the frames instantiation
                       // compiled to other scalar code and its launch ran 2 % longer)
    if constexpr (kList) in_clip = gt < it.valid; else in_clip = gt < a.valid;
    wave_lds_order();                     // the frame sums have read this wave's rows
#pragma unroll
    for (int mt = 0; mt < kRT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = in_clip ? fmaxf(accR[mt][4 * g + e], 0.0f) : 0.0f;
        store4(act + tr * kLS + 32 * mt + 8 * g + 4 * half, v[0], v[1], v[2], v[3]);
      }
  };

  // stage 0: a_0 = relu(nc_conv(relu(x))) on the VALU in accumulator layout (srwn_nc_input_fwd's operations), r_0
  {
    Frag<bf16_t> cf[kKS];
    if (active) {
      const float* xb = a.x + (int64_t)b * a.ld;
      float x0, x1;
      if constexpr (kList) {                           // col < ring_len and a row that is read is < valid <= ring_len:
        int c0 = it.col + gt, c1 = it.col + gt + 1;    // one compare and subtract wraps it
        if (c0 >= a.ring_len) c0 -= a.ring_len;
        if (c1 >= a.ring_len) c1 -= a.ring_len;
        x0 = gt < it.valid ? fmaxf(xb[c0], 0.0f) : 0.0f;
        x1 = gt + 1 < it.valid ? fmaxf(xb[c1], 0.0f) : 0.0f;
      } else {
        x0 = gt < a.valid ? fmaxf(xb[gt], 0.0f) : 0.0f;
        x1 = gt + 1 < a.valid ? fmaxf(xb[gt + 1], 0.0f) : 0.0f;
      }
#pragma unroll
      for (int mt = 0; mt < kRT; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c0 = 32 * mt + 8 * g + 4 * half;
          const f32x4 w0 = *reinterpret_cast<const f32x4*>(a.nc_w + c0);
          const f32x4 w1 = *reinterpret_cast<const f32x4*>(a.nc_w + kC + c0);
          const f32x4 bb = *reinterpret_cast<const f32x4*>(a.nc_b + c0);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int q = 4 * g + e;
            const float v = fmaxf(fmaf(x1, w1[e], fmaf(x0, w0[e], bb[e])), 0.0f);
            cf[2 * mt + (q >> 3)].set(q & 7, v);
          }
        }
    }
    copies_landed();
    __syncthreads();   // images, biases and the cleared rows landed
    if (active) residual(cf, lds_bias + kC);
    __syncthreads();
    if (a.L > 1) lds_dma_copy(a.wres, lds_res, kResBytes, wave, lane, 4);
  }

  for (int l = 0; l < a.L; ++l) {
    const float* bias = lds_bias + ((l + 1) & 1) * 256;
    // (the next layer's biases are fetched ahead of the image copies: a wait for them behind those would drain the copies)
    float next_bias = 0.0f;
    if (l + 1 < a.L) next_bias = tid < kC ? a.bias_c[(l + 1) * kC + tid] : a.bias_r[(l + 1) * kC + tid - kC];
    f32x16 accF[kRT];
    if (active) {
#pragma unroll
      for (int mt = 0; mt < kRT; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + 32 * mt + 8 * g + 4 * half);
#pragma unroll
          for (int e = 0; e < 4; ++e) accF[mt][4 * g + e] = bv[e];
        }
      // operands of k-step s+1 are read from LDS before the MFMAs of k-step s issue (nc_layer_fwd_kernel)
      constexpr int NS = kTaps * kKS;
      Frag<bf16_t> af[2][kRT], bfr[2];
      auto fetch = [&](int s, int slot) {
        const int k = s / kKS, ks = s % kKS;
        bfr[slot] = load_nat(act + (tr + k) * kLS + 16 * ks + 8 * half);
#pragma unroll
        for (int mt = 0; mt < kRT; ++mt) af[slot][mt] = lds_conv[(mt * NS + s) * 64 + lane];
      };
      fetch(0, 0);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (s + 1 < NS) fetch(s + 1, (s + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mt = 0; mt < kRT; ++mt) mma(accF[mt], af[s & 1][mt], bfr[s & 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    copies_landed();
    __syncthreads();   // every wave has read r_l and the conv image; the residual image of this layer landed
    if (l + 1 < a.L) {
      lds_bias[(l & 1) * 256 + tid] = next_bias;
      lds_dma_copy(a.wconv + (int64_t)(l + 1) * a.wconv_stride, lds_conv, kConvBytes, wave, lane, 4);
    }
    Frag<bf16_t> cf[kKS];
    if (active) {      // a_{l+1} -> this wave's rows (r_l is no longer needed), as the bf16 values the next product sees
#pragma unroll
      for (int mt = 0; mt < kRT; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int q = 4 * g + e;
            v[e] = fmaxf(accF[mt][q], 0.0f);
            cf[2 * mt + (q >> 3)].set(q & 7, v[e]);
          }
          store4(act + tr * kLS + 32 * mt + 8 * g + 4 * half, v[0], v[1], v[2], v[3]);
        }
    }
    wave_lds_order();
    if (wave < 3) {    // sum over the tile's frame rows, ascending; lane = channels 2 lane, 2 lane + 1
      const int hi = min(32, nrows - 32 * wave);
      float s0 = 0.0f, s1 = 0.0f;
      for (int rr = 0; rr < hi; ++rr) {
        const bf16x2 v = *reinterpret_cast<const bf16x2*>(act + (32 * wave + rr) * kLS + 2 * lane);
        s0 += (float)v[0];
        s1 += (float)v[1];
      }
      *reinterpret_cast<f32x2*>(lds_sum + wave * kC + 2 * lane) = f32x2{s0, s1};
    }
    if (active && l + 1 < a.L) residual(cf, bias + kC);   // the last layer's residual output is never used
    copies_landed();
    __syncthreads();   // r_{l+1} and the tile sums are written; the next conv image landed
    if (l + 2 < a.L) lds_dma_copy(a.wres + (int64_t)(l + 1) * a.wres_stride, lds_res, kResBytes, wave, lane, 4);
    if (wave == 0) {
      const f32x2 p0 = *reinterpret_cast<const f32x2*>(lds_sum + 2 * lane);
      const f32x2 p1 = *reinterpret_cast<const f32x2*>(lds_sum + kC + 2 * lane);
      const f32x2 p2 = *reinterpret_cast<const f32x2*>(lds_sum + 2 * kC + 2 * lane);
      *reinterpret_cast<f32x2*>(a.parts + (((int64_t)seg * a.L + l) * R + row) * kC + 2 * lane) = (p0 + p1) + p2;
    }
  }
}

// means[i] = scale * sum over segments (ascending) of parts[seg][i]
__global__ __launch_bounds__(256) void nc_frame_finish_kernel(const float* __restrict__ parts, bf16_t* __restrict__ out,
                                                              int nseg, int64_t n, float scale) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.0f;
  for (int k = 0; k < nseg; ++k) s += parts[(int64_t)k * n + i];
  out[i] = (bf16_t)(s * scale);
}

// dst row streams[i], columns (first_col[i] + j) mod ring_len <- src[src_offset[i] + j], j < counts[i]
__global__ __launch_bounds__(256) void audio_ring_put_kernel(float* __restrict__ ring, int ring_len, int capacity,
                                                             const float* __restrict__ src,
                                                             const int32_t* __restrict__ streams,
                                                             const int32_t* __restrict__ src_offset,
                                                             const int32_t* __restrict__ first_col,
                                                             const int32_t* __restrict__ counts, int max_count) {
  const int i = blockIdx.y;
  const int u = streams[i], c0 = first_col[i], n = min(min(counts[i], max_count), ring_len);
  if (u < 0 || u >= capacity || c0 < 0 || c0 >= ring_len || src_offset[i] < 0) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  int c = c0 + j;                                      // < 2 ring_len
  if (c >= ring_len) c -= ring_len;
  ring[(int64_t)u * ring_len + c] = src[(int64_t)src_offset[i] + j];
}

// once per device and kernel: the attribute call is host time on a path of five launches.  The attribute belongs to the
// current device; two threads that both find the bit clear both set the same value, which is harmless.
template <class Kern>
int allow_lds(Kern kern, std::atomic<uint64_t>& lds_set, const char* who) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  const uint64_t bit = (dev >= 0 && dev < 64) ? (uint64_t)1 << dev : 0;       // (beyond 64 devices: every call)
  if (!(lds_set.load(std::memory_order_acquire) & bit)) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e != hipSuccess) return set_error((int)e, "%s: LDS %zu: %s", who, kLdsBytes, hipGetErrorString(e));
    lds_set.fetch_or(bit, std::memory_order_release);
  }
  return 0;
}

// what the two chain entries check alike; 1: go on
int check_chain(const char* who, bool nulls, const void* wres, int32_t nlayers, int32_t C, int32_t K, int32_t dtype) {
  if (nulls) return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if (dtype != SRWN_BF16 && dtype != SRWN_F32) return set_error(SRWN_E_DTYPE, "%s: dtype %d", who, dtype);
  if (C != kC || K != kTaps || dtype != SRWN_BF16)
    return set_error(SRWN_E_UNSUPPORTED, "%s: built for 128 channels, K=2, bf16 (got C=%d K=%d dtype=%d)", who, C, K, dtype);
  if (nlayers < 1 || nlayers > kMaxL)
    return set_error(SRWN_E_SHAPE, "%s: %d layers, the kernel holds 1..%d", who, nlayers, kMaxL);
  if (nlayers > 1 && !wres) return set_error(SRWN_E_NULL, "%s: null pointer", who);
  return 1;
}

int finish_frames(const float* partials, void* means, int nseg, int64_t n, int32_t pool_stride, hipStream_t st) {
  hipLaunchKernelGGL(nc_frame_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, partials, (bf16_t*)means,
                     nseg, n, 1.0f / (float)pool_stride);
  return check_launch("nc_frame_finish");
}

}  // namespace

extern "C" int32_t srwn_nc_encode_max_layers(void) { return kMaxL; }

extern "C" int64_t srwn_nc_encode_partials(int32_t B, int32_t nframes, int32_t pool_stride, int32_t nlayers) {
  if (B < 0 || nframes < 0 || pool_stride < 1 || nlayers < 0) return 0;
  return (int64_t)((pool_stride + kSeg - 1) / kSeg) * nlayers * B * nframes * kC;
}

extern "C" int64_t srwn_nc_encode_list_partials(int32_t nitems, int32_t pool_stride, int32_t nlayers) {
  return srwn_nc_encode_partials(1, nitems, pool_stride, nlayers);
}

extern "C" int srwn_nc_encode_frames(const float* x, int64_t ld, const float* nc_w, const float* nc_b, const void* nc_wr,
                                     const float* nc_br, const void* wconv, int64_t wconv_stride, const void* wres,
                                     int64_t wres_stride, const float* bias_c, const float* bias_r, float* partials,
                                     void* means, int32_t B, int32_t nframes, int32_t pool_stride, int32_t valid_rows,
                                     int32_t nlayers, int32_t C, int32_t K, int32_t dtype, void* stream) {
  const char* who = "nc_encode_frames";
  if (B == 0 || nframes == 0) return 0;
  int rc = check_chain(who, !x || !nc_w || !nc_b || !nc_wr || !nc_br || !wconv || !bias_c || !bias_r || !partials || !means,
                       wres, nlayers, C, K, dtype);
  if (rc != 1) return rc;
  if (B < 0 || nframes < 0 || B > 65535 || nframes > 65535 || pool_stride < 1 ||
      (int64_t)nframes * pool_stride + nlayers + 1 > 0x7fffffffLL)
    return set_error(SRWN_E_SHAPE, "nc_encode_frames: B=%d nframes=%d pool=%d", B, nframes, pool_stride);
  const int64_t need = (int64_t)nframes * pool_stride;
  if (valid_rows < need || valid_rows > need + nlayers + 1 || ld < valid_rows)
    return set_error(SRWN_E_SHAPE, "nc_encode_frames: valid_rows %d outside [%lld, %lld] (ld %lld)", valid_rows,
                     (long long)need, (long long)(need + nlayers + 1), (long long)ld);
  const int nseg = (pool_stride + kSeg - 1) / kSeg;
  if (nseg > 65535) return set_error(SRWN_E_SHAPE, "nc_encode_frames: pool_stride %d", pool_stride);
  NcEncArgs a;
  a.x = x; a.ld = ld; a.nc_w = nc_w; a.nc_b = nc_b; a.nc_wr = (const bf16_t*)nc_wr; a.nc_br = nc_br;
  a.wconv = (const bf16_t*)wconv; a.wconv_stride = wconv_stride; a.wres = (const bf16_t*)wres; a.wres_stride = wres_stride;
  a.bias_c = bias_c; a.bias_r = bias_r; a.parts = partials;
  a.L = nlayers; a.P = pool_stride; a.nframes = nframes; a.valid = valid_rows;
  hipStream_t st = (hipStream_t)stream;
  static std::atomic<uint64_t> lds_set{0};
  if ((rc = allow_lds(nc_encode_frames_kernel<NcEncArgs>, lds_set, who))) return rc;
  hipLaunchKernelGGL(nc_encode_frames_kernel<NcEncArgs>, dim3((unsigned)nseg, (unsigned)nframes, (unsigned)B), dim3(256),
                     kLdsBytes, st, a);
  if ((rc = check_launch(who))) return rc;
  return finish_frames(partials, means, nseg, (int64_t)nlayers * B * nframes * kC, pool_stride, st);
}

extern "C" int srwn_nc_encode_frame_list(const float* ring, int32_t ring_len, int32_t capacity, const SrwnEncFrame* frames,
                                         int32_t nitems, const float* nc_w, const float* nc_b, const void* nc_wr,
                                         const float* nc_br, const void* wconv, int64_t wconv_stride, const void* wres,
                                         int64_t wres_stride, const float* bias_c, const float* bias_r, float* partials,
                                         void* means, int32_t pool_stride, int32_t nlayers, int32_t C, int32_t K,
                                         int32_t dtype, void* stream) {
  const char* who = "nc_encode_frame_list";
  if (nitems == 0) return 0;
  int rc = check_chain(who, !ring || !frames || !nc_w || !nc_b || !nc_wr || !nc_br || !wconv || !bias_c || !bias_r ||
                                !partials || !means, wres, nlayers, C, K, dtype);
  if (rc != 1) return rc;
  if (pool_stride < 1 || (pool_stride + kSeg - 1) / kSeg > 65535)
    return set_error(SRWN_E_SHAPE, "nc_encode_frame_list: pool_stride %d", pool_stride);
  if (nitems < 0 || nitems > 65535 || capacity < 1 || (int64_t)pool_stride + nlayers + 1 > 0x7fffffffLL ||
      ring_len < pool_stride + nlayers + 1)
    return set_error(SRWN_E_SHAPE, "nc_encode_frame_list: nitems=%d capacity=%d ring_len=%d (a frame reads %lld samples)",
                     nitems, capacity, ring_len, (long long)pool_stride + nlayers + 1);
  const int nseg = (pool_stride + kSeg - 1) / kSeg;
  NcListArgs a;
  a.x = ring; a.ld = ring_len; a.nc_w = nc_w; a.nc_b = nc_b; a.nc_wr = (const bf16_t*)nc_wr; a.nc_br = nc_br;
  a.wconv = (const bf16_t*)wconv; a.wconv_stride = wconv_stride; a.wres = (const bf16_t*)wres; a.wres_stride = wres_stride;
  a.bias_c = bias_c; a.bias_r = bias_r; a.parts = partials;
  a.L = nlayers; a.P = pool_stride; a.nframes = 1; a.valid = 0;
  a.items = frames; a.ring_len = ring_len; a.capacity = capacity;
  hipStream_t st = (hipStream_t)stream;
  static std::atomic<uint64_t> lds_set{0};
  if ((rc = allow_lds(nc_encode_frames_kernel<NcListArgs>, lds_set, who))) return rc;
  hipLaunchKernelGGL(nc_encode_frames_kernel<NcListArgs>, dim3((unsigned)nseg, (unsigned)nitems), dim3(256), kLdsBytes, st,
                     a);
  if ((rc = check_launch(who))) return rc;
  return finish_frames(partials, means, nseg, (int64_t)nlayers * nitems * kC, pool_stride, st);
}

extern "C" int srwn_audio_ring_put(float* ring, int32_t ring_len, int32_t capacity, const float* src,
                                   const int32_t* streams, const int32_t* src_offset, const int32_t* first_col,
                                   const int32_t* counts, int32_t n, int32_t max_count, void* stream) {
  if (n == 0 || max_count == 0) return 0;
  if (!ring || !src || !streams || !src_offset || !first_col || !counts)
    return set_error(SRWN_E_NULL, "audio_ring_put: null pointer");
  if (ring_len < 1 || capacity < 1 || n < 0 || n > 65535 || max_count < 0 || max_count > ring_len)
    return set_error(SRWN_E_SHAPE, "audio_ring_put: ring_len=%d capacity=%d n=%d max_count=%d", ring_len, capacity, n,
                     max_count);
  hipLaunchKernelGGL(audio_ring_put_kernel, dim3((unsigned)((max_count + 255) / 256), (unsigned)n), dim3(256), 0,
                     (hipStream_t)stream, ring, ring_len, capacity, src, streams, src_offset, first_col, counts, max_count);
  return check_launch("audio_ring_put");
}
