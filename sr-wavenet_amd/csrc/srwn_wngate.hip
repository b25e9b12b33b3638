// Canonical WaveNet gate (gate_mode "wavenet"): c = tanh(Wf*x + bf) * sigmoid(Wg*x + bg), one launch per layer.
// The training twin of srwn_residual_layer_fwd / _bwd (csrc/srwn_fwd.hip, csrc/srwn_bwd.hip) for the gated unit that
// ops.py:31-32 builds and ops.py:33 discards.  gfx950 (MI355X) only; MFMA orientation and lane maps: srwn_common.h.
//   forward   both causal convs as ONE (K*R)-deep contraction into 2R output rows from the packed [Wf | Wg] image, the
//             gate epilogue, the 1x1 residual on c straight from the accumulators, dense output (x + res)*sqrt(.5)
//             (+ the next layer's conditioning bias).  Stores x_{l+1}, z, s and c (c feeds the skip sum and the 1x1
//             weight gradients with SRWN_PRO_NONE).
//   backward  G_{l+1} = G_{l+2}*sqrt(.5) + sum_k [Wf|Wg]_{l+1}[k] . D_{l+1}[t + (K-1-k) d_{l+1}]  (contraction over K*2R)
//             dc = Wr_l . (G_{l+1} sqrt(.5)) + skip term;   D_l = [dc*s*(1-z^2) | dc*z*s*(1-s)]   [rows, 2R]
// Persistent waves over 32-step time tiles; the weight images sit in LDS (LDS-DMA), activation fragments are read
// straight from HBM (natural k order, one 16-byte load per lane), outputs leave as whole rows through a wave-private
// LDS stage (store_rows_via_lds).
#include "srwn_common.h"
#include "srwn_host.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

// sigmoid on the whole real line (the gate pre-activation is not bounded like the reference gate's tanh output, so
// Math<bf16_t>::sigmoid_'s polynomial on [-1, 1] does not apply).  fp32: libm; bf16: hardware exp2 / rcp.
template <typename T> __device__ __forceinline__ float wn_sigmoid(float x);
template <> __device__ __forceinline__ float wn_sigmoid<float>(float x) { return 1.0f / (1.0f + expf(-x)); }
template <> __device__ __forceinline__ float wn_sigmoid<bf16_t>(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}

constexpr int kWnK = 2;   // filter_width (the only one built, as for the reference-gate kernels)

struct WnFwdArgs {
  const void* x;         // x_l [B,T,R] (the layer's complete, conditioned input)
  const void* cond;      // next layer's frame bias [B, frames, >= R] rows cond_stride apart (COND)
  const void* wconv;     // packed [2R/32][K*R/16] natural: rows 0..R-1 = Wf, R..2R-1 = Wg; k = tap*R + in channel
  const void* wres;      // packed [R/32][R/16] permuted (pack_res)
  const float* bias_f; const float* bias_g; const float* bias_r;
  void* h_out; void* z_out; void* s_out; void* c_out;
  int Tlen, dilation, cond_frames, pool, cond_stride, ntb, ntiles;
};

template <typename T, int RT, bool COND>
__global__ __launch_bounds__(256) void wavenet_layer_fwd_kernel(WnFwdArgs a) {
  constexpr int K = kWnK, R = 32 * RT, KS = R / 16;
  constexpr int NCONV = 2 * RT * K * KS, NRES = RT * KS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Frag<T>* lds_conv = reinterpret_cast<Frag<T>*>(smem);
  Frag<T>* lds_res = lds_conv + NCONV * 64;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  T* stage = reinterpret_cast<T*>(lds_res + NRES * 64) + wave * (32 * RowStage<T>::stride(R));   // wave-private
  lds_dma_copy(a.wconv, lds_conv, NCONV * 64 * (int)sizeof(Frag<T>), wave, lane, 4);
  lds_dma_copy(a.wres, lds_res, NRES * 64 * (int)sizeof(Frag<T>), wave, lane, 4);
  __syncthreads();   // weights landed (vmcnt(0) + barrier)

  const int col = lane & 31, half = lane >> 5;
  const T* x = reinterpret_cast<const T*>(a.x);
  for (int tile = blockIdx.x * 4 + wave; tile < a.ntiles; tile += gridDim.x * 4) {
    const int b = tile / a.ntb;
    const int t0 = (tile - b * a.ntb) * 32;
    const int tc = t0 + col;
    const bool ok = tc < a.Tlen;
    const int tcc = ok ? tc : a.Tlen - 1;
    const int rows_valid = a.Tlen - t0;   // >= 1
    const size_t boff = (size_t)b * a.Tlen;

    // B fragments of both taps (rows clamped into the clip, zeroed where the tap is outside it)
    Frag<T> cur[K][KS];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int tk = tc - (K - 1 - k) * a.dilation;
      const bool valid = ok && tk >= 0;
      const int tkc = tk < 0 ? 0 : (tk < a.Tlen ? tk : a.Tlen - 1);
      const T* row = x + (boff + tkc) * R + 8 * half;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const Frag<T> f = load_nat(row + 16 * ks);
        cur[k][ks] = valid ? f : zero_frag<T>();
      }
    }

    // ---- filter and gate conv as one (K*R)-deep contraction into 2R rows; accumulators start at the biases
    f32x16 acc[2 * RT];
#pragma unroll
    for (int mt = 0; mt < 2 * RT; ++mt)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int n = 32 * (mt % RT) + crow(q, half);
        acc[mt][q] = mt < RT ? a.bias_f[n] : a.bias_g[n];
      }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int mt = 0; mt < 2 * RT; ++mt) mma(acc[mt], lds_conv[(mt * (K * KS) + k * KS + ks) * 64 + lane], cur[k][ks]);

    // ---- gate: z = tanh(f), s = sigmoid(g), c = z*s; c in registers is the B operand of the 1x1 residual
    Frag<T> cf[KS];
    {
      float zv[RT][16], sv[RT][16], cv[RT][16];
#pragma unroll
      for (int mt = 0; mt < RT; ++mt)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float z = Math<T>::tanh_(acc[mt][q]);
          const float s = wn_sigmoid<T>(acc[RT + mt][q]);
          zv[mt][q] = z;
          sv[mt][q] = s;
          cv[mt][q] = z * s;
          cf[2 * mt + (q >> 3)].set(q & 7, z * s);
        }
      store_rows_via_lds<T, RT>(stage, reinterpret_cast<T*>(a.z_out) + (boff + t0) * R, R, zv, rows_valid, lane);
      store_rows_via_lds<T, RT>(stage, reinterpret_cast<T*>(a.s_out) + (boff + t0) * R, R, sv, rows_valid, lane);
      store_rows_via_lds<T, RT>(stage, reinterpret_cast<T*>(a.c_out) + (boff + t0) * R, R, cv, rows_valid, lane);
    }

    // ---- 1x1 residual, scaled residual add (+ the NEXT layer's conditioning bias)
    f32x16 accR[RT];
#pragma unroll
    for (int mt = 0; mt < RT; ++mt)
#pragma unroll
      for (int q = 0; q < 16; ++q) accR[mt][q] = a.bias_r[32 * mt + crow(q, half)];
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int mt = 0; mt < RT; ++mt) mma(accR[mt], lds_res[(mt * KS + s) * 64 + lane], cf[s]);
    {
      const T* xr = x + (boff + tcc) * R;
      const T* cb = COND ? reinterpret_cast<const T*>(a.cond) + ((size_t)b * a.cond_frames + tcc / a.pool) * a.cond_stride
                         : nullptr;
      float hv[RT][16];
#pragma unroll
      for (int mt = 0; mt < RT; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ch = 32 * mt + 8 * g + 4 * half;
          const f32x4 xv = load4(xr + ch);
          f32x4 cv = {0.f, 0.f, 0.f, 0.f};
          if (COND) cv = load4(cb + ch);
#pragma unroll
          for (int e = 0; e < 4; ++e) hv[mt][4 * g + e] = (xv[e] + accR[mt][4 * g + e]) * kSqrtHalf + cv[e];
        }
      store_rows_via_lds<T, RT>(stage, reinterpret_cast<T*>(a.h_out) + (boff + t0) * R, R, hv, rows_valid, lane);
    }
  }
}

struct WnBwdArgs {
  const void* g_in;      // G_{l+2} [B,T,R] (NULL: zero)                                   (up)
  const void* d_up;      // D_{l+1} [B,T,2R]                                                (up)
  const void* wconvT;    // [WfT | WgT] of layer l+1: two packed [R/32][K*R/16] images back to back, natural,
                         // rows = in channel i, k = tap*R + out channel o                     (up)
  void* g_out;           // G_{l+1} [B,T,R]                                                 (up)
  const void* wresT;     // packed [R/32][R/16] permuted: rows = n, k = m (Wr_l[n][m])      (up && down)
  const void* wskipT;    // packed [R/32][S/16] natural: rows = n, k = s (Ws_l[n][s])       (down, no dcs)
  const void* dtotal;    // [B*T, S]                                                        (down, no dcs)
  const void* dcs;       // Ws_l . dtotal [B,T,R]                                           (down, dcs mode)
  const void* z; const void* s;   // z_l, s_l [B,T,R]                                        (down)
  void* d_out;           // D_l [B,T,2R]                                                     (down)
  int Tlen, dil_up, S, ntb, ntiles, up, down;
};

template <typename T, int RT>
__global__ __launch_bounds__(256) void wavenet_layer_bwd_kernel(WnBwdArgs a) {
  constexpr int K = kWnK, R = 32 * RT, KS = R / 16;
  constexpr int NCONV = 2 * RT * K * KS, NRES = RT * KS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Frag<T>* lds_conv = reinterpret_cast<Frag<T>*>(smem);
  Frag<T>* lds_res = lds_conv + NCONV * 64;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  T* stage = reinterpret_cast<T*>(lds_res + NRES * 64) + wave * (32 * RowStage<T>::stride(R));
  const bool up = a.up != 0, down = a.down != 0, gin = a.g_in != nullptr, dcs = a.dcs != nullptr;
  const bool skip_here = down && !dcs && a.S > 0;
  if (up) lds_dma_copy(a.wconvT, lds_conv, NCONV * 64 * (int)sizeof(Frag<T>), wave, lane, 4);
  if (up && down) lds_dma_copy(a.wresT, lds_res, NRES * 64 * (int)sizeof(Frag<T>), wave, lane, 4);
  __syncthreads();

  const int col = lane & 31, half = lane >> 5;
  const int KSS = a.S / 16;
  const Frag<T>* wskip = reinterpret_cast<const Frag<T>*>(a.wskipT);
  for (int tile = blockIdx.x * 4 + wave; tile < a.ntiles; tile += gridDim.x * 4) {
    const int b = tile / a.ntb;
    const int t0 = (tile - b * a.ntb) * 32;
    const int tc = t0 + col;
    const bool ok = tc < a.Tlen;
    const int tcc = ok ? tc : a.Tlen - 1;
    const int rows_valid = a.Tlen - t0;
    const size_t boff = (size_t)b * a.Tlen;
    const size_t rowi = boff + tcc;

    f32x16 accG[RT];
#pragma unroll
    for (int mt = 0; mt < RT; ++mt)
#pragma unroll
      for (int q = 0; q < 16; ++q) accG[mt][q] = 0.0f;
    if (up) {
      // residual path: G_{l+2} * sqrt(.5) in accumulator layout
      if (gin) {
        const T* gr = reinterpret_cast<const T*>(a.g_in) + rowi * R;
#pragma unroll
        for (int mt = 0; mt < RT; ++mt)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x4 v = load4(gr + 32 * mt + 8 * g + 4 * half);
#pragma unroll
            for (int e = 0; e < 4; ++e) accG[mt][4 * g + e] = ok ? v[e] * kSqrtHalf : 0.0f;
          }
      }
      // both convs' data gradients: anti-causal taps read D_{l+1} at t + (K-1-k)*d (zero beyond the clip);
      // part p = 0 contracts over the filter half of D with WfT, p = 1 over the gate half with WgT
      const T* du = reinterpret_cast<const T*>(a.d_up);
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int tk = tc + (K - 1 - k) * a.dil_up;
          const bool valid = ok && tk < a.Tlen;
          const int tkc = tk < a.Tlen ? tk : a.Tlen - 1;
          const T* row = du + (boff + tkc) * (2 * R) + p * R + 8 * half;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const Frag<T> f = load_nat(row + 16 * ks);
            const Frag<T> bf = valid ? f : zero_frag<T>();
#pragma unroll
            for (int mt = 0; mt < RT; ++mt)
              mma(accG[mt], lds_conv[((p * RT + mt) * (K * KS) + k * KS + ks) * 64 + lane], bf);
          }
        }
      float gv[RT][16];
#pragma unroll
      for (int mt = 0; mt < RT; ++mt)
#pragma unroll
        for (int q = 0; q < 16; ++q) gv[mt][q] = accG[mt][q];
      store_rows_via_lds<T, RT>(stage, reinterpret_cast<T*>(a.g_out) + (boff + t0) * R, R, gv, rows_valid, lane);
    }
    if (down) {
      f32x16 accC[RT];
#pragma unroll
      for (int mt = 0; mt < RT; ++mt)
#pragma unroll
        for (int q = 0; q < 16; ++q) accC[mt][q] = 0.0f;
      if (dcs) {
        const T* dr = reinterpret_cast<const T*>(a.dcs) + rowi * R;
#pragma unroll
        for (int mt = 0; mt < RT; ++mt)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x4 v = load4(dr + 32 * mt + 8 * g + 4 * half);
#pragma unroll
            for (int e = 0; e < 4; ++e) accC[mt][4 * g + e] = ok ? v[e] : 0.0f;
          }
      }
      if (up) {
        // dres = G_{l+1} * sqrt(.5): the accumulator tile is the B operand (permuted k order)
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          Frag<T> bf;
#pragma unroll
          for (int j = 0; j < 8; ++j) bf.set(j, accG[s >> 1][8 * (s & 1) + j] * kSqrtHalf);
#pragma unroll
          for (int mt = 0; mt < RT; ++mt) mma(accC[mt], lds_res[(mt * KS + s) * 64 + lane], bf);
        }
      }
      if (skip_here) {
        // Ws_l . dtotal with the skip image read from L2 (S/16 k-steps)
        const T* dt = reinterpret_cast<const T*>(a.dtotal) + rowi * a.S + 8 * half;
        for (int ks = 0; ks < KSS; ++ks) {
          const Frag<T> f = load_nat(dt + 16 * ks);
          const Frag<T> bf = ok ? f : zero_frag<T>();
#pragma unroll
          for (int mt = 0; mt < RT; ++mt) mma(accC[mt], wskip[(mt * KSS + ks) * 64 + lane], bf);
        }
      }
      // D = [dc * s * (1 - z^2) | dc * z * s * (1 - s)]
      const T* zr = reinterpret_cast<const T*>(a.z) + rowi * R;
      const T* sr = reinterpret_cast<const T*>(a.s) + rowi * R;
      float df[RT][16], dg[RT][16];
#pragma unroll
      for (int mt = 0; mt < RT; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ch = 32 * mt + 8 * g + 4 * half;
          const f32x4 zv = load4(zr + ch), sv = load4(sr + ch);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float dc = accC[mt][4 * g + e], z = zv[e], s = sv[e];
            df[mt][4 * g + e] = dc * s * (1.0f - z * z);
            dg[mt][4 * g + e] = dc * z * s * (1.0f - s);
          }
        }
      T* dtile = reinterpret_cast<T*>(a.d_out) + (boff + t0) * (2 * R);
      store_rows_via_lds<T, RT>(stage, dtile, 2 * R, df, rows_valid, lane);
      store_rows_via_lds<T, RT>(stage, dtile + R, 2 * R, dg, rows_valid, lane);
    }
  }
}

template <typename T, int RT>
size_t wn_lds_bytes() {
  constexpr int R = 32 * RT, KS = R / 16;
  return (size_t)(2 * RT * kWnK * KS + RT * KS) * 64 * sizeof(Frag<T>) + (size_t)4 * 32 * RowStage<T>::stride(R) * sizeof(T);
}

int wn_grid(long long ntiles) {
  long long blocks = (ntiles + 3) / 4;
  return (int)(blocks > 512 ? 512 : blocks);   // persistent waves: two workgroups per CU at most
}

template <typename T, int RT>
int launch_wn_fwd(WnFwdArgs a, int B, bool cond, hipStream_t st) {
  const size_t sh = wn_lds_bytes<T, RT>();
  a.ntb = (a.Tlen + 31) / 32;
  a.ntiles = (int)((long long)B * a.ntb);
  auto kfn = cond ? wavenet_layer_fwd_kernel<T, RT, true> : wavenet_layer_fwd_kernel<T, RT, false>;
  if (sh > 32768) {
    hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    if (e != hipSuccess) return set_error((int)e, "wavenet_layer_fwd: LDS %zu: %s", sh, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kfn, dim3(wn_grid(a.ntiles)), dim3(256), sh, st, a);
  return check_launch("wavenet_layer_fwd");
}

template <typename T, int RT>
int launch_wn_bwd(WnBwdArgs a, int B, hipStream_t st) {
  const size_t sh = wn_lds_bytes<T, RT>();
  a.ntb = (a.Tlen + 31) / 32;
  a.ntiles = (int)((long long)B * a.ntb);
  auto kfn = wavenet_layer_bwd_kernel<T, RT>;
  if (sh > 32768) {
    hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    if (e != hipSuccess) return set_error((int)e, "wavenet_layer_bwd: LDS %zu: %s", sh, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(kfn, dim3(wn_grid(a.ntiles)), dim3(256), sh, st, a);
  return check_launch("wavenet_layer_bwd");
}

}  // namespace

extern "C" int srwn_wavenet_layer_fwd(const void* x, const void* cond, const void* wconv, const void* wres,
                                      const float* bias_f, const float* bias_g, const float* bias_r, void* h_out,
                                      void* z_out, void* s_out, void* c_out, int32_t B, int32_t T, int32_t R, int32_t K,
                                      int32_t dilation, int32_t cond_frames, int32_t pool_stride,
                                      int32_t cond_row_stride, int32_t dtype, void* stream) {
  if (!x || !wconv || !wres || !bias_f || !bias_g || !bias_r || !h_out || !z_out || !s_out || !c_out)
    return set_error(SRWN_E_NULL, "wavenet_layer_fwd: null pointer");
  if (B < 0 || T < 0 || dilation < 1) return set_error(SRWN_E_SHAPE, "wavenet_layer_fwd: B=%d T=%d d=%d", B, T, dilation);
  if ((long long)B * ((T + 31) / 32) > 0x7fffffffLL) return set_error(SRWN_E_SHAPE, "wavenet_layer_fwd: too many tiles");
  if (cond && (pool_stride < 1 || cond_frames < 1 || cond_row_stride < R || cond_row_stride % 8 ||
               (int64_t)cond_frames * pool_stride < T))
    return set_error(SRWN_E_SHAPE, "wavenet_layer_fwd: cond frames %d x pool %d < T %d (row stride %d)", cond_frames,
                     pool_stride, T, cond_row_stride);
  if (K != kWnK) return set_error(SRWN_E_UNSUPPORTED, "wavenet_layer_fwd: filter_width %d (only 2 is built)", K);
  if (dtype != SRWN_BF16 && dtype != SRWN_F32) return set_error(SRWN_E_DTYPE, "wavenet_layer_fwd: dtype %d", dtype);
  if (R != 32 && R != 64) return set_error(SRWN_E_UNSUPPORTED, "wavenet_layer_fwd: dilation_channels %d (built: 32, 64)", R);
  if (B == 0 || T == 0) return 0;
  WnFwdArgs a{x, cond, wconv, wres, bias_f, bias_g, bias_r, h_out, z_out, s_out, c_out, T, dilation,
              cond ? cond_frames : 1, cond ? pool_stride : 1, cond ? cond_row_stride : R, 0, 0};
  hipStream_t st = (hipStream_t)stream;
  const bool c = cond != nullptr;
  if (dtype == SRWN_BF16) return R == 32 ? launch_wn_fwd<bf16_t, 1>(a, B, c, st) : launch_wn_fwd<bf16_t, 2>(a, B, c, st);
  return R == 32 ? launch_wn_fwd<float, 1>(a, B, c, st) : launch_wn_fwd<float, 2>(a, B, c, st);
}

extern "C" int srwn_wavenet_layer_bwd(const void* g_in, const void* d_up, const void* wconvT_up, void* g_out,
                                      const void* wresT, const void* wskipT, const void* dtotal, const void* dcs,
                                      const void* z, const void* s, void* d_out, int32_t B, int32_t T, int32_t R,
                                      int32_t S, int32_t K, int32_t dilation_up, int32_t has_up, int32_t has_down,
                                      int32_t dtype, void* stream) {
  if (has_up != 0 && has_up != 1) return set_error(SRWN_E_SHAPE, "wavenet_layer_bwd: has_up=%d", has_up);
  if (!has_up && !has_down) return set_error(SRWN_E_SHAPE, "wavenet_layer_bwd: neither UP nor DOWN");
  if (has_up && (!d_up || !wconvT_up || !g_out)) return set_error(SRWN_E_NULL, "wavenet_layer_bwd: UP needs d_up, wconvT_up, g_out");
  if (has_down && (!z || !s || !d_out)) return set_error(SRWN_E_NULL, "wavenet_layer_bwd: DOWN needs z, s, d_out");
  if (has_down && !dcs && (!wskipT || !dtotal)) return set_error(SRWN_E_NULL, "wavenet_layer_bwd: DOWN needs dcs, or wskipT + dtotal");
  if (has_up && has_down && !wresT) return set_error(SRWN_E_NULL, "wavenet_layer_bwd: UP+DOWN needs wresT");
  if (B < 0 || T < 0 || (has_up && dilation_up < 1) || (has_down && !dcs && (S < 16 || S % 16)))
    return set_error(SRWN_E_SHAPE, "wavenet_layer_bwd: B=%d T=%d S=%d d=%d", B, T, S, dilation_up);
  if ((long long)B * ((T + 31) / 32) > 0x7fffffffLL) return set_error(SRWN_E_SHAPE, "wavenet_layer_bwd: too many tiles");
  if (K != kWnK) return set_error(SRWN_E_UNSUPPORTED, "wavenet_layer_bwd: filter_width %d (only 2 is built)", K);
  if (dtype != SRWN_BF16 && dtype != SRWN_F32) return set_error(SRWN_E_DTYPE, "wavenet_layer_bwd: dtype %d", dtype);
  if (R != 32 && R != 64) return set_error(SRWN_E_UNSUPPORTED, "wavenet_layer_bwd: dilation_channels %d (built: 32, 64)", R);
  if (B == 0 || T == 0) return 0;
  WnBwdArgs a{g_in, d_up, wconvT_up, g_out, wresT, wskipT, dtotal, has_down ? dcs : nullptr, z, s, d_out, T,
              has_up ? dilation_up : 1, (has_down && !dcs) ? S : 0, 0, 0, has_up, has_down};
  if (!has_up) a.g_in = nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SRWN_BF16) return R == 32 ? launch_wn_bwd<bf16_t, 1>(a, B, st) : launch_wn_bwd<bf16_t, 2>(a, B, st);
  return R == 32 ? launch_wn_bwd<float, 1>(a, B, st) : launch_wn_bwd<float, 2>(a, B, st);
}
