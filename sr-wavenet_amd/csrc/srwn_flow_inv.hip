// Inversion of one inverse-autoregressive flow of the Parallel-WaveNet student (model.py:456-487): audio -> noise.
//
// A flow maps x_in to x_out[t] = x_in[t] * exp(p0[t]) + p1[t], where (p0, p1)[t] = head(stack(RightShift(x_in)))[t] reads
// x_in[< t] only.  The forward direction is therefore parallel over t (the training path, the stream synthesizer) and the
// inverse is sequential: x_in[t] = (x_out[t] - p1[t]) * exp(-p0[t]) needs the stack's output at t, which needs the
// RECOVERED x_in[t-1], x_in[t-2].  One step is one pass through the flow's L layers -- exactly the work of one step of the
// queue-cached generator (srwn_gen.hip), whose machinery this kernel restates without the skip path, the 1x1 head chain
// and the samplers: per layer a ring of the last d_l + 1 layer inputs, the conditioned layer chain in registers, the
// conv + residual weight images of layer l + 1 streamed into LDS by LDS-DMA while layer l computes, one persistent
// workgroup (4 waves) per group of 32 streams (the 32 columns of the MFMA tiles).  Every wave runs the whole chain on the
// same operands (the layer images are issued by all four, a quarter of the pieces each); wave 0 writes the rings and the
// outputs.  The head (relu -> R x 2 product, model.py:451-452) is a sum over the lane's channels and one exchange between
// the two half-waves; the recovered sample stays in registers for the next step's entry conv.
#include "srwn_common.h"
#include "srwn_gen_ring.h"
#include "srwn_host.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

constexpr size_t kFlowInvLdsMax = 160 * 1024;   // LDS of one CU (gfx950): what one workgroup can be given

struct FlowInvArgs {
  const void* wcr;      // per layer: [conv image RT x 2KS (tap0 natural, tap1 permuted) | res image RT x KS (permuted)]
  const float* bias_f; const float* bias_r;   // [L][R]
  const float* init_w; const float* init_b;   // [2][R], [R]
  const float* flow_w; const float* flow_b;   // [R][2], [2]
  void* ring;           // layer input rings, element offsets ring_off[l], depth dil[l]+1 slots of [32][R]
  // y / x_in [B][Tout], prm [B][Tout][2] arrive shifted back by t0 rows (srwn_gen.hip, GenArgs): row t of them is the
  // launch's row t - t0, and the step loop keeps one counter
  const float* y; float* x_in; float* prm;
  // cond: cb_l of stream u and frame f at cond + l * cond_ls + (u * cond_frames + f) * cond_ld, R values of T
  const void* cond; int cond_frames; int pool; long long cond_ld; long long cond_ls;
  int B, Tout, nsteps, L, t0;   // nsteps: the END step t0 + n
  float* carry;         // [B][2] = (x_in[t0-1], x_in[t0-2]) in, (x_in[t0+n-1], x_in[t0+n-2]) out; NULL: zeros, none written
  long long ring_group_elems;
  int dil[kGenMaxLayers];
  long long ring_off[kGenMaxLayers];
};

template <typename T, int NBUF, int RT>
__global__ __launch_bounds__(256) void flow_invert_kernel(FlowInvArgs a) {
  constexpr int R = 32 * RT, KS = R / 16;
  constexpr int FB = sizeof(Frag<T>) * 64;
  constexpr int LAYER_FR = RT * 2 * KS + RT * KS;                // fragment images per layer (conv + res)
  constexpr int LAYER_B = LAYER_FR * FB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* wbuf = smem;                                             // [NBUF][LAYER_B]
  float* c_bf = reinterpret_cast<float*>(smem + NBUF * LAYER_B); // [L][R]
  float* c_br = c_bf + a.L * R;      // [L][R]
  float* c_iw = c_br + a.L * R;      // [2][R]
  float* c_ib = c_iw + 2 * R;        // [R]
  float* c_fw = c_ib + R;            // [R][2]
  float* c_fb = c_fw + 2 * R;        // [2]

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 31, half = lane >> 5;
  const int ug = blockIdx.x * 32 + col;                          // this lane's stream
  const bool uok = ug < a.B;
  const char* wcr = reinterpret_cast<const char*>(a.wcr);
  T* ring = reinterpret_cast<T*>(a.ring) + (size_t)blockIdx.x * a.ring_group_elems;   // one ring set per group
  int par = 0;   // which weight buffer holds the layer being computed (toggles every layer, across steps)

  for (int i = threadIdx.x; i < a.L * R; i += 256) { c_bf[i] = a.bias_f[i]; c_br[i] = a.bias_r[i]; }
  if (threadIdx.x < 2 * R) { c_iw[threadIdx.x] = a.init_w[threadIdx.x]; c_fw[threadIdx.x] = a.flow_w[threadIdx.x]; }
  if (threadIdx.x < R) c_ib[threadIdx.x] = a.init_b[threadIdx.x];
  if (threadIdx.x < 2) c_fb[threadIdx.x] = a.flow_b[threadIdx.x];
  // the last two recovered samples, in registers of every lane of every wave (all of them compute the same step)
  float a1 = 0.0f, a2 = 0.0f;
  if (a.carry && uok) { a1 = a.carry[2 * ug]; a2 = a.carry[2 * ug + 1]; }
  lds_dma_copy(wcr, wbuf, LAYER_B, wave, lane, 4);
  __syncthreads();

  // operands of one layer that do not depend on the current step's activations: the tap-0 window from the ring (written
  // d >= 1 steps ago) and cb_l of the current frame.  Loaded two layers ahead, unconditionally (clamped)
  struct Pre { Frag<T> xd[KS]; f32x4 cc[RT][4]; };
  const T* condp = reinterpret_cast<const T*>(a.cond);
  const int ucl = uok ? ug : (a.B - 1);                          // clamped stream for conditioning loads
  auto preload = [&](int l_, int t, Pre& p) {
    const int l = l_ < a.L ? l_ : a.L - 1;
    const int d = a.dil[l], depth = d + 1;
    const int td = t - d;
    const int slot = (td >= 0 ? td : 0) % depth;
    const T* rp = ring + a.ring_off[l] + ((size_t)slot * 32 + col) * R + 8 * half;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) p.xd[ks] = load_nat(rp + 16 * ks);
    const int fc = min(t / a.pool, a.cond_frames - 1);
    const T* ccp = condp + (size_t)l * a.cond_ls + ((size_t)ucl * a.cond_frames + fc) * a.cond_ld + 4 * half;
#pragma unroll
    for (int mt = 0; mt < RT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) p.cc[mt][g] = load4(ccp + 32 * mt + 8 * g);
  };

  for (int t = a.t0; t < a.nsteps; ++t) {
    const float yv = uok ? a.y[(size_t)ug * a.Tout + t] : 0.0f;   // read at the head, a whole stack away
    // ---- entry conv with RightShift (model.py:423-424) on the recovered samples, in the order of flow_entry_row
    float h[RT][16];
#pragma unroll
    for (int mt = 0; mt < RT; ++mt)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int n = 32 * mt + crow(q, half);
        h[mt][q] = fmaf(a1, c_iw[R + n], fmaf(a2, c_iw[n], c_ib[n]));
      }

    auto layer = [&](int l, const Pre& p, Pre& pfill, int lfill) {
      const int d = a.dil[l];
      const int depth = d + 1;
      const int buf = (NBUF == 2) ? par : 0;
      if (NBUF == 2) {   // stream the next layer's (or next step's first layer's) conv+res weights
        const int ln = (l + 1 < a.L) ? l + 1 : 0;
        lds_dma_copy(wcr + (size_t)ln * LAYER_B, wbuf + (par ^ 1) * LAYER_B, LAYER_B, wave, lane, 4);
        par ^= 1;
      }
      preload(lfill, t, pfill);   // issued AFTER the LDS-DMA
      Frag<T> xd[KS];
      const bool tap0 = (t - d) >= 0;   // zero before the clip starts
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) xd[ks] = tap0 ? p.xd[ks] : zero_frag<T>();
      // the layer's complete input = output of the layer below + cb_l, rounded once (srwn_residual_layer_fwd adds the
      // next layer's bias before storing); below layer 0 the entry conv's output was stored (rounded) first
#pragma unroll
      for (int mt = 0; mt < RT; ++mt)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float base = (l == 0) ? (float)(T)h[mt][q] : h[mt][q];
          h[mt][q] = base + p.cc[mt][q >> 2][q & 3];
        }
      // x_l[t] -> ring (one writer), and as the permuted-order B fragments of tap 1
      Frag<T> xc[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) xc[s].set(j, h[s >> 1][8 * (s & 1) + j]);
      if (wave == 0) {
        T* wp = ring + a.ring_off[l] + ((size_t)(t % depth) * 32 + col) * R;
#pragma unroll
        for (int mt = 0; mt < RT; ++mt)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            store4(wp + 32 * mt + 8 * g + 4 * half, h[mt][4 * g], h[mt][4 * g + 1], h[mt][4 * g + 2], h[mt][4 * g + 3]);
      }
      // in bf16 mode the residual operand is the rounded activation the training graph stored
#pragma unroll
      for (int mt = 0; mt < RT; ++mt)
#pragma unroll
        for (int q = 0; q < 16; ++q) h[mt][q] = xc[2 * mt + (q >> 3)].get(q & 7);

      const Frag<T>* lw = reinterpret_cast<const Frag<T>*>(wbuf + buf * LAYER_B) + lane;
      f32x16 accF[RT];
#pragma unroll
      for (int mt = 0; mt < RT; ++mt)
#pragma unroll
        for (int q = 0; q < 16; ++q) accF[mt][q] = c_bf[l * R + 32 * mt + crow(q, half)];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int mt = 0; mt < RT; ++mt) {
          mma(accF[mt], lw[(mt * 2 * KS + ks) * 64], xd[ks]);
          mma(accF[mt], lw[(mt * 2 * KS + KS + ks) * 64], xc[ks]);
        }
      Frag<T> cf[KS];
#pragma unroll
      for (int mt = 0; mt < RT; ++mt)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          float z = Math<T>::tanh_(accF[mt][q]);
          z = (float)(T)z;   // the training graph stores z in T and rebuilds the gate from it
          cf[2 * mt + (q >> 3)].set(q & 7, gate_of_z<T>(z));
        }
      f32x16 accR[RT];
#pragma unroll
      for (int mt = 0; mt < RT; ++mt)
#pragma unroll
        for (int q = 0; q < 16; ++q) accR[mt][q] = c_br[l * R + 32 * mt + crow(q, half)];
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int mt = 0; mt < RT; ++mt) mma(accR[mt], lw[(RT * 2 * KS + mt * KS + s) * 64], cf[s]);
#pragma unroll
      for (int mt = 0; mt < RT; ++mt)
#pragma unroll
        for (int q = 0; q < 16; ++q) h[mt][q] = (h[mt][q] + accR[mt][q]) * kSqrtHalf;
      __syncthreads();   // next layer's weights landed; ring write of this layer ordered before later reads
      if (NBUF == 1) {
        const int ln = (l + 1 < a.L) ? l + 1 : 0;
        lds_dma_copy(wcr + (size_t)ln * LAYER_B, wbuf, LAYER_B, wave, lane, 4);
        __syncthreads();
      }
    };

    // three rotating operand sets: layer l computes while l+1 and l+2 are in flight
    Pre p0, p1, p2;
    preload(0, t, p0);
    preload(1, t, p1);
    for (int l = 0; l < a.L; l += 3) {
      layer(l, p0, p2, l + 2);
      if (l + 1 >= a.L) break;
      layer(l + 1, p1, p0, l + 3);
      if (l + 2 >= a.L) break;
      layer(l + 2, p2, p1, l + 4);
    }

    // ---- head (model.py:451-452): prm = relu(x_L rounded to T) . flow_w + flow_b, in fp32.  A lane holds 16 RT of the
    // column's channels, its partner in the other half-wave the rest
    float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
    for (int mt = 0; mt < RT; ++mt)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int n = 32 * mt + crow(q, half);
        const float r = fmaxf((float)(T)h[mt][q], 0.0f);
        s0 = fmaf(r, c_fw[2 * n], s0);
        s1 = fmaf(r, c_fw[2 * n + 1], s1);
      }
    s0 += __shfl_xor(s0, 32, 64);
    s1 += __shfl_xor(s1, 32, 64);
    const float q0 = s0 + c_fb[0], q1 = s1 + c_fb[1];
    // ---- the inverse of the affine transform (model.py:479-483)
    const float x = uok ? (yv - q1) * expf(-q0) : 0.0f;
    if (wave == 0 && half == 0 && uok) {
      a.x_in[(size_t)ug * a.Tout + t] = x;
      if (a.prm) *reinterpret_cast<f32x2*>(a.prm + ((size_t)ug * a.Tout + t) * 2) = f32x2{q0, q1};
    }
    a2 = a1;
    a1 = x;
  }
  if (a.carry && wave == 0 && half == 0 && uok) *reinterpret_cast<f32x2*>(a.carry + 2 * ug) = f32x2{a1, a2};
}

template <typename T, int NBUF>
int flow_invert_launch(const FlowInvArgs& a, int R, unsigned groups, hipStream_t st) {
  const size_t lfr = (size_t)(R / 32) * 3 * (R / 16);   // fragment images per layer: conv RT x 2KS + residual RT x KS
  const size_t sh = NBUF * lfr * sizeof(Frag<T>) * 64 + (size_t)(2 * a.L * R + 5 * R + 2) * 4;
  if (sh > kFlowInvLdsMax)
    return set_error(SRWN_E_SHAPE, "flow_invert: the layer images and the constants of %d layers take %zu bytes of LDS "
                     "(a workgroup has %zu)", a.L, sh, kFlowInvLdsMax);
  auto kfn = R == 64 ? flow_invert_kernel<T, NBUF, 2> : flow_invert_kernel<T, NBUF, 1>;
  hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
  if (e != hipSuccess) return set_error((int)e, "flow_invert: LDS %zu: %s", sh, hipGetErrorString(e));
  hipLaunchKernelGGL(kfn, dim3(groups), dim3(256), sh, st, a);
  return check_launch("flow_invert");
}

}  // namespace

extern "C" int srwn_flow_invert(const void* wcr, const float* bias_f, const float* bias_r, const float* init_w,
                                const float* init_b, const float* flow_w, const float* flow_b, void* ring, const float* y,
                                float* x_in, float* prm, const int32_t* dilations, int32_t nlayers, int32_t B,
                                int32_t Tout, int32_t nsteps, int32_t R, int32_t K, const void* cond, int32_t cond_frames,
                                int32_t pool_stride, int64_t cond_ld, int64_t cond_layer_stride, int32_t dtype,
                                void* stream, int32_t t0, float* carry) {
  if (B == 0 || nsteps == 0) return 0;
  if (B < 0 || nsteps < 0 || t0 < 0 || nsteps > Tout || (int64_t)t0 + nsteps > INT32_MAX)
    return set_error(SRWN_E_SHAPE, "flow_invert: B=%d nsteps=%d Tout=%d t0=%d", B, nsteps, Tout, t0);
  if (t0 > 0 && !carry) return set_error(SRWN_E_NULL, "flow_invert: a launch that resumes at t0=%d needs the carry", t0);
  if (!wcr || !bias_f || !bias_r || !init_w || !init_b || !flow_w || !flow_b || !ring || !y || !x_in || !dilations || !cond)
    return set_error(SRWN_E_NULL, "flow_invert: null pointer");
  if ((R != 64 && R != 32) || K != 2)
    return set_error(SRWN_E_UNSUPPORTED, "flow_invert: built for R=64 or 32, K=2 (got R=%d K=%d)", R, K);
  if (dtype != SRWN_BF16 && dtype != SRWN_F32) return set_error(SRWN_E_DTYPE, "flow_invert: dtype %d", dtype);
  if (nlayers < 1 || nlayers > kGenMaxLayers) return set_error(SRWN_E_SHAPE, "flow_invert: layers=%d", nlayers);
  if (cond_frames < 1 || pool_stride < 1 || cond_ld < R || cond_layer_stride < 0 ||
      (int64_t)cond_frames * pool_stride < (int64_t)t0 + nsteps)
    return set_error(SRWN_E_SHAPE, "flow_invert: cond_frames=%d pool_stride=%d cond_ld=%lld cond_layer_stride=%lld for "
                     "steps [%d, %lld)", cond_frames, pool_stride, (long long)cond_ld, (long long)cond_layer_stride, t0,
                     (long long)t0 + nsteps);
  FlowInvArgs a;
  a.wcr = wcr; a.bias_f = bias_f; a.bias_r = bias_r; a.init_w = init_w; a.init_b = init_b; a.flow_w = flow_w;
  a.flow_b = flow_b; a.ring = ring;
  // the shifted row pointers of the resume form (never dereferenced below row t0)
  const ptrdiff_t sh = (ptrdiff_t)t0;
  a.y = y - sh; a.x_in = x_in - sh; a.prm = prm ? prm - 2 * sh : nullptr;
  a.cond = cond; a.cond_frames = cond_frames; a.pool = pool_stride; a.cond_ld = cond_ld; a.cond_ls = cond_layer_stride;
  a.B = B; a.Tout = Tout; a.nsteps = t0 + nsteps; a.L = nlayers; a.t0 = t0; a.carry = carry;
  int bad;
  a.ring_group_elems = gen_ring_layout(dilations, nlayers, R, INT32_MAX, &bad, a.dil, a.ring_off);
  if (bad >= 0) return set_error(SRWN_E_SHAPE, "flow_invert: dilation %d", dilations[bad]);
  const unsigned groups = (unsigned)((B + 31) / 32);
  hipStream_t st = (hipStream_t)stream;
  // bf16: double-buffered layer images; fp32 (twice the bytes): one buffer, refilled behind the layer's barrier
  if (dtype == SRWN_BF16) return flow_invert_launch<bf16_t, 2>(a, R, groups, st);
  return flow_invert_launch<float, 1>(a, R, groups, st);
}
