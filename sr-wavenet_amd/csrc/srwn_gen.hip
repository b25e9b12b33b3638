// Queue-cached incremental (autoregressive) generation for the mu-law softmax teacher and for the conditioned
// mixture-of-logistics decoder of WaveNetAutoEncoder (the teacher generator.py:150-170 / teacher.py:140-171 sample
// from with a whole-clip pass per sample).
//
// The reference has no fast generator: its only sampler re-runs the whole clip once per
// generated sample (teacher.py:140-171, O(T^2 L)).  This kernel keeps, per layer, a ring of the last
// d_l + 1 layer inputs and produces one sample per step with exactly the arithmetic of the training
// graph (ops.py:23-46, model.py:158-196 with RightShift), so step t's logits equal the full forward's
// logits[:, t] on the same prefix -- the property the parity test pins.
//
// One persistent workgroup (4 waves) serves a group of up to 32 utterances (grid = number of groups): the 32 utterances are the 32 columns of
// the MFMA tiles, so a step costs the same MFMAs for 1 or 32 voices.  Per layer every wave runs the tiny
// conv -> gate -> residual chain redundantly in registers (no intra-layer exchange) and owns one quarter
// (64 channels) of the skip / head products; conv+residual weights of layer l+1 stream into LDS by LDS-DMA
// while layer l computes; skip/head weights are read straight from L2 (each wave uses distinct rows).
#include <cstdlib>
#include <type_traits>
#include "srwn_common.h"
#include "srwn_gen_ring.h"
#include "srwn_host.h"
#include "srwn_sample.h"
#include "../../include/srwn.h"

using namespace srwn;

struct GenArgs {
  const void* wcr;      // per layer: [conv image RT x 2KS (tap0 natural, tap1 permuted) | res image RT x KS (permuted)]
  const void* wskip;    // [S/32][L*R/16] permuted k order (B operand = gate tile in registers)
  const void* w1;       // [S/32][S/16] natural
  const void* w2;       // [Cp/32][S/16] natural
  const float* bias_f; const float* bias_r;   // [L][R]
  const float* bs_sum; const float* b1; const float* b2;   // [S], [S], [Cp]
  const float* init_w; const float* init_b;   // [2][R], [R]
  void* ring;           // layer input rings, element offsets ring_off[l], depth dil[l]+1 slots of [32][R]
  float* audio_out; int32_t* codes_out; float* logits_out; const float* forced;
  int B, Tout, nsteps, L, C, mode, Q;
  // conditioning (model.py:180-183): cond [B*frames, cond_ld] holds cb of every layer at columns [l*R, (l+1)*R);
  // layer l adds row (u, t / pool) to its input, rounded to T like the training kernel.  NULL = unconditioned.
  const void* cond; int cond_frames; int pool; long long cond_ld;
  int M;                // > 0: mixture-of-logistics head with M mixtures (C = 4M logits) instead of the softmax
  // resume form: the launch runs the absolute steps t0 <= t < nsteps (here: the END step t0 + n) -- ring slots, the
  // delayed-tap test, the conditioning frame and the RNG counters see t; audio_out / codes_out / logits_out / forced arrive
  // shifted back by t0 rows, so that row t of them is the launch's row t - t0 and the step loop keeps no second counter
  // (one more live scalar spilled SGPRs to scratch).  carry [B][2] = (a[t0-1], a[t0-2]) in, (a[t0+n-1], a[t0+n-2]) out --
  // the input samples the next step reads: forced ones where forced, else emitted ones.  t0 = 0 / NULL: the one-shot call
  int t0; float* carry;
  long long ring_group_elems;
  unsigned long long seed;
  int dil[kGenMaxLayers];
  long long ring_off[kGenMaxLayers];
};
// the slot form (generation pools, srwn.h SrwnGenSlot): t0 is the pool's clock; a struct of its own, so that the other
// instantiations keep their arguments
struct GenSlotArgs : GenArgs { SrwnGenSlot* slots; };
// the forms with sampling controls (srwn.h, SrwnGenSampling): instantiations of their own with the per-utterance array, so
// that a launch without controls runs the kernels it ran before
struct GenSampArgs : GenArgs { const SrwnGenSampling* sampling; };
struct GenSlotSampArgs : GenSlotArgs { const SrwnGenSampling* sampling; };
template <bool SLOTS, bool SAMP> struct GenArgsOf {
  using type = typename std::conditional<SLOTS, typename std::conditional<SAMP, GenSlotSampArgs, GenSlotArgs>::type,
                                         typename std::conditional<SAMP, GenSampArgs, GenArgs>::type>::type;
};

// the carry a launch leaves for the next one (its last __syncthreads ordered prev): the samples step t_end reads, i.e. the
// emitted ones of a free-running launch, the forced ones of a forced launch (prev[] holds the emitted ones there; after a
// single step its older entry is still the carried a[t0-1]).  `forced` is shifted back by t0 rows like the outputs.
__device__ __forceinline__ void gen_carry_out(float* carry, const float* forced, const float* prev, int u, int ul, int B,
                                              int Tout, int t0, int t_end) {
  if (u >= B) return;
  float c0 = prev[ul], c1 = prev[32 + ul];
  if (forced) {
    c0 = forced[(size_t)u * Tout + t_end - 1];
    if (t_end - t0 >= 2) c1 = forced[(size_t)u * Tout + t_end - 2];
  }
  carry[2 * u] = c0;
  carry[2 * u + 1] = c1;
}

template <typename T, int RT> struct GenCond { f32x4 cc[RT][4]; };
struct GenNoCond {};

// RING (the live form, srwn.h: srwn_generate_mol_live_sampled): the conditioning table is a ring of cond_frames rows per
// utterance that the caller keeps feeding; instantiations of their own, so that every other launch keeps its code.
// SLOTS && RING (the live slot form, srwn.h: srwn_generate_mol_live_slots_sampled): each slot's table rows are a ring read
// at the slot's OWN frame, and a column stores into the layer rings only while its slot runs -- a slot that has used up
// its frames keeps its ring rows as its last own step left them, for srwn_generate_ring_rotate_slots to realign
template <typename T, int NBUF, bool COND, int RT, int SS, bool SLOTS = false, bool SAMP = false, bool RING = false>
__global__ __launch_bounds__(256) void generate_kernel(typename GenArgsOf<SLOTS, SAMP>::type a) {
  constexpr int R = 32 * RT, KS = R / 16, S = SS, SQ = S / 4;   // SQ: skip/head-1 channels per wave
  constexpr int MQ = SQ / 32;                                    // ... = MQ 32-row tiles per wave
  constexpr int LGS = 256;                                       // row stride of the logits exchange (C <= 256)
  constexpr int FB = sizeof(Frag<T>) * 64;
  constexpr int LAYER_FR = RT * 2 * KS + RT * KS;                // 24 fragment images per layer (conv + res)
  constexpr int LAYER_B = LAYER_FR * FB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* wbuf = smem;                                             // [NBUF][LAYER_B]
  T* xch = reinterpret_cast<T*>(smem + NBUF * LAYER_B);          // [32][S] activation exchange (r0 / r1)
  float* lgl = reinterpret_cast<float*>(xch + 32 * S);           // [32][LGS] logits
  float* prev = lgl + 32 * LGS;                                  // [2][32] last two samples (starting as the carry)
  float* cst = prev + 64;                                        // constants: biases of every layer + head + input conv
  float* c_bf = cst;                 // [L][R]
  float* c_br = c_bf + a.L * R;      // [L][R]
  float* c_bs = c_br + a.L * R;      // [S]
  float* c_b1 = c_bs + S;            // [S]
  float* c_b2 = c_b1 + S;            // [LGS]
  float* c_iw = c_b2 + LGS;          // [2][R]
  float* c_ib = c_iw + 2 * R;        // [R]
  float* c_dec = c_ib + R;           // [256] mu-law decode of every code (ops.py:96-104 has a pow(): one table per launch)
  int* sl = reinterpret_cast<int*>(c_dec + 256);   // slot form: [5][32] t, steps run, seed lo, seed hi, current frame
  int* sc = sl + (SLOTS ? 5 * 32 : 0);             // sampling controls: [4][32] tau, top_p (floats), top_k, on

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 31, half = lane >> 5;
  const int u0 = blockIdx.x * 32;                                // first utterance of this workgroup's group
  const int ug = u0 + col;                                       // this lane's utterance
  const bool uok = ug < a.B;
  const char* wcr = reinterpret_cast<const char*>(a.wcr);
  const Frag<T>* wskip = reinterpret_cast<const Frag<T>*>(a.wskip);
  const Frag<T>* w1 = reinterpret_cast<const Frag<T>*>(a.w1);
  const Frag<T>* w2 = reinterpret_cast<const Frag<T>*>(a.w2);
  const int ks_skip = a.L * KS;
  T* ring = reinterpret_cast<T*>(a.ring) + (size_t)blockIdx.x * a.ring_group_elems;   // one ring set per group
  int par = 0;   // which weight buffer holds the layer being computed (toggles every layer, across steps)

  for (int i = threadIdx.x; i < a.L * R; i += 256) { c_bf[i] = a.bias_f[i]; c_br[i] = a.bias_r[i]; }
  for (int i = threadIdx.x; i < S; i += 256) { c_bs[i] = a.bs_sum[i]; c_b1[i] = a.b1[i]; }
  for (int i = threadIdx.x; i < LGS; i += 256)
    c_b2[i] = (i < (a.C + 31) / 32 * 32) ? a.b2[i] : 0.0f;     // the last 1x1 has ceil(C/32)*32 rows
  if (threadIdx.x < 2 * R) c_iw[threadIdx.x] = a.init_w[threadIdx.x];
  if (threadIdx.x < R) c_ib[threadIdx.x] = a.init_b[threadIdx.x];
  if (threadIdx.x < 64) {
    const int u = u0 + (threadIdx.x & 31);
    prev[threadIdx.x] = (a.carry && u < a.B) ? a.carry[2 * u + (threadIdx.x >> 5)] : 0.0f;
  }
  if (a.Q >= 2) c_dec[threadIdx.x] = gen_mu_law_decode(threadIdx.x < a.Q ? threadIdx.x : a.Q - 1, a.Q);
  if constexpr (SLOTS) {   // the group's slots, read once (a.nsteps is the END step here: the launch runs a.nsteps - t0)
    if (threadIdx.x < 32) {
      const int u = u0 + threadIdx.x;
      int st = 0, sn = 0;
      unsigned long long sd = 0;
      if (u < a.B) {
        const SrwnGenSlot g = a.slots[u];
        const long long left = (long long)g.t_end - g.t;
        const int n = a.nsteps - a.t0;
        st = g.t; sd = g.seed;
        sn = left <= 0 ? 0 : (left < n ? (int)left : n);
      }
      sl[threadIdx.x] = st; sl[32 + threadIdx.x] = sn;
      sl[64 + threadIdx.x] = (int)(unsigned)sd; sl[96 + threadIdx.x] = (int)(unsigned)(sd >> 32);
      if constexpr (COND && RING) sl[128 + threadIdx.x] = gen_ring_row(st / a.pool, a.cond_frames);
      else if constexpr (COND) sl[128 + threadIdx.x] = max(min(st / a.pool, a.cond_frames - 1), 0);
    }
  }
  if constexpr (SAMP) {   // the group's controls, sanitised, read once (mode 0 ignores them)
    if (threadIdx.x < 32) {
      const int u = u0 + threadIdx.x;
      samp::Ctl c{1.0f, 1.0f, 0, 0};
      if (u < a.B && a.mode == 1) c = samp::sanitise(a.sampling, u, a.C);
      sc[threadIdx.x] = __builtin_bit_cast(int, c.tau); sc[32 + threadIdx.x] = __builtin_bit_cast(int, c.top_p);
      sc[64 + threadIdx.x] = c.top_k; sc[96 + threadIdx.x] = c.on;
    }
  }
  lds_dma_copy(wcr, wbuf, LAYER_B, wave, lane, 4);
  __syncthreads();
  // slot form: the seed of local utterance ul, its own step at absolute step t, and whether it runs at step t
  auto slot_seed = [&](int ul) {
    return (unsigned long long)(unsigned)sl[64 + ul] | ((unsigned long long)(unsigned)sl[96 + ul] << 32);
  };
  auto slot_t = [&](int ul, int t) { return (int)((unsigned)sl[ul] + (unsigned)(t - a.t0)); };
  auto live = [&](int ul, int t) {
    if constexpr (SLOTS) return t - a.t0 < sl[32 + ul];
    else return true;
  };

  // operands of one layer that do not depend on the current step's activations: the tap-0 window from
  // the ring (written d >= 1 steps ago) and this wave's skip-weight fragments (from L2).  Loaded two
  // layers ahead, unconditionally (clamped), so their latency hides behind the dependent MFMA chain.
  // (the conditioning operands exist only in the COND instantiation: they cost 32 VGPRs per operand set)
  struct Pre : std::conditional<COND, GenCond<T, RT>, GenNoCond>::type { Frag<T> xd[KS]; Frag<T> ws[MQ][KS]; };
  const T* condp = COND ? reinterpret_cast<const T*>(a.cond) : nullptr;
  const int ucl = uok ? ug : (a.B - 1);                          // clamped utterance for conditioning loads
  auto preload = [&](int l_, int t, Pre& p) {
    const int l = l_ < a.L ? l_ : a.L - 1;
    const int d = a.dil[l], depth = d + 1;
    const int td = t - d;
    // (slot form: a true modulus -- a primed slot has real history while the clock is still below d)
    const int slot = SLOTS ? (td >= 0 ? td % depth : td + depth) : (td >= 0 ? td : 0) % depth;
    const T* rp = ring + a.ring_off[l] + ((size_t)slot * 32 + col) * R + 8 * half;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) p.xd[ks] = load_nat(rp + 16 * ks);
    if constexpr (COND) {   // cb_l of the current frame (accumulator layout); the ring holds conditioned inputs
      int fc = min(t / a.pool, a.cond_frames - 1);
      if constexpr (SLOTS) fc = sl[128 + col];   // the slot's own frame at step t (one division per step, not per layer)
      // the live form: frame q sits in row q mod cond_frames.  Every preload of this body is issued for the step that is
      // running (the `t` above is the step loop's, also for the sets filled two layers ahead), so no lookup reads a frame
      // ahead of the step: the row is always one the caller has fed
      if constexpr (RING && !SLOTS) fc = (t / a.pool) % a.cond_frames;
      const T* ccp = condp + ((size_t)ucl * a.cond_frames + fc) * a.cond_ld + (size_t)l * R + 4 * half;
#pragma unroll
      for (int mt = 0; mt < RT; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) p.cc[mt][g] = load4(ccp + 32 * mt + 8 * g);
    }
#pragma unroll
    for (int m = 0; m < MQ; ++m)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) p.ws[m][ks] = wskip[((size_t)(MQ * wave + m) * ks_skip + l * KS + ks) * 64 + lane];
  };

  for (int t = a.t0; t < a.nsteps; ++t) {
    // ---- input conv with RightShift (model.py:172-173): h0[t] = w[0]*audio[t-2] + w[1]*audio[t-1] + b
    // (prev[] starts as the carry, so a forced launch's first two steps read it there: shifted, the carried a[t0-1]
    // is prev[32 + col] at step t0 + 1)
    float a1 = 0.0f, a2 = 0.0f;
    if (uok) {
      if (a.forced) {
        a1 = (t >= a.t0 + 1) ? a.forced[(size_t)ug * a.Tout + t - 1] : prev[col];
        a2 = (t >= a.t0 + 2) ? a.forced[(size_t)ug * a.Tout + t - 2] : prev[32 + col];
      } else {
        a1 = prev[col];
        a2 = prev[32 + col];
      }
    }
    float h[RT][16];
#pragma unroll
    for (int mt = 0; mt < RT; ++mt)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int n = 32 * mt + crow(q, half);
        h[mt][q] = fmaf(c_iw[n], a2, fmaf(c_iw[R + n], a1, c_ib[n]));
      }
    f32x16 accS[MQ];
#pragma unroll
    for (int m = 0; m < MQ; ++m)
#pragma unroll
      for (int q = 0; q < 16; ++q) accS[m][q] = c_bs[SQ * wave + 32 * m + crow(q, half)];

    auto layer = [&](int l, const Pre& p, Pre& pfill, int lfill) {
      const int d = a.dil[l];
      const int depth = d + 1;
      const int buf = (NBUF == 2) ? par : 0;
      if (NBUF == 2) {   // stream the next layer's (or next step's first layer's) conv+res weights
        const int ln = (l + 1 < a.L) ? l + 1 : 0;
        lds_dma_copy(wcr + (size_t)ln * LAYER_B, wbuf + (par ^ 1) * LAYER_B, LAYER_B, wave, lane, 4);
        par ^= 1;
      }
      preload(lfill, t, pfill);   // issued AFTER the LDS-DMA so the counted wait below leaves it in flight
      Frag<T> xd[KS];
      const bool tap0 = SLOTS || (t - d) >= 0;   // zero before the clip starts (slot form: the rings hold the padding)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) xd[ks] = tap0 ? p.xd[ks] : zero_frag<T>();
      if constexpr (COND) {
        // the layer's complete input = output of the layer below + cb_l, rounded once (srwn_residual_layer_fwd adds
        // the next layer's bias before storing); below layer 0 the input conv's output was stored (rounded) first
#pragma unroll
        for (int mt = 0; mt < RT; ++mt)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const float base = (l == 0) ? (float)(T)h[mt][q] : h[mt][q];
            h[mt][q] = base + p.cc[mt][q >> 2][q & 3];
          }
      }
      // x_l[t] -> ring (one writer), and as the permuted-order B fragments of tap 1
      Frag<T> xc[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) xc[s].set(j, h[s >> 1][8 * (s & 1) + j]);
      // (live slot form: only while the column's slot runs at this step -- an idle column computes on junk as in the slot
      // form, but leaves its ring rows alone)
      if (wave == 0 && (!(SLOTS && RING) || live(col, t))) {   // one writer per ring slot
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
      // this wave's quarter of the skip 1x1 (ops.py:44), accumulated over layers (model.py:50)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int m = 0; m < MQ; ++m) mma(accS[m], p.ws[m][ks], cf[ks]);
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

    // ---- head: relu(sum skip) -> 1x1 + relu -> 1x1 (model.py:51-56); quarters exchanged through LDS
#pragma unroll
    for (int m = 0; m < MQ; ++m)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        store4(xch + col * S + SQ * wave + 32 * m + 8 * g + 4 * half, fmaxf(accS[m][4 * g], 0.f),
               fmaxf(accS[m][4 * g + 1], 0.f), fmaxf(accS[m][4 * g + 2], 0.f), fmaxf(accS[m][4 * g + 3], 0.f));
    __syncthreads();
    f32x16 acc1[MQ];
#pragma unroll
    for (int m = 0; m < MQ; ++m)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc1[m][q] = c_b1[SQ * wave + 32 * m + crow(q, half)];
#pragma unroll
    for (int ks = 0; ks < S / 16; ++ks) {
      const Frag<T> bf = load_nat(xch + col * S + 16 * ks + 8 * half);
#pragma unroll
      for (int m = 0; m < MQ; ++m) mma(acc1[m], w1[((size_t)(MQ * wave + m) * (S / 16) + ks) * 64 + lane], bf);
    }
    __syncthreads();   // everyone has read r0
#pragma unroll
    for (int m = 0; m < MQ; ++m)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        store4(xch + col * S + SQ * wave + 32 * m + 8 * g + 4 * half, fmaxf(acc1[m][4 * g], 0.f),
               fmaxf(acc1[m][4 * g + 1], 0.f), fmaxf(acc1[m][4 * g + 2], 0.f), fmaxf(acc1[m][4 * g + 3], 0.f));
    __syncthreads();
    f32x16 acc2[2];
    const int cp_pad = (a.C + 31) / 32 * 32;   // rows of the last 1x1's image (256 for the softmax head, 4M padded for MoL)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc2[m][q] = c_b2[64 * wave + 32 * m + crow(q, half)];   // 2 class tiles per wave
#pragma unroll
    for (int ks = 0; ks < S / 16; ++ks) {
      const Frag<T> bf = load_nat(xch + col * S + 16 * ks + 8 * half);
#pragma unroll
      for (int m = 0; m < 2; ++m)
        if (32 * (2 * wave + m) < cp_pad) mma(acc2[m], w2[((size_t)(2 * wave + m) * (S / 16) + ks) * 64 + lane], bf);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<f32x4*>(lgl + col * LGS + 64 * wave + 32 * m + 8 * g + 4 * half) =
            f32x4{acc2[m][4 * g], acc2[m][4 * g + 1], acc2[m][4 * g + 2], acc2[m][4 * g + 3]};
    __syncthreads();

    if (a.M > 0) {
      // ---- mixture-of-logistics head (model.py:196-198): sample_from_discretized_mix_logistic (ops.py:178-201) with
      //      counter-based uniforms; lanes = utterances (M <= 16 mixtures: a short serial loop)
      if (wave == 0 && half == 0) {
        const float* l = lgl + col * LGS;
        // slot form: the slot's seed and own step under utterance key 0 (what a batch-of-one run draws)
        const unsigned long long sseed = SLOTS ? slot_seed(col) : a.seed;
        const unsigned su = SLOTS ? 0u : (unsigned)ug;
        const int tu = SLOTS ? slot_t(col, t) : t;
        int sel = 0;
        float best = -INFINITY;
        for (int m = 0; m < a.M; ++m) {
          const float u1 = 1e-5f + (1.0f - 2e-5f) * gen_uniform(sseed, su, (unsigned)(tu * (a.M + 1) + m));
          float v = l[m] - logf(-logf(u1));
          if constexpr (SAMP) v = l[m] / __builtin_bit_cast(float, sc[col]) - logf(-logf(u1));   // (tau = 1: the same bits)
          if (v > best) { best = v; sel = m; }
        }
        float smp = l[a.M + sel];                                  // mode 0: the selected mean (no logistic noise)
        if (a.mode == 1) {
          const float u2 = 1e-5f + (1.0f - 2e-5f) * gen_uniform(sseed, su, (unsigned)(tu * (a.M + 1) + a.M));
          float sc_ = expf(fmaxf(l[2 * a.M + sel], -7.0f));
          if constexpr (SAMP) sc_ = __builtin_bit_cast(float, sc[col]) * sc_;      // the temperature on the logistic noise
          smp += sc_ * (logf(u2) - logf(1.0f - u2));
        }
        // slot form: the frame table of step t + 1 (every preload of step t is behind the head's barriers, the step's last
        // one orders this before the next; clamped at 0 too: an idle slot may hold any t).  Conditioning comes with this
        // head only: the conditioned softmax teacher is not built
        // (live slot form: the ring row of that frame, which after a starved slot's last step may be one not fed yet -- the
        // modulus keeps it inside the table, the column is idle at that step and the next launch computes its own)
        if constexpr (SLOTS && COND && RING) sl[128 + col] = gen_ring_row(slot_t(col, t + 1) / a.pool, a.cond_frames);
        else if constexpr (SLOTS && COND) sl[128 + col] = max(min(slot_t(col, t + 1) / a.pool, a.cond_frames - 1), 0);
        smp = fminf(fmaxf(smp, -1.0f), 1.0f);
        if (live(col, t)) {
          if (uok) {
            a.audio_out[(size_t)ug * a.Tout + t] = smp;
            a.codes_out[(size_t)ug * a.Tout + t] = sel;
          }
          prev[32 + col] = prev[col];
          prev[col] = smp;
        }
      }
      if (a.logits_out) {
        for (int i = threadIdx.x; i < 32 * a.C; i += 256) {
          const int ul = i / a.C, c = i - ul * a.C;
          if (u0 + ul < a.B && live(ul, t)) a.logits_out[((size_t)(u0 + ul) * a.Tout + t) * a.C + c] = lgl[ul * LGS + c];
        }
      }
      __syncthreads();
      continue;
    }
    // ---- softmax over the C classes, pick a code, mu-law decode: wave w serves utterances 8w..8w+7 with
    //      lanes = classes (4 per lane: conflict-free LDS rows, shuffle reductions instead of serial loops)
    for (int i = 0; i < 8; ++i) {
      const int ul = 8 * wave + i;                        // wave-uniform, local to the group
      const int u = u0 + ul;
      const f32x4 v = *reinterpret_cast<const f32x4*>(lgl + ul * LGS + 4 * lane);
      float m = -INFINITY; int am = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * lane + e < a.C && v[e] > m) { m = v[e]; am = 4 * lane + e; }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float mo = __shfl_xor(m, off); const int ao = __shfl_xor(am, off);
        if (mo > m || (mo == m && ao < am)) { m = mo; am = ao; }
      }
      int code = am;
      if (a.mode == 1) {   // categorical sample from softmax(logits): inclusive prefix sums over the lanes
        float ev[4], loc = 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) { ev[e] = (4 * lane + e < a.C) ? __expf(v[e] - m) : 0.0f; loc += ev[e]; }
        float inc = loc;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const float o = __shfl_up(inc, off);
          if (lane >= off) inc += o;
        }
        const float total = __shfl(inc, 63);
        const float target = (SLOTS ? gen_uniform(slot_seed(ul), 0u, (unsigned)slot_t(ul, t))
                                    : gen_uniform(a.seed, (unsigned)u, (unsigned)t)) * total;
        const unsigned long long hit = __ballot(inc > target);
        const int src = hit ? (__ffsll((long long)hit) - 1) : 63;
        float run = inc - loc;
        int pick = 4 * lane + 3;
#pragma unroll
        for (int e = 3; e >= 0; --e) { if (run + ev[0] + (e > 0 ? ev[1] : 0.f) + (e > 1 ? ev[2] : 0.f) + (e > 2 ? ev[3] : 0.f) > target) pick = 4 * lane + e; }
        if (pick >= a.C) pick = a.C - 1;
        code = __shfl(pick, src);
        if constexpr (SAMP) {
          // an utterance with controls: temperature / top-k / nucleus selection on its row (srwn_sample.h) behind a
          // wave-uniform branch; one at the defaults or an idle slot keeps the draw above
          if (__builtin_amdgcn_readfirstlane((int)(sc[96 + ul] != 0 && live(ul, t)))) {
            const float un = SLOTS ? gen_uniform(slot_seed(ul), 0u, (unsigned)slot_t(ul, t))
                                   : gen_uniform(a.seed, (unsigned)u, (unsigned)t);
            code = samp::filtered_code(v, a.C, __builtin_bit_cast(float, sc[ul]), sc[64 + ul],
                                       __builtin_bit_cast(float, sc[32 + ul]), un, lane);
          }
        }
      }
      if (lane == 0 && live(ul, t)) {
        const float smp = c_dec[code];
        if (u < a.B) {
          a.audio_out[(size_t)u * a.Tout + t] = smp;
          a.codes_out[(size_t)u * a.Tout + t] = code;
        }
        prev[32 + ul] = prev[ul];
        prev[ul] = smp;
      }
      if (a.logits_out && u < a.B && 4 * lane < a.C && live(ul, t)) {
        float* lo = a.logits_out + ((size_t)u * a.Tout + t) * a.C + 4 * lane;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (4 * lane + e < a.C) lo[e] = v[e];
      }
    }
    __syncthreads();
  }
  if constexpr (SLOTS) {   // the steps each slot ran (prev[] stopped with them); its own step advances by as many
    const int ul = threadIdx.x, u = u0 + ul;
    if (ul < 32 && u < a.B && sl[32 + ul] > 0) {
      gen_carry_out(a.carry, a.forced, prev, u, ul, a.B, a.Tout, a.t0, a.t0 + sl[32 + ul]);
      a.slots[u].t = sl[ul] + sl[32 + ul];
    }
  } else if (a.carry && threadIdx.x < 32) {
    gen_carry_out(a.carry, a.forced, prev, u0 + threadIdx.x, threadIdx.x, a.B, a.Tout, a.t0, a.nsteps);
  }
}

extern "C" int64_t srwn_generate_ring_elems(const int32_t* dilations, int32_t nlayers, int32_t R) {
  int bad;
  return gen_ring_layout(dilations, nlayers, R, INT32_MAX, &bad);   // per group of 32 utterances
}

template <bool SL, bool SA, bool RG = false, typename A>
static int generate_launch(A& a, int R, int S, bool cond, int dtype, int nlayers, unsigned groups, hipStream_t st) {
  const size_t lfr = (size_t)(R / 32) * 3 * (R / 16);   // fragment images per layer: conv RT x 2KS + residual RT x KS
  const size_t slot_lds = (SL ? 5 * 32 * 4 : 0) + (SA ? 4 * 32 * 4 : 0);   // the per-slot table, the sampling controls
  // widths: (64, 256) the north-star stack, (32, 256) generator.py's default teacher, (32, 128) teacher.py's
#define SRWN_GEN_PICK(TT, NB)                                                                                             \
  ((R == 64 && S == 256) ? (cond ? generate_kernel<TT, NB, true, 2, 256, SL, SA> : generate_kernel<TT, NB, false, 2, 256, SL, SA>)  \
   : (R == 32 && S == 256) ? (cond ? generate_kernel<TT, NB, true, 1, 256, SL, SA> : generate_kernel<TT, NB, false, 1, 256, SL, SA>) \
   : (R == 32 && S == 128) ? (cond ? generate_kernel<TT, NB, true, 1, 128, SL, SA> : generate_kernel<TT, NB, false, 1, 128, SL, SA>) \
                           : (cond ? generate_kernel<TT, NB, true, 2, 128, SL, SA> : generate_kernel<TT, NB, false, 2, 128, SL, SA>))
  // the live forms are conditioned (without slots, or the live slot form): their own instantiation of every width
#define SRWN_GEN_PICK_RING(TT, NB)                                                             \
  ((R == 64 && S == 256) ? generate_kernel<TT, NB, true, 2, 256, SL, SA, true>                 \
   : (R == 32 && S == 256) ? generate_kernel<TT, NB, true, 1, 256, SL, SA, true>               \
   : (R == 32 && S == 128) ? generate_kernel<TT, NB, true, 1, 128, SL, SA, true>               \
                           : generate_kernel<TT, NB, true, 2, 128, SL, SA, true>)
#define SRWN_GEN_KFN(TT, NB) [&] { if constexpr (RG) return SRWN_GEN_PICK_RING(TT, NB); else return SRWN_GEN_PICK(TT, NB); }()
  if (dtype == SRWN_BF16) {
    auto kfn = SRWN_GEN_KFN(bf16_t, 2);
    const size_t sh = 2 * lfr * sizeof(Frag<bf16_t>) * 64 + 32 * S * sizeof(bf16_t) + 32 * 256 * 4 + 64 * 4 +
                      (size_t)(2 * nlayers * R + 2 * S + 256 + 3 * R + 256) * 4 + slot_lds;
    hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    if (e != hipSuccess) return set_error((int)e, "generate: LDS %zu: %s", sh, hipGetErrorString(e));
    hipLaunchKernelGGL(kfn, dim3(groups), dim3(256), sh, st, a);
  } else if (dtype == SRWN_F32) {
    auto kfn = SRWN_GEN_KFN(float, 1);
    const size_t sh = 1 * lfr * sizeof(Frag<float>) * 64 + 32 * S * sizeof(float) + 32 * 256 * 4 + 64 * 4 +
                      (size_t)(2 * nlayers * R + 2 * S + 256 + 3 * R + 256) * 4 + slot_lds;
    hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    if (e != hipSuccess) return set_error((int)e, "generate: LDS %zu: %s", sh, hipGetErrorString(e));
    hipLaunchKernelGGL(kfn, dim3(groups), dim3(256), sh, st, a);
  } else {
    return set_error(SRWN_E_DTYPE, "generate: dtype %d", dtype);
  }
#undef SRWN_GEN_KFN
#undef SRWN_GEN_PICK_RING
#undef SRWN_GEN_PICK
  return check_launch("generate");
}

static int generate_impl(const void* wcr, const void* wskip, const void* w1, const void* w2, const float* bias_f,
                         const float* bias_r, const float* bs_sum, const float* b1, const float* b2,
                         const float* init_w, const float* init_b, void* ring, float* audio_out, int32_t* codes_out,
                         float* logits_out, const float* forced, const int32_t* dilations, int32_t nlayers, int32_t B,
                         int32_t Tout, int32_t nsteps, int32_t R, int32_t S, int32_t C, int32_t K, int32_t mode,
                         uint64_t seed, int32_t dtype, void* stream, const void* cond, int32_t cond_frames,
                         int32_t pool, int64_t cond_ld, int32_t M, int32_t t0, float* carry,
                         const SrwnGenSampling* sampling, SrwnGenSlot* slots = nullptr, bool slot_form = false,
                         bool ring_form = false) {
  // the mixture-of-logistics head (M > 0): its conditioning, checked before anything else as its entry points always did
  if (M > 0 && cond && (cond_frames < 1 || pool < 1 || cond_ld < (int64_t)nlayers * R))
    return set_error(SRWN_E_SHAPE, "%s: cond_frames=%d pool_stride=%d cond_ld=%lld",
                     slot_form ? "generate_mol_slots" : "generate_mol", cond_frames, pool, (long long)cond_ld);
  if (!cond) cond_frames = pool = 1;
  if (B == 0 || nsteps == 0) return 0;
  if (t0 < 0 || (int64_t)t0 + nsteps > INT32_MAX) return set_error(SRWN_E_SHAPE, "generate: t0=%d", t0);
  if (t0 > 0 && !carry) return set_error(SRWN_E_NULL, "generate: a launch that resumes at t0=%d needs the carry", t0);
  if (slot_form && (!carry || !slots)) return set_error(SRWN_E_NULL, "generate_slots: the carry and the slots are required");
  if (!wcr || !wskip || !w1 || !w2 || !bias_f || !bias_r || !bs_sum || !b1 || !b2 || !init_w || !init_b || !ring ||
      !audio_out || !codes_out || !dilations)
    return set_error(SRWN_E_NULL, "generate: null pointer");
  if ((R != 64 && R != 32) || (S != 256 && S != 128) || K != 2 || C < 2 || C > 256)
    return set_error(SRWN_E_UNSUPPORTED, "generate: built for R=64 or 32, S=256 or 128, K=2, C<=256 (got R=%d S=%d K=%d C=%d)", R, S, K, C);
  if (B < 0 || nsteps < 0 || nsteps > Tout || nlayers < 1 || nlayers > kGenMaxLayers || (mode != 0 && mode != 1))
    return set_error(SRWN_E_SHAPE, "generate: B=%d nsteps=%d Tout=%d layers=%d mode=%d", B, nsteps, Tout, nlayers, mode);
  GenSlotSampArgs a;   // (the other instantiations get its GenSlotArgs / GenArgs part)
  a.slots = slots;
  a.sampling = sampling;
  a.wcr = wcr; a.wskip = wskip; a.w1 = w1; a.w2 = w2; a.bias_f = bias_f; a.bias_r = bias_r; a.bs_sum = bs_sum;
  a.b1 = b1; a.b2 = b2; a.init_w = init_w; a.init_b = init_b; a.ring = ring; a.audio_out = audio_out;
  a.codes_out = codes_out; a.logits_out = logits_out; a.forced = forced;
  a.B = B; a.Tout = Tout; a.nsteps = nsteps; a.L = nlayers; a.C = C; a.mode = mode; a.Q = C; a.seed = seed;
  a.cond = cond; a.cond_frames = cond_frames; a.pool = pool; a.cond_ld = cond_ld; a.M = M;
  // the shifted row pointers of the resume form (never dereferenced below row t0)
  const ptrdiff_t sh = (ptrdiff_t)t0;
  a.audio_out = audio_out - sh; a.codes_out = codes_out - sh;
  a.logits_out = logits_out ? logits_out - sh * C : nullptr; a.forced = forced ? forced - sh : nullptr;
  a.nsteps = t0 + nsteps; a.t0 = t0; a.carry = carry;
  int bad;
  a.ring_group_elems = gen_ring_layout(dilations, nlayers, R, INT32_MAX, &bad, a.dil, a.ring_off);
  if (bad >= 0) return set_error(SRWN_E_SHAPE, "generate: dilation %d", dilations[bad]);
  const unsigned groups = (unsigned)((B + 31) / 32);
  hipStream_t st = (hipStream_t)stream;
  const bool cd = cond != nullptr;
  if (slot_form && ring_form) {
    if (sampling) return generate_launch<true, true, true>(a, R, S, cd, dtype, nlayers, groups, st);
    return generate_launch<true, false, true>(static_cast<GenSlotArgs&>(a), R, S, cd, dtype, nlayers, groups, st);
  }
  if (slot_form) {
    if (sampling) return generate_launch<true, true>(a, R, S, cd, dtype, nlayers, groups, st);
    return generate_launch<true, false>(static_cast<GenSlotArgs&>(a), R, S, cd, dtype, nlayers, groups, st);
  }
  if (sampling) {   // (no slots: the GenArgs part and the array)
    GenSampArgs b;
    static_cast<GenArgs&>(b) = a;
    b.sampling = sampling;
    if (ring_form) return generate_launch<false, true, true>(b, R, S, cd, dtype, nlayers, groups, st);
    return generate_launch<false, true>(b, R, S, cd, dtype, nlayers, groups, st);
  }
  if (ring_form) return generate_launch<false, false, true>(static_cast<GenArgs&>(a), R, S, cd, dtype, nlayers, groups, st);
  return generate_launch<false, false>(static_cast<GenArgs&>(a), R, S, cd, dtype, nlayers, groups, st);
}

extern "C" int srwn_generate_resume_sampled(const void* wcr, const void* wskip, const void* w1, const void* w2,
                                    const float* bias_f, const float* bias_r, const float* bs_sum, const float* b1,
                                    const float* b2, const float* init_w, const float* init_b, void* ring,
                                    float* audio_out, int32_t* codes_out, float* logits_out, const float* forced,
                                    const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps,
                                    int32_t R, int32_t S, int32_t C, int32_t K, int32_t mode, uint64_t seed,
                                    int32_t dtype, void* stream, int32_t t0, float* carry, const SrwnGenSampling* sampling) {
  return generate_impl(wcr, wskip, w1, w2, bias_f, bias_r, bs_sum, b1, b2, init_w, init_b, ring, audio_out, codes_out,
                       logits_out, forced, dilations, nlayers, B, Tout, nsteps, R, S, C, K, mode, seed, dtype, stream,
                       nullptr, 1, 1, 0, 0, t0, carry, sampling);
}

// (without sampling controls: the call above with NULL)
extern "C" int srwn_generate_resume(const void* wcr, const void* wskip, const void* w1, const void* w2,
                                    const float* bias_f, const float* bias_r, const float* bs_sum, const float* b1,
                                    const float* b2, const float* init_w, const float* init_b, void* ring,
                                    float* audio_out, int32_t* codes_out, float* logits_out, const float* forced,
                                    const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps,
                                    int32_t R, int32_t S, int32_t C, int32_t K, int32_t mode, uint64_t seed,
                                    int32_t dtype, void* stream, int32_t t0, float* carry) {
  return srwn_generate_resume_sampled(wcr, wskip, w1, w2, bias_f, bias_r, bs_sum, b1, b2, init_w, init_b, ring,
      audio_out, codes_out, logits_out, forced, dilations, nlayers, B, Tout, nsteps, R, S, C, K, mode, seed, dtype,
      stream, t0, carry, nullptr);
}

extern "C" int srwn_generate(const void* wcr, const void* wskip, const void* w1, const void* w2, const float* bias_f,
                             const float* bias_r, const float* bs_sum, const float* b1, const float* b2,
                             const float* init_w, const float* init_b, void* ring, float* audio_out,
                             int32_t* codes_out, float* logits_out, const float* forced, const int32_t* dilations,
                             int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps, int32_t R, int32_t S,
                             int32_t C, int32_t K, int32_t mode, uint64_t seed, int32_t dtype, void* stream) {
  return srwn_generate_resume(wcr, wskip, w1, w2, bias_f, bias_r, bs_sum, b1, b2, init_w, init_b, ring, audio_out,
                              codes_out, logits_out, forced, dilations, nlayers, B, Tout, nsteps, R, S, C, K, mode, seed,
                              dtype, stream, 0, nullptr);
}

// The conditioned mixture-of-logistics decoder (WaveNetAutoEncoder.createDecoder, model.py:158-200): cond
// [B*cond_frames, cond_ld] = the per-layer conditioning biases cb_l at columns [l*R, (l+1)*R) (srwn_pw_linear of
// encoding_w_condition, model.py:180); head = 4*num_mixtures logits, sampled as ops.py:178-201.  b2 and the w2
// image cover ceil(4M/32)*32 rows.  codes_out receives the selected mixture index.
extern "C" int srwn_generate_mol_resume_sampled(const void* wcr, const void* wskip, const void* w1, const void* w2,
                                        const float* bias_f, const float* bias_r, const float* bs_sum, const float* b1,
                                        const float* b2, const float* init_w, const float* init_b, void* ring,
                                        float* audio_out, int32_t* codes_out, float* logits_out, const float* forced,
                                        const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout,
                                        int32_t nsteps, int32_t R, int32_t S, int32_t K, int32_t num_mixtures,
                                        const void* cond, int32_t cond_frames, int32_t pool_stride, int64_t cond_ld,
                                        int32_t mode, uint64_t seed, int32_t dtype, void* stream, int32_t t0,
                                        float* carry, const SrwnGenSampling* sampling) {
  if (num_mixtures < 1 || num_mixtures > 16)
    return set_error(SRWN_E_SHAPE, "generate_mol: num_mixtures=%d (1..16)", num_mixtures);
  return generate_impl(wcr, wskip, w1, w2, bias_f, bias_r, bs_sum, b1, b2, init_w, init_b, ring, audio_out, codes_out,
                       logits_out, forced, dilations, nlayers, B, Tout, nsteps, R, S, 4 * num_mixtures, K, mode, seed,
                       dtype, stream, cond, cond_frames, pool_stride, cond_ld, num_mixtures, t0,
                       carry, sampling);
}

// (without sampling controls: the call above with NULL)
extern "C" int srwn_generate_mol_resume(const void* wcr, const void* wskip, const void* w1, const void* w2,
                                        const float* bias_f, const float* bias_r, const float* bs_sum, const float* b1,
                                        const float* b2, const float* init_w, const float* init_b, void* ring,
                                        float* audio_out, int32_t* codes_out, float* logits_out, const float* forced,
                                        const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout,
                                        int32_t nsteps, int32_t R, int32_t S, int32_t K, int32_t num_mixtures,
                                        const void* cond, int32_t cond_frames, int32_t pool_stride, int64_t cond_ld,
                                        int32_t mode, uint64_t seed, int32_t dtype, void* stream, int32_t t0,
                                        float* carry) {
  return srwn_generate_mol_resume_sampled(wcr, wskip, w1, w2, bias_f, bias_r, bs_sum, b1, b2, init_w, init_b, ring,
      audio_out, codes_out, logits_out, forced, dilations, nlayers, B, Tout, nsteps, R, S, K, num_mixtures, cond,
      cond_frames, pool_stride, cond_ld, mode, seed, dtype, stream, t0, carry, nullptr);
}

extern "C" int srwn_generate_mol(const void* wcr, const void* wskip, const void* w1, const void* w2,
                                 const float* bias_f, const float* bias_r, const float* bs_sum, const float* b1,
                                 const float* b2, const float* init_w, const float* init_b, void* ring,
                                 float* audio_out, int32_t* codes_out, float* logits_out, const float* forced,
                                 const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps,
                                 int32_t R, int32_t S, int32_t K, int32_t num_mixtures, const void* cond,
                                 int32_t cond_frames, int32_t pool_stride, int64_t cond_ld, int32_t mode, uint64_t seed,
                                 int32_t dtype, void* stream) {
  return srwn_generate_mol_resume(wcr, wskip, w1, w2, bias_f, bias_r, bs_sum, b1, b2, init_w, init_b, ring, audio_out,
                                  codes_out, logits_out, forced, dilations, nlayers, B, Tout, nsteps, R, S, K,
                                  num_mixtures, cond, cond_frames, pool_stride, cond_ld, mode, seed, dtype, stream, 0,
                                  nullptr);
}

// ---- the live form (srwn.h, srwn_version() 112): srwn_generate_mol_resume_sampled over a conditioning table that is a ring
// of cond_frames frames per utterance (frame q in row q mod cond_frames), fed while the run goes on.  `cond` is required
extern "C" int srwn_generate_mol_live_sampled(const void* wcr, const void* wskip, const void* w1, const void* w2,
                                      const float* bias_f, const float* bias_r, const float* bs_sum, const float* b1,
                                      const float* b2, const float* init_w, const float* init_b, void* ring,
                                      float* audio_out, int32_t* codes_out, float* logits_out, const float* forced,
                                      const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout,
                                      int32_t nsteps, int32_t R, int32_t S, int32_t K, int32_t num_mixtures,
                                      const void* cond, int32_t cond_frames, int32_t pool_stride, int64_t cond_ld,
                                      int32_t mode, uint64_t seed, int32_t dtype, void* stream, int32_t t0,
                                      float* carry, const SrwnGenSampling* sampling) {
  if (!cond) return set_error(SRWN_E_NULL, "generate_mol_live: the conditioning ring is required");
  if (num_mixtures < 1 || num_mixtures > 16)
    return set_error(SRWN_E_SHAPE, "generate_mol_live: num_mixtures=%d (1..16)", num_mixtures);
  if (cond_frames < 1 || pool_stride < 1 || cond_ld < (int64_t)nlayers * R)
    return set_error(SRWN_E_SHAPE, "generate_mol_live: cond_frames=%d pool_stride=%d cond_ld=%lld", cond_frames,
                     pool_stride, (long long)cond_ld);
  return generate_impl(wcr, wskip, w1, w2, bias_f, bias_r, bs_sum, b1, b2, init_w, init_b, ring, audio_out, codes_out,
                       logits_out, forced, dilations, nlayers, B, Tout, nsteps, R, S, 4 * num_mixtures, K, mode, seed,
                       dtype, stream, cond, cond_frames, pool_stride, cond_ld, num_mixtures, t0, carry, sampling, nullptr,
                       false, true);
}

// ---- the slot form (generation pools, srwn.h): the arguments of the *_resume twins without the seed, with the pool's
// clock as t0 and the per-slot state
extern "C" int srwn_generate_slots_sampled(const void* wcr, const void* wskip, const void* w1, const void* w2,
                                   const float* bias_f, const float* bias_r, const float* bs_sum, const float* b1,
                                   const float* b2, const float* init_w, const float* init_b, void* ring,
                                   float* audio_out, int32_t* codes_out, float* logits_out, const float* forced,
                                   const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps,
                                   int32_t R, int32_t S, int32_t C, int32_t K, int32_t mode, int32_t dtype, void* stream,
                                   int32_t clock, float* carry, SrwnGenSlot* slots, const SrwnGenSampling* sampling) {
  return generate_impl(wcr, wskip, w1, w2, bias_f, bias_r, bs_sum, b1, b2, init_w, init_b, ring, audio_out, codes_out,
                       logits_out, forced, dilations, nlayers, B, Tout, nsteps, R, S, C, K, mode, 0, dtype, stream,
                       nullptr, 1, 1, 0, 0, clock, carry, sampling, slots, true);
}

// (without sampling controls: the call above with NULL)
extern "C" int srwn_generate_slots(const void* wcr, const void* wskip, const void* w1, const void* w2,
                                   const float* bias_f, const float* bias_r, const float* bs_sum, const float* b1,
                                   const float* b2, const float* init_w, const float* init_b, void* ring,
                                   float* audio_out, int32_t* codes_out, float* logits_out, const float* forced,
                                   const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps,
                                   int32_t R, int32_t S, int32_t C, int32_t K, int32_t mode, int32_t dtype, void* stream,
                                   int32_t clock, float* carry, SrwnGenSlot* slots) {
  return srwn_generate_slots_sampled(wcr, wskip, w1, w2, bias_f, bias_r, bs_sum, b1, b2, init_w, init_b, ring,
      audio_out, codes_out, logits_out, forced, dilations, nlayers, B, Tout, nsteps, R, S, C, K, mode, dtype,
      stream, clock, carry, slots, nullptr);
}

extern "C" int srwn_generate_mol_slots_sampled(const void* wcr, const void* wskip, const void* w1, const void* w2,
                                       const float* bias_f, const float* bias_r, const float* bs_sum, const float* b1,
                                       const float* b2, const float* init_w, const float* init_b, void* ring,
                                       float* audio_out, int32_t* codes_out, float* logits_out, const float* forced,
                                       const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout,
                                       int32_t nsteps, int32_t R, int32_t S, int32_t K, int32_t num_mixtures,
                                       const void* cond, int32_t cond_frames, int32_t pool_stride, int64_t cond_ld,
                                       int32_t mode, int32_t dtype, void* stream, int32_t clock, float* carry,
                                       SrwnGenSlot* slots, const SrwnGenSampling* sampling) {
  if (num_mixtures < 1 || num_mixtures > 16)
    return set_error(SRWN_E_SHAPE, "generate_mol_slots: num_mixtures=%d (1..16)", num_mixtures);
  return generate_impl(wcr, wskip, w1, w2, bias_f, bias_r, bs_sum, b1, b2, init_w, init_b, ring, audio_out, codes_out,
                       logits_out, forced, dilations, nlayers, B, Tout, nsteps, R, S, 4 * num_mixtures, K, mode, 0,
                       dtype, stream, cond, cond_frames, pool_stride, cond_ld, num_mixtures, clock,
                       carry, sampling, slots, true);
}

// (without sampling controls: the call above with NULL)
extern "C" int srwn_generate_mol_slots(const void* wcr, const void* wskip, const void* w1, const void* w2,
                                       const float* bias_f, const float* bias_r, const float* bs_sum, const float* b1,
                                       const float* b2, const float* init_w, const float* init_b, void* ring,
                                       float* audio_out, int32_t* codes_out, float* logits_out, const float* forced,
                                       const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout,
                                       int32_t nsteps, int32_t R, int32_t S, int32_t K, int32_t num_mixtures,
                                       const void* cond, int32_t cond_frames, int32_t pool_stride, int64_t cond_ld,
                                       int32_t mode, int32_t dtype, void* stream, int32_t clock, float* carry,
                                       SrwnGenSlot* slots) {
  return srwn_generate_mol_slots_sampled(wcr, wskip, w1, w2, bias_f, bias_r, bs_sum, b1, b2, init_w, init_b, ring,
      audio_out, codes_out, logits_out, forced, dilations, nlayers, B, Tout, nsteps, R, S, K, num_mixtures, cond,
      cond_frames, pool_stride, cond_ld, mode, dtype, stream, clock, carry, slots, nullptr);
}

// ---- the live slot form (srwn.h, srwn_version() 114): srwn_generate_mol_slots_sampled over per-slot conditioning RINGS of
// cond_frames frames (a slot's own frame q in row q mod cond_frames), with the ring stores of idle columns held back
extern "C" int srwn_generate_mol_live_slots_sampled(const void* wcr, const void* wskip, const void* w1, const void* w2,
                                       const float* bias_f, const float* bias_r, const float* bs_sum, const float* b1,
                                       const float* b2, const float* init_w, const float* init_b, void* ring,
                                       float* audio_out, int32_t* codes_out, float* logits_out, const float* forced,
                                       const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout,
                                       int32_t nsteps, int32_t R, int32_t S, int32_t K, int32_t num_mixtures,
                                       const void* cond, int32_t cond_frames, int32_t pool_stride, int64_t cond_ld,
                                       int32_t mode, int32_t dtype, void* stream, int32_t clock, float* carry,
                                       SrwnGenSlot* slots, const SrwnGenSampling* sampling) {
  if (!cond) return set_error(SRWN_E_NULL, "generate_mol_live_slots: the conditioning ring is required");
  if (num_mixtures < 1 || num_mixtures > 16)
    return set_error(SRWN_E_SHAPE, "generate_mol_live_slots: num_mixtures=%d (1..16)", num_mixtures);
  if (cond_frames < 1 || pool_stride < 1 || cond_ld < (int64_t)nlayers * R)
    return set_error(SRWN_E_SHAPE, "generate_mol_live_slots: cond_frames=%d pool_stride=%d cond_ld=%lld", cond_frames,
                     pool_stride, (long long)cond_ld);
  return generate_impl(wcr, wskip, w1, w2, bias_f, bias_r, bs_sum, b1, b2, init_w, init_b, ring, audio_out, codes_out,
                       logits_out, forced, dilations, nlayers, B, Tout, nsteps, R, S, 4 * num_mixtures, K, mode, 0,
                       dtype, stream, cond, cond_frames, pool_stride, cond_ld, num_mixtures, clock,
                       carry, sampling, slots, true, true);
}

// ---- the rings after a prompt of P samples, from the layer inputs of ONE parallel forward pass over it (what the loop of
// teacher.py:140-171 would have left after P steps): slot s of layer l <- x_l[t], the t in [P-1-d_l, P-1] with
// t = s (mod d_l+1); zero where t < 0 or the utterance is past B (the causal padding the bodies rely on).  Memory-bound:
// one 16-byte vector per thread, consecutive threads along the R channels of a row, then rows, then slots.
struct RingFillArgs {
  const void* xs; void* ring;
  long long layer_stride, ring_group_elems;
  int T_src, P, B, R;
  int dil[kGenMaxLayers];
  long long ring_off[kGenMaxLayers];
};

template <typename T>
__global__ __launch_bounds__(256) void ring_fill_kernel(RingFillArgs a) {
  constexpr int V = 16 / sizeof(T);
  const int l = blockIdx.y, g = blockIdx.z;
  const int d = a.dil[l], depth = d + 1, vpr = a.R / V;
  const int nvec = depth * 32 * vpr;
  const int base = a.P - 1 - d;                                  // oldest step the ring still holds (may be < 0)
  const T* xp = reinterpret_cast<const T*>(a.xs) + (size_t)l * a.layer_stride;
  T* rp = reinterpret_cast<T*>(a.ring) + (size_t)g * a.ring_group_elems + a.ring_off[l];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nvec; i += gridDim.x * 256) {
    const int cv = i % vpr, r = i / vpr;                         // r = slot * 32 + row
    const int row = r & 31, s = r >> 5, u = 32 * g + row;
    int off = (s - base) % depth;
    if (off < 0) off += depth;
    const int t = base + off;
    uint4 v = {0u, 0u, 0u, 0u};
    if (t >= 0 && u < a.B) v = *reinterpret_cast<const uint4*>(xp + ((size_t)u * a.T_src + t) * a.R + cv * V);
    *reinterpret_cast<uint4*>(rp + (size_t)r * a.R + cv * V) = v;
  }
}

extern "C" int srwn_generate_ring_fill(const void* xs, int64_t layer_stride, int32_t T_src, int32_t P,
                                       const int32_t* dilations, int32_t nlayers, int32_t B, int32_t R, void* ring,
                                       int32_t dtype, void* stream) {
  if (B == 0) return 0;
  if (!ring || !dilations || (P > 0 && !xs)) return set_error(SRWN_E_NULL, "generate_ring_fill: null pointer");
  if (R != 64 && R != 32) return set_error(SRWN_E_UNSUPPORTED, "generate_ring_fill: built for R=64 or 32 (got R=%d)", R);
  if (dtype != SRWN_BF16 && dtype != SRWN_F32) return set_error(SRWN_E_DTYPE, "generate_ring_fill: dtype %d", dtype);
  const int V = dtype == SRWN_BF16 ? 8 : 4;
  if (B < 0 || P < 0 || T_src < P || nlayers < 1 || nlayers > kGenMaxLayers || layer_stride < 0 ||
      (P > 0 && (layer_stride % V || (reinterpret_cast<uintptr_t>(xs) & 15) || (nlayers > 1 && layer_stride < (int64_t)B * T_src * R))))
    return set_error(SRWN_E_SHAPE, "generate_ring_fill: B=%d P=%d T_src=%d layers=%d layer_stride=%lld", B, P, T_src,
                     nlayers, (long long)layer_stride);
  RingFillArgs a;
  a.xs = xs; a.ring = ring; a.layer_stride = layer_stride; a.T_src = T_src; a.P = P; a.B = B; a.R = R;
  int bad, maxvec = 0;
  a.ring_group_elems = gen_ring_layout(dilations, nlayers, R, 1 << 20, &bad, a.dil, a.ring_off);
  if (bad >= 0) return set_error(SRWN_E_SHAPE, "generate_ring_fill: dilation %d", dilations[bad]);
  for (int l = 0; l < nlayers; ++l) maxvec = max(maxvec, (a.dil[l] + 1) * 32 * (R / V));
  if ((reinterpret_cast<uintptr_t>(ring) & 15)) return set_error(SRWN_E_SHAPE, "generate_ring_fill: ring not 16-byte aligned");
  const dim3 grid((unsigned)min((maxvec + 255) / 256, 1024), (unsigned)nlayers, (unsigned)((B + 31) / 32));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SRWN_BF16) hipLaunchKernelGGL(ring_fill_kernel<bf16_t>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(ring_fill_kernel<float>, grid, dim3(256), 0, st, a);
  return check_launch("generate_ring_fill");
}

// ---- the rings of pool slots after prompts (srwn.h): row i of one parallel forward pass -> the rows of slot dst[i] of
// every layer ring, so that a slot launch at `clock` continues it at its local step P[i].  Local step tau sits at ring
// position (clock - P + tau) mod (d+1): the oldest one the ring holds, base = P - 1 - d, at (clock - 1 - d) mod (d+1)
// whatever P is.  One (layer, row) per workgroup column; 16-byte vectors along the row's R channels, then positions.
struct RingFillSlotsArgs {
  const void* xs; void* ring; const int32_t* dst; const int32_t* P;
  long long layer_stride, ring_group_elems;
  int T_src, B, R, clock;
  int dil[kGenMaxLayers];
  long long ring_off[kGenMaxLayers];
};

template <typename T>
__global__ __launch_bounds__(256) void ring_fill_slots_kernel(RingFillSlotsArgs a) {
  constexpr int V = 16 / sizeof(T);
  const int l = blockIdx.y, i = blockIdx.z;
  const int u = a.dst[i], P = a.P[i];
  if (u < 0 || u >= a.B || P < 0 || P > a.T_src) return;     // a row that names no slot of the pool, or overlong
  const int d = a.dil[l], depth = d + 1, vpr = a.R / V;
  const int nvec = depth * vpr;
  const int base = P - 1 - d;
  int sb = (a.clock - 1 - d) % depth;                          // ring position of local step base
  if (sb < 0) sb += depth;
  const T* xp = a.xs ? reinterpret_cast<const T*>(a.xs) + (size_t)l * a.layer_stride + (size_t)i * a.T_src * a.R : nullptr;
  T* rp = reinterpret_cast<T*>(a.ring) + (size_t)(u >> 5) * a.ring_group_elems + a.ring_off[l] + (size_t)(u & 31) * a.R;
  for (int k = blockIdx.x * 256 + threadIdx.x; k < nvec; k += gridDim.x * 256) {
    const int cv = k % vpr, s = k / vpr;
    int off = s - sb;
    if (off < 0) off += depth;
    const int tau = base + off;                                  // <= P - 1 < T_src
    uint4 v = {0u, 0u, 0u, 0u};
    if (xp && tau >= 0) v = *reinterpret_cast<const uint4*>(xp + (size_t)tau * a.R + cv * V);
    *reinterpret_cast<uint4*>(rp + (size_t)s * 32 * a.R + cv * V) = v;
  }
}

extern "C" int srwn_generate_ring_fill_slots(const void* xs, int64_t layer_stride, int32_t T_src, int32_t n,
                                             const int32_t* dst, const int32_t* P, int32_t clock,
                                             const int32_t* dilations, int32_t nlayers, int32_t B, int32_t R, void* ring,
                                             int32_t dtype, void* stream) {
  if (n < 0) return set_error(SRWN_E_SHAPE, "generate_ring_fill_slots: n=%d", n);
  if (n == 0) return 0;
  if (!ring || !dilations || !dst || !P) return set_error(SRWN_E_NULL, "generate_ring_fill_slots: null pointer");
  if (R != 64 && R != 32) return set_error(SRWN_E_UNSUPPORTED, "generate_ring_fill_slots: built for R=64 or 32 (got R=%d)", R);
  if (dtype != SRWN_BF16 && dtype != SRWN_F32) return set_error(SRWN_E_DTYPE, "generate_ring_fill_slots: dtype %d", dtype);
  const int V = dtype == SRWN_BF16 ? 8 : 4;
  if (B < 1 || clock < 0 || T_src < 0 || n > 65535 || nlayers < 1 || nlayers > kGenMaxLayers || layer_stride < 0 ||
      (xs && (layer_stride % V || (reinterpret_cast<uintptr_t>(xs) & 15) ||
              (nlayers > 1 && layer_stride < (int64_t)n * T_src * R))))
    return set_error(SRWN_E_SHAPE, "generate_ring_fill_slots: n=%d B=%d clock=%d T_src=%d layers=%d layer_stride=%lld", n, B,
                     clock, T_src, nlayers, (long long)layer_stride);
  if ((reinterpret_cast<uintptr_t>(ring) & 15))
    return set_error(SRWN_E_SHAPE, "generate_ring_fill_slots: ring not 16-byte aligned");
  RingFillSlotsArgs a;
  a.xs = xs; a.ring = ring; a.dst = dst; a.P = P; a.layer_stride = layer_stride; a.T_src = T_src; a.B = B; a.R = R;
  a.clock = clock;
  int bad, maxvec = 0;
  a.ring_group_elems = gen_ring_layout(dilations, nlayers, R, 1 << 20, &bad, a.dil, a.ring_off);
  if (bad >= 0) return set_error(SRWN_E_SHAPE, "generate_ring_fill_slots: dilation %d", dilations[bad]);
  for (int l = 0; l < nlayers; ++l) maxvec = max(maxvec, (a.dil[l] + 1) * (R / V));
  const dim3 grid((unsigned)min((maxvec + 255) / 256, 1024), (unsigned)nlayers, (unsigned)n);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SRWN_BF16) hipLaunchKernelGGL(ring_fill_slots_kernel<bf16_t>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(ring_fill_slots_kernel<float>, grid, dim3(256), 0, st, a);
  return check_launch("generate_ring_fill_slots");
}

// ---- the feed of the live form (srwn.h): the projected conditioning rows of k new frames per utterance -> their rows of
// the ring table.  Memory-bound: one 16-byte vector per thread, consecutive threads along a row.
struct CondScatterArgs {
  const void* rows; void* table;
  long long rows_ld, cond_ld, first;
  int B, k, cond_frames, vpr;
};

template <typename T>
__global__ __launch_bounds__(256) void cond_scatter_kernel(CondScatterArgs a) {
  constexpr int V = 16 / sizeof(T);
  const long long nvec = (long long)a.B * a.k * a.vpr;
  const int f0 = (int)(a.first % a.cond_frames);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long long)gridDim.x * 256) {
    const int cv = (int)(i % a.vpr);
    const long long r = i / a.vpr;                               // source row u * k + j
    const int u = (int)(r / a.k), j = (int)(r - (long long)u * a.k);
    int slot = f0 + j;                                           // j < k <= cond_frames: one wrap
    slot = slot < a.cond_frames ? slot : slot - a.cond_frames;
    const T* sp = reinterpret_cast<const T*>(a.rows) + r * a.rows_ld + cv * V;
    T* dp = reinterpret_cast<T*>(a.table) + ((long long)u * a.cond_frames + slot) * a.cond_ld + cv * V;
    *reinterpret_cast<uint4*>(dp) = *reinterpret_cast<const uint4*>(sp);
  }
}

extern "C" int srwn_cond_ring_scatter(const void* rows, int64_t rows_ld, void* table, int64_t cond_ld, int32_t B,
                                          int32_t k, int64_t first_frame, int32_t cond_frames, int32_t width,
                                          int32_t dtype, void* stream) {
  if (B == 0 || k == 0) return 0;
  if (!rows || !table) return set_error(SRWN_E_NULL, "cond_ring_scatter: null pointer");
  if (dtype != SRWN_BF16 && dtype != SRWN_F32) return set_error(SRWN_E_DTYPE, "cond_ring_scatter: dtype %d", dtype);
  const int V = dtype == SRWN_BF16 ? 8 : 4;
  if (B < 0 || k < 0 || cond_frames < 1 || k > cond_frames || first_frame < 0 || width < V || width % V || rows_ld < width ||
      cond_ld < width || rows_ld % V || cond_ld % V || (reinterpret_cast<uintptr_t>(rows) & 15) ||
      (reinterpret_cast<uintptr_t>(table) & 15) || (int64_t)B * cond_frames > 0x7fffffffLL)
    return set_error(SRWN_E_SHAPE, "cond_ring_scatter: B=%d k=%d first=%lld cond_frames=%d width=%d ld %lld / %lld", B, k,
                     (long long)first_frame, cond_frames, width, (long long)rows_ld, (long long)cond_ld);
  CondScatterArgs a;
  a.rows = rows; a.table = table; a.rows_ld = rows_ld; a.cond_ld = cond_ld; a.first = first_frame;
  a.B = B; a.k = k; a.cond_frames = cond_frames; a.vpr = width / V;
  const long long nvec = (long long)B * k * a.vpr;
  const dim3 grid((unsigned)min((nvec + 255) / 256, (long long)4096));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SRWN_BF16) hipLaunchKernelGGL(cond_scatter_kernel<bf16_t>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(cond_scatter_kernel<float>, grid, dim3(256), 0, st, a);
  return check_launch("cond_ring_scatter");
}

// ---- the ring columns of pool slots that resume after a pause (srwn.h, srwn_version() 114).  The rings follow the pool's
// clock: step c writes position c mod D (D = d_l + 1) and reads the delayed tap at (c + 1) mod D.  A slot whose last own
// step ended at clock c_stop and whose next one runs at clock c' (its stores held back in between) needs
// new[(p + shift) mod D] = old[p] with shift = c' - c_stop.  One OWNER workgroup per (listed slot, layer) column rotates it
// in place by three reversals -- the whole column, its first s = shift mod D positions, the remaining D - s -- each a set
// of disjoint swaps (a thread reads both ends of its pair into registers before it writes either), ordered by the
// workgroup's own barriers: correct for any shift and depth, with no scratch and no ordering between workgroups.
struct RingRotateArgs {
  void* ring; const int32_t* slot_ids; const int32_t* shift;
  long long ring_group_elems;
  int B, R;
  int dil[kGenMaxLayers];
  long long ring_off[kGenMaxLayers];
};

template <typename T>
__global__ __launch_bounds__(256) void ring_rotate_slots_kernel(RingRotateArgs a) {
  constexpr int V = 16 / sizeof(T);
  const int l = blockIdx.x, i = blockIdx.y;
  const int u = a.slot_ids[i], sh = a.shift[i];
  if (u < 0 || u >= a.B || sh < 0) return;                     // a row that names no slot of the pool (workgroup-uniform)
  const int depth = a.dil[l] + 1, vpr = a.R / V;
  const int s = sh % depth;
  if (s == 0) return;                                          // in phase: the column keeps its bits
  T* rp = reinterpret_cast<T*>(a.ring) + (size_t)(u >> 5) * a.ring_group_elems + a.ring_off[l] + (size_t)(u & 31) * a.R;
  const size_t pos_stride = (size_t)32 * a.R;
  auto reverse = [&](int lo, int n) {                          // positions [lo, lo + n) of the column, in place
    const long long nv = (long long)(n / 2) * vpr;
    for (long long k = threadIdx.x; k < nv; k += 256) {
      const int cv = (int)(k % vpr), j = (int)(k / vpr);
      uint4* pa = reinterpret_cast<uint4*>(rp + (size_t)(lo + j) * pos_stride + cv * V);
      uint4* pb = reinterpret_cast<uint4*>(rp + (size_t)(lo + n - 1 - j) * pos_stride + cv * V);
      const uint4 va = *pa, vb = *pb;
      *pa = vb;
      *pb = va;
    }
  };
  reverse(0, depth);
  __syncthreads();
  reverse(0, s);
  reverse(s, depth - s);                                       // (disjoint from the one above: no barrier between them)
}

extern "C" int srwn_generate_ring_rotate_slots(void* ring, const int32_t* dilations, int32_t nlayers, int32_t capacity,
                                               int32_t R, const int32_t* slot_ids, const int32_t* shift, int32_t n,
                                               int32_t dtype, void* stream) {
  if (n < 0) return set_error(SRWN_E_SHAPE, "generate_ring_rotate_slots: n=%d", n);
  if (n == 0) return 0;
  if (!ring || !dilations || !slot_ids || !shift) return set_error(SRWN_E_NULL, "generate_ring_rotate_slots: null pointer");
  if (R != 64 && R != 32) return set_error(SRWN_E_UNSUPPORTED, "generate_ring_rotate_slots: built for R=64 or 32 (got R=%d)", R);
  if (dtype != SRWN_BF16 && dtype != SRWN_F32) return set_error(SRWN_E_DTYPE, "generate_ring_rotate_slots: dtype %d", dtype);
  if (capacity < 1 || n > 65535 || nlayers < 1 || nlayers > kGenMaxLayers)
    return set_error(SRWN_E_SHAPE, "generate_ring_rotate_slots: n=%d capacity=%d layers=%d", n, capacity, nlayers);
  if ((reinterpret_cast<uintptr_t>(ring) & 15))
    return set_error(SRWN_E_SHAPE, "generate_ring_rotate_slots: ring not 16-byte aligned");
  RingRotateArgs a;
  a.ring = ring; a.slot_ids = slot_ids; a.shift = shift; a.B = capacity; a.R = R;
  int bad;
  a.ring_group_elems = gen_ring_layout(dilations, nlayers, R, INT32_MAX - 1, &bad, a.dil, a.ring_off);
  if (bad >= 0) return set_error(SRWN_E_SHAPE, "generate_ring_rotate_slots: dilation %d", dilations[bad]);
  const dim3 grid((unsigned)nlayers, (unsigned)n);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SRWN_BF16) hipLaunchKernelGGL(ring_rotate_slots_kernel<bf16_t>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(ring_rotate_slots_kernel<float>, grid, dim3(256), 0, st, a);
  return check_launch("generate_ring_rotate_slots");
}

// ---- the feed of the live slot form (srwn.h): projected conditioning rows -> the table rows a device list names (ragged
// slots: dst_row[i] = slot * cond_frames + (fed_slot + j) mod cond_frames, computed by the host).  A row whose destination
// is outside the table is skipped.  Memory-bound: one 16-byte vector per thread, consecutive threads along a row.
struct CondScatterSlotsArgs {
  const void* rows; void* table; const int32_t* dst_row;
  long long rows_ld, cond_ld;
  int n_rows, table_rows, vpr;
};

template <typename T>
__global__ __launch_bounds__(256) void cond_scatter_slots_kernel(CondScatterSlotsArgs a) {
  constexpr int V = 16 / sizeof(T);
  const long long nvec = (long long)a.n_rows * a.vpr;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long long)gridDim.x * 256) {
    const int cv = (int)(i % a.vpr);
    const long long r = i / a.vpr;
    const int d = a.dst_row[r];
    if (d < 0 || d >= a.table_rows) continue;
    const T* sp = reinterpret_cast<const T*>(a.rows) + r * a.rows_ld + cv * V;
    T* dp = reinterpret_cast<T*>(a.table) + (long long)d * a.cond_ld + cv * V;
    *reinterpret_cast<uint4*>(dp) = *reinterpret_cast<const uint4*>(sp);
  }
}

extern "C" int srwn_cond_ring_scatter_slots(const void* rows, int64_t rows_ld, void* table, int64_t cond_ld,
                                            int32_t n_rows, const int32_t* dst_row, int32_t table_rows, int32_t width,
                                            int32_t dtype, void* stream) {
  if (n_rows < 0) return set_error(SRWN_E_SHAPE, "cond_ring_scatter_slots: n_rows=%d", n_rows);
  if (n_rows == 0) return 0;
  if (!rows || !table || !dst_row) return set_error(SRWN_E_NULL, "cond_ring_scatter_slots: null pointer");
  if (dtype != SRWN_BF16 && dtype != SRWN_F32) return set_error(SRWN_E_DTYPE, "cond_ring_scatter_slots: dtype %d", dtype);
  const int V = dtype == SRWN_BF16 ? 8 : 4;
  if (n_rows < 0 || table_rows < 1 || width < V || width % V || rows_ld < width || cond_ld < width || rows_ld % V ||
      cond_ld % V || (reinterpret_cast<uintptr_t>(rows) & 15) || (reinterpret_cast<uintptr_t>(table) & 15))
    return set_error(SRWN_E_SHAPE, "cond_ring_scatter_slots: n_rows=%d table_rows=%d width=%d ld %lld / %lld", n_rows,
                     table_rows, width, (long long)rows_ld, (long long)cond_ld);
  CondScatterSlotsArgs a;
  a.rows = rows; a.table = table; a.dst_row = dst_row; a.rows_ld = rows_ld; a.cond_ld = cond_ld;
  a.n_rows = n_rows; a.table_rows = table_rows; a.vpr = width / V;
  const long long nvec = (long long)n_rows * a.vpr;
  const dim3 grid((unsigned)min((nvec + 255) / 256, (long long)4096));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SRWN_BF16) hipLaunchKernelGGL(cond_scatter_slots_kernel<bf16_t>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(cond_scatter_slots_kernel<float>, grid, dim3(256), 0, st, a);
  return check_launch("cond_ring_scatter_slots");
}
