// Streaming likelihood scorer of the softmax teacher (class WaveNetTeacher: createDecoder's stack, model.py:158-196, with the
// per-sample softmax over mu-law codes, model.py:100-112): nll[t] = -log p(code[t] | audio[< t]) for the rows of a chunk.
// gfx950 (MI355X) only; MFMA orientation and lane maps: srwn_common.h.  The stack runs through the streaming classifier's
// entry, group and roll launches (srwn_recog_stream_in on the audio delayed by one sample -- the RightShift --,
// srwn_residual_group_fwd_stream_z, srwn_recog_roll); here is the head, one launch:
//   score head     skip sum from the stored z (gate rebuilt as the skip sum's SRWN_PRO_GATE does), relu, head 1x1, relu, last
//                  1x1, log-softmax and the gather of the target's column, one workgroup per (stream, 32-row tile of the
//                  chunk): r0, r1 and the logits never reach HBM, one fp32 per sample does
//   nll rows       the parity twin of the head's last step: the same reduction from a logits buffer that three
//                  srwn_pw_linear calls wrote
// Both reduce a row with ONE device routine, row_nll, on the same lane-to-column map, and both forms of the three products
// start at the bias and take their k-steps in order: the two paths give the same bits.  A row depends on its own z rows
// only, so a stream has the same bits in any chunking, at any batch size and in any row of the batch.
//
// The conditioned mixture-of-logistics decoder (createDecoder with the encoding, model.py:158-196, trained on
// discretized_mix_logistic_loss, ops.py:124-175; srwn_version() 117) has the same two forms with another last step:
//   mol score head   the score head through the logits (ONE device body, score_head_logits, serves both kernels; the 4M
//                    logits are Cp = 32 or 64 columns in a small LDS block), then row_mol_nll on the undelayed audio
//   mol score rows   its parity twin, row_mol_nll on a logits buffer in HBM
//
// Scorer pools (srwn.h, srwn_version() 118): the softmax scorer's `capacity` rows as slots on the pool's table of
// SrwnSynthSlot, each a stream at a clock of its own with ran = slot_rows(slots[u], n) rows in a chunk of n.
//   pool entry       srwn_score_stream_in_slots: one launch over the pool's audio ring writes the first boundary buffer's
//                    chunk rows from a[s - 2] and a[s - 1] (the RightShift folded into the read: srwn_recog_stream_in's
//                    arithmetic on the delayed audio, no staged copy, no carry) AND the target codes mu_law(a[s])
//                    (srwn_mulaw.h: the routine of srwn_mu_law_encode)
//   slot forms       of the score head and of nll rows: the SLOTS instantiations of the same kernel templates; a workgroup
//                    whose tile starts at or behind ran returns before its first barrier, the others run the clock form's
//                    body with ran in the place of n
//
// Mixture-of-logistics scorer pools (srwn.h, srwn_version() 119): the same for the conditioned mixture-of-logistics scorer.
//   pool entry       srwn_mol_score_stream_in_slots: one launch over the pool's audio ring writes the first boundary buffer's
//                    chunk rows from a[s - 2], a[s - 1] and the slot's conditioning ring (flow_entry_row, srwn_flow_in.h: the
//                    routine of srwn_flow_stream_in -- no staged chunk, no carry) AND the targets x_out = a[s]
//   slot forms       of the mol score head and of mol score rows: the SLOTS instantiations, as above
#include <cmath>
#include "srwn_common.h"
#include "srwn_flow_in.h"
#include "srwn_host.h"
#include "srwn_mulaw.h"
#include "srwn_slots.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

constexpr int kRowLanes = 8;                  // lanes that share a row of logits in row_nll
constexpr int kMaxClasses = 256;
constexpr int kLogitStride = kMaxClasses + 4; // fp32 elements per row of the LDS logits block (16-byte rows, banks 4 apart)
constexpr int kMaxMixtures = 16;              // 4M <= 64 columns: two 32-column tiles, two mixtures per lane of row_mol_nll
constexpr int kMolStride = 4 * kMaxMixtures + 4;      // the same rule for the mixture head's LDS logits block

// What a SLOTS instantiation takes behind the clock form's arguments: the pool's table.  The kernels take it as a parameter
// pack TABLE... that is empty in the clock forms, whose argument lists so stay exactly what they were; the host bodies
// carry it as a SlotsArg.
template <bool SLOTS> struct SlotsArg {};
template <> struct SlotsArg<true> { const SrwnSynthSlot* table; };
__device__ __forceinline__ const SrwnSynthSlot* table_of(const SrwnSynthSlot* table) { return table; }

// rows slot u has in a chunk of n (a negative clock: none)
__device__ __forceinline__ int ran_of(const SrwnSynthSlot* table, int u, int n) {
  const SrwnSynthSlot sl = table[u];
  return sl.t < 0 ? 0 : slot_rows(sl, n);
}

// ------------------------------------------------------------------------------------------
// pool entry: recog_stream_in_kernel's thread map (8 channels per thread, one row per group of R/8 lanes) on the pool's
// audio ring [capacity][ring_len], sample s of a slot in column s mod ring_len.  Row i < ran(u) of slot u, s = slots[u].t + i:
//   v = b; v = fma(a[s-2], w[0], v); v = fma(a[s-1], w[1], v); round to T     (srwn_recog_stream_in on the delayed audio;
//                                                                              samples before time 0 read as 0)
//   codes[u][i] = mu_law_encode_one(a[s])                                     (the row's first thread)
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void score_stream_in_slots_kernel(const float* __restrict__ ring, int ring_len,
                                                                    const float* __restrict__ w,
                                                                    const float* __restrict__ bias, T* __restrict__ out,
                                                                    int64_t out_clip_rows, int hist,
                                                                    int32_t* __restrict__ codes, int64_t codes_stride,
                                                                    int B, int n, int R, float mu, float log1p_mu,
                                                                    const SrwnSynthSlot* __restrict__ slots) {
  const int lpr = R / 8;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = idx / lpr;
  const int sub = (int)(idx % lpr);
  if (row >= (int64_t)B * n) return;
  const int b = (int)(row / n);
  const int t = (int)(row - (int64_t)b * n);
  const SrwnSynthSlot sl = slots[b];
  if (sl.t < 0 || t >= slot_rows(sl, n)) return;
  const float* xb = ring + (int64_t)b * ring_len;
  const long long s = sl.t + t;
  const int c2 = (int)(s % ring_len);                          // a[s]; (ring_len >= 3: the two columns before it differ)
  const int c1 = c2 > 0 ? c2 - 1 : ring_len - 1;
  const int c0 = c1 > 0 ? c1 - 1 : ring_len - 1;
  const float x0 = s >= 2 ? xb[c0] : 0.0f;
  const float x1 = s >= 1 ? xb[c1] : 0.0f;
  if (sub == 0) codes[(int64_t)b * codes_stride + t] = mu_law_encode_one(xb[c2], mu, log1p_mu);
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

// ------------------------------------------------------------------------------------------
// mixture-of-logistics pool entry: the thread map above on the same ring.  Row i < ran(u) of slot u, s = slots[u].t + i:
//   out row = flow_entry_row(a[s-2], a[s-1], cond ring row u * cond_frames + (s / pool) mod cond_frames)
//                                                                             (srwn_flow_stream_in's arithmetic and bits;
//                                                                              samples before time 0 read as 0)
//   x_out[u][i] = a[s]                                                        (the row's first thread: the target, not delayed)
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void mol_score_stream_in_slots_kernel(const float* __restrict__ ring, int ring_len,
                                                                        const float* __restrict__ w,
                                                                        const float* __restrict__ bias,
                                                                        const T* __restrict__ cond, int cond_frames, int pool,
                                                                        int64_t cond_stride, T* __restrict__ out,
                                                                        int64_t out_clip_rows, int hist,
                                                                        float* __restrict__ x_out, int64_t x_stride, int B,
                                                                        int n, int R,
                                                                        const SrwnSynthSlot* __restrict__ slots) {
  const int lpr = R / 8;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = idx / lpr;
  const int sub = (int)(idx % lpr);
  if (row >= (int64_t)B * n) return;
  const int b = (int)(row / n);
  const int t = (int)(row - (int64_t)b * n);
  const SrwnSynthSlot sl = slots[b];
  if (sl.t < 0 || t >= slot_rows(sl, n)) return;
  const float* xb = ring + (int64_t)b * ring_len;
  const long long s = sl.t + t;
  const int c2 = (int)(s % ring_len);                          // a[s]; (ring_len >= 3: the two columns before it differ)
  const int c1 = c2 > 0 ? c2 - 1 : ring_len - 1;
  const int c0 = c1 > 0 ? c1 - 1 : ring_len - 1;
  const float x0 = s >= 2 ? xb[c0] : 0.0f;
  const float x1 = s >= 1 ? xb[c1] : 0.0f;
  if (sub == 0) x_out[(int64_t)b * x_stride + t] = xb[c2];
  flow_entry_row<T>(x0, x1, w, bias, cond, cond_frames, pool, cond_stride, b, s,
                    out, (int64_t)b * out_clip_rows + hist + t, R, sub);
}

// ------------------------------------------------------------------------------------------
// One row of logits -> nll = log(sum_c exp(l[c] - max)) + max - l[code] and the argmax (lowest index on ties), over the
// columns [0, C) only: what lies behind column C (the padding of the last 32-column tile) is never read.  Called by the 8
// consecutive lanes of a row's group, all of them, lane `sub` of the group: lane sub owns the columns sub, sub + 8, ... in
// rising order (its max, then its sum of exp(l - max) in that order), and the lanes' values meet in an xor butterfly
// (distances 1, 2, 4; fp32 addition commutes, so every lane of the group ends with the same bits).  Returns the same
// value in all 8 lanes.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float row_nll(const float* logits_row, int C, int code, int sub, int* best) {
  float m = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = sub; c < C; c += kRowLanes) {
    const float v = logits_row[c];
    if (v > m) { m = v; bi = c; }             // (strict: the lowest of a lane's equal columns stays)
  }
#pragma unroll
  for (int s = 1; s < kRowLanes; s <<= 1) {
    const float om = __shfl_xor(m, s, 64);
    const int ob = __shfl_xor(bi, s, 64);
    if (om > m || (om == m && ob < bi)) { m = om; bi = ob; }
  }
  float sum = 0.0f;
  for (int c = sub; c < C; c += kRowLanes) sum += expf(logits_row[c] - m);
#pragma unroll
  for (int s = 1; s < kRowLanes; s <<= 1) sum += __shfl_xor(sum, s, 64);
  *best = bi;
  return logf(sum) + m - logits_row[code];
}

// What both kernels do with a tile's 32 rows of logits: thread (row = tid / 8, sub = tid % 8) of the workgroup reduces row
// t0 + row of stream b.  A row beyond the chunk (the last tile) is reduced like the chunk's last row and stores nothing.
// A code outside [0, C) is clamped into it (srwn_mu_law_encode never writes one).
__device__ __forceinline__ void reduce_rows(const float* logits_row, int64_t orow, bool live, int C,
                                            const int32_t* __restrict__ codes, float* __restrict__ nll,
                                            int32_t* __restrict__ best, float* __restrict__ logits_out, int sub) {
  int code = codes[orow];
  code = code < 0 ? 0 : (code >= C ? C - 1 : code);
  int bi;
  const float v = row_nll(logits_row, C, code, sub, &bi);
  if (!live) return;
  if (sub == 0) {
    nll[orow] = v;
    if (best) best[orow] = bi;
  }
  if (logits_out)
    for (int c = sub; c < C; c += kRowLanes) logits_out[orow * C + c] = logits_row[c];
}

// ------------------------------------------------------------------------------------------
// One row of the mixture-of-logistics head: l = (logit_probs [M], means [M], log_scales [M], coeffs [M]) and the target
// sample xv -> nll = -log_sum_exp_m(log p_m(xv) + log_softmax(logit_probs)_m)  (ops.py:124-175 with sum_all = False), in
// mol_nll_rows_kernel's per-mixture arithmetic (srwn_ops.hip: the four tf.where branches, the log-scale floor -7, the half
// bin 1/255, log 127.5).  Called by the 8 lanes of a row's group, lane `sub` of it: lane sub owns the mixtures sub and
// sub + 8 below M (M <= 16), in that order, and the lanes' values meet in row_nll's xor butterfly (1, 2, 4).  A lane
// without a mixture brings -inf to a max and nothing to a sum, and never subtracts from its -inf.  The columns from 3M on
// (the coeffs, unused for one audio channel, and the tile's padding) are never read.  The same value in all 8 lanes.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float mol_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ float mol_softplus(float v) { return v > 0.0f ? v + log1pf(expf(-v)) : log1pf(expf(v)); }

// log p_m(xv) of one mixture component (ops.py:147-169)
__device__ __forceinline__ float mol_component(float xv, float mean, float raw_log_scale) {
  const float ls = fmaxf(raw_log_scale, -7.0f);
  const float cx = xv - mean, inv = expf(-ls);
  const float plus_in = inv * (cx + 1.0f / 255.0f), min_in = inv * (cx - 1.0f / 255.0f), mid_in = inv * cx;
  const float cdf_delta = mol_sigmoid(plus_in) - mol_sigmoid(min_in);
  if (xv < -0.999f) return plus_in - mol_softplus(plus_in);
  if (xv > 0.999f) return -mol_softplus(min_in);
  if (cdf_delta > 1e-5f) return logf(fmaxf(cdf_delta, 1e-12f));
  return mid_in - ls - 2.0f * mol_softplus(mid_in) - logf(127.5f);
}

__device__ __forceinline__ float butterfly_max(float v) {
#pragma unroll
  for (int s = 1; s < kRowLanes; s <<= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
  return v;
}
__device__ __forceinline__ float butterfly_sum(float v) {
#pragma unroll
  for (int s = 1; s < kRowLanes; s <<= 1) v += __shfl_xor(v, s, 64);
  return v;
}

__device__ __forceinline__ float row_mol_nll(const float* l, int M, float xv, int sub) {
  const bool has0 = sub < M, has1 = sub + kRowLanes < M;
  const float p0 = has0 ? l[sub] : -INFINITY, p1 = has1 ? l[sub + kRowLanes] : -INFINITY;
  // log-softmax of the mixture logits (lane 0 always owns mixture 0: the max is finite)
  const float mp = butterfly_max(fmaxf(p0, p1));
  float sp = 0.0f;
  if (has0) sp += expf(p0 - mp);
  if (has1) sp += expf(p1 - mp);
  const float lsp = mp + logf(butterfly_sum(sp));
  float v0 = -INFINITY, v1 = -INFINITY;
  if (has0) v0 = mol_component(xv, l[M + sub], l[2 * M + sub]) + (p0 - lsp);
  if (has1) v1 = mol_component(xv, l[M + sub + kRowLanes], l[2 * M + sub + kRowLanes]) + (p1 - lsp);
  const float best = butterfly_max(fmaxf(v0, v1));
  float s = 0.0f;
  if (has0) s += expf(v0 - best);
  if (has1) s += expf(v1 - best);
  return -(best + logf(butterfly_sum(s)));
}

// reduce_rows for the mixture head: thread (row, sub) reduces row t0 + row of stream b on the target sample x[xrow]; a row
// beyond the chunk is reduced like the chunk's last row and stores nothing.  logits_out takes the 4M real columns.
__device__ __forceinline__ void reduce_mol_rows(const float* logits_row, int64_t orow, int64_t xrow, bool live, int M,
                                                const float* __restrict__ x, float* __restrict__ nll,
                                                float* __restrict__ logits_out, int sub) {
  const float v = row_mol_nll(logits_row, M, x[xrow], sub);
  if (!live) return;
  if (sub == 0) nll[orow] = v;
  if (logits_out)
    for (int c = sub; c < 4 * M; c += kRowLanes) logits_out[orow * (4 * M) + c] = logits_row[c];
}

// ------------------------------------------------------------------------------------------
// score head.  Workgroup = (stream b, tile i of the chunk's ceil(n / 32) tiles), 4 waves; wave w owns the output channels
// [w * S/4, (w + 1) * S/4) of the first two products and the 32-column tiles w, w + 4 of the logits.  In pooled_stream_head's
// arithmetic (srwn_recog.hip):
//   accS = bs_sum + sum_l Ws_l . gate(z_l)      B fragments: 8 channels of one z row per lane (natural k order), the gate
//                                               on the fragment; A fragments from the packed skip image in L2
//   r0 = relu(accS) rounded to T -> xch[32][S]  LDS, rows = time: the B operand of the head 1x1 for all four waves
//   acc1 = b1 + W1 . r0;  r1 = relu(acc1) rounded to T -> xch again, once every wave has read r0 (a barrier)
//   logits = b2 + W2 . r1 (fp32)  -> lg[32][kLogitStride]      all Cp = 32 * ceil(C / 32) columns; the image's rows behind C
//                                               and their biases are zero, and row_nll never reads those columns
//   nll, best = row_nll(lg[row])                8 lanes per row
// A column of the tile beyond the chunk's last row re-reads that row (as the pooled head masks) and stores nothing.
// Dynamic LDS: xch = 32 x (S + 16 / sizeof(T)) x sizeof(T) bytes (33 280 for S = 256 in fp32), then lg = 33 280 bytes.
// ------------------------------------------------------------------------------------------
template <typename T, int S> constexpr int xch_bytes() { return 32 * RowStage<T>::stride(S) * (int)sizeof(T); }
constexpr int kLogitBytes = 32 * kLogitStride * (int)sizeof(float);

// The body both heads share, through the logits: every thread of the workgroup calls it; afterwards (a barrier inside) lg
// holds the tile's 32 rows of ctiles * 32 logits at a row stride of LGS floats.  *b_out, *t0_out, *valid_out: the stream,
// the tile's first chunk row and its rows inside the chunk.
template <typename T, int R, int S, int LGS>
__device__ __forceinline__ void score_head_logits(const T* __restrict__ z, int64_t z_layer_stride, int64_t z_clip_rows, int L,
                                                  const T* __restrict__ wskip, const float* __restrict__ bs_sum,
                                                  const T* __restrict__ w1, const float* __restrict__ b1,
                                                  const T* __restrict__ w2, const float* __restrict__ b2, int n, int ntiles,
                                                  int ctiles, T* xch, float* lg, int* b_out, int* t0_out, int* valid_out) {
  constexpr int MTW = S / 128;                // 32-channel output tiles per wave
  constexpr int KSL = R / 16;                 // k-steps per layer
  constexpr int KS1 = S / 16;
  constexpr int LS = RowStage<T>::stride(S);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int col = lane & 31, half = lane >> 5;
  const int b = (int)blockIdx.x / ntiles, t0 = 32 * ((int)blockIdx.x % ntiles);
  const int valid = n - t0 < 32 ? n - t0 : 32;
  const int ks_skip = L * KSL;
  const Frag<T>* ws = reinterpret_cast<const Frag<T>*>(wskip) + (size_t)(wave * MTW) * ks_skip * 64 + lane;
  const Frag<T>* wh = reinterpret_cast<const Frag<T>*>(w1) + (size_t)(wave * MTW) * KS1 * 64 + lane;
  const int trow = t0 + (col < valid ? col : valid - 1);      // (a masked column re-reads the chunk's last row)
  const T* zr = z + ((int64_t)b * z_clip_rows + trow) * R + 8 * half;
  f32x16 acc[MTW];
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[mt][q] = bs_sum[32 * (wave * MTW + mt) + crow(q, half)];
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
    for (int q = 0; q < 16; ++q) acc[mt][q] = b1[32 * (wave * MTW + mt) + crow(q, half)];
#pragma unroll 4
  for (int ks = 0; ks < KS1; ++ks) {
    const Frag<T> bf = load_nat(xch + col * LS + 16 * ks + 8 * half);
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) mma(acc[mt], wh[((size_t)mt * KS1 + ks) * 64], bf);
  }
  __syncthreads();                            // every wave has read r0: r1 takes its place
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      store4(xch + col * LS + 32 * (wave * MTW + mt) + 8 * g + 4 * half, fmaxf(acc[mt][4 * g], 0.0f),
             fmaxf(acc[mt][4 * g + 1], 0.0f), fmaxf(acc[mt][4 * g + 2], 0.0f), fmaxf(acc[mt][4 * g + 3], 0.0f));
  __syncthreads();
  for (int mt = wave; mt < ctiles; mt += 4) { // (wave-uniform; the mixture head's ctiles <= 2: two waves idle here, and k is
    // NOT split across them -- that would change the summation order and lose the parity twin)
    const Frag<T>* wl = reinterpret_cast<const Frag<T>*>(w2) + (size_t)mt * KS1 * 64 + lane;
    f32x16 a2;
#pragma unroll
    for (int q = 0; q < 16; ++q) a2[q] = b2[32 * mt + crow(q, half)];
#pragma unroll 4
    for (int ks = 0; ks < KS1; ++ks) mma(a2, wl[(size_t)ks * 64], load_nat(xch + col * LS + 16 * ks + 8 * half));
#pragma unroll
    for (int g = 0; g < 4; ++g)
      store4(lg + col * LGS + 32 * mt + 8 * g + 4 * half, a2[4 * g], a2[4 * g + 1], a2[4 * g + 2], a2[4 * g + 3]);
  }
  __syncthreads();
  *b_out = b; *t0_out = t0; *valid_out = valid;
}

// SLOTS (srwn_stream_score_head_slots): stream b is slot b of the pool's table with ran(b) rows in the place of n; the
// workgroup of a tile that starts at or behind ran(b) returns here, before the first barrier (workgroup-uniform).
template <typename T, int R, int S, bool SLOTS = false, typename... TABLE>
__global__ __launch_bounds__(256) void stream_score_head_kernel(const T* __restrict__ z, int64_t z_layer_stride,
                                                                 int64_t z_clip_rows, int L, const T* __restrict__ wskip,
                                                                 const float* __restrict__ bs_sum,
                                                                 const T* __restrict__ w1, const float* __restrict__ b1,
                                                                 const T* __restrict__ w2, const float* __restrict__ b2,
                                                                 const int32_t* __restrict__ codes,
                                                                 float* __restrict__ nll, int32_t* __restrict__ best,
                                                                 float* __restrict__ logits_out, int64_t out_stride, int n,
                                                                 int ntiles, int C, TABLE... table) {
  static_assert(sizeof...(TABLE) == (SLOTS ? 1 : 0), "the table, in the slot form only");
  if constexpr (SLOTS) {
    n = ran_of(table_of(table...), (int)blockIdx.x / ntiles, n);
    if (32 * ((int)blockIdx.x % ntiles) >= n) return;
  }
  extern __shared__ __attribute__((aligned(16))) char score_lds[];
  T* xch = reinterpret_cast<T*>(score_lds);
  float* lg = reinterpret_cast<float*>(score_lds + xch_bytes<T, S>());
  int b, t0, valid;
  score_head_logits<T, R, S, kLogitStride>(z, z_layer_stride, z_clip_rows, L, wskip, bs_sum, w1, b1, w2, b2, n, ntiles,
                                           (C + 31) / 32, xch, lg, &b, &t0, &valid);
  const int row = (int)threadIdx.x / kRowLanes, sub = (int)threadIdx.x % kRowLanes;
  const bool live = row < valid;
  const int64_t orow = (int64_t)b * out_stride + t0 + (live ? row : valid - 1);
  reduce_rows(lg + row * kLogitStride, orow, live, C, codes, nll, best, logits_out, sub);
}

// ------------------------------------------------------------------------------------------
// mol score head: the score head with the mixture-of-logistics reduction.  logits = b2 + W2 . r1 stay fp32 (the means must
// resolve 1/255 bins) in lg[32][kMolStride]: the Cp / 32 <= 2 column tiles of the 4M logits, waves 0 and 1.  x [B][x_stride]
// fp32 is the chunk's own audio (the target of row t is x[t], NOT delayed).
// Dynamic LDS: xch as above, then lg = 32 x 68 x 4 = 8 704 bytes.
// ------------------------------------------------------------------------------------------
constexpr int kMolLogitBytes = 32 * kMolStride * (int)sizeof(float);

// SLOTS (srwn_stream_mol_score_head_slots): as in the score head.
template <typename T, int R, int S, bool SLOTS = false, typename... TABLE>
__global__ __launch_bounds__(256) void mol_stream_score_head_kernel(const T* __restrict__ z, int64_t z_layer_stride,
                                                                     int64_t z_clip_rows, int L, const T* __restrict__ wskip,
                                                                     const float* __restrict__ bs_sum,
                                                                     const T* __restrict__ w1, const float* __restrict__ b1,
                                                                     const T* __restrict__ w2, const float* __restrict__ b2,
                                                                     const float* __restrict__ x, int64_t x_stride,
                                                                     float* __restrict__ nll, float* __restrict__ logits_out,
                                                                     int64_t out_stride, int n, int ntiles, int M,
                                                                     TABLE... table) {
  static_assert(sizeof...(TABLE) == (SLOTS ? 1 : 0), "the table, in the slot form only");
  if constexpr (SLOTS) {
    n = ran_of(table_of(table...), (int)blockIdx.x / ntiles, n);
    if (32 * ((int)blockIdx.x % ntiles) >= n) return;
  }
  extern __shared__ __attribute__((aligned(16))) char score_lds[];
  T* xch = reinterpret_cast<T*>(score_lds);
  float* lg = reinterpret_cast<float*>(score_lds + xch_bytes<T, S>());
  int b, t0, valid;
  score_head_logits<T, R, S, kMolStride>(z, z_layer_stride, z_clip_rows, L, wskip, bs_sum, w1, b1, w2, b2, n, ntiles,
                                         (4 * M + 31) / 32, xch, lg, &b, &t0, &valid);
  const int row = (int)threadIdx.x / kRowLanes, sub = (int)threadIdx.x % kRowLanes;
  const bool live = row < valid;
  const int t = t0 + (live ? row : valid - 1);
  reduce_mol_rows(lg + row * kMolStride, (int64_t)b * out_stride + t, (int64_t)b * x_stride + t, live, M, x, nll, logits_out,
                  sub);
}

// ------------------------------------------------------------------------------------------
// nll rows (parity twin): logits [B][clip_rows][ld] fp32 of the chunk -> nll, best and the copy of the C real columns.
// The score head's grid and its thread-to-row map, row_nll on the row in HBM.
// ------------------------------------------------------------------------------------------
// SLOTS (srwn_nll_rows_slots): as in the score head.
template <bool SLOTS = false, typename... TABLE>
__global__ __launch_bounds__(256) void nll_rows_kernel(const float* __restrict__ logits, int64_t ld, int64_t clip_rows,
                                                       const int32_t* __restrict__ codes, float* __restrict__ nll,
                                                       int32_t* __restrict__ best, float* __restrict__ logits_out,
                                                       int64_t out_stride, int n, int ntiles, int C, TABLE... table) {
  static_assert(sizeof...(TABLE) == (SLOTS ? 1 : 0), "the table, in the slot form only");
  if constexpr (SLOTS) {
    n = ran_of(table_of(table...), (int)blockIdx.x / ntiles, n);
    if (32 * ((int)blockIdx.x % ntiles) >= n) return;
  }
  const int b = (int)blockIdx.x / ntiles, t0 = 32 * ((int)blockIdx.x % ntiles);
  const int valid = n - t0 < 32 ? n - t0 : 32;
  const int row = (int)threadIdx.x / kRowLanes, sub = (int)threadIdx.x % kRowLanes;
  const bool live = row < valid;
  const int t = t0 + (live ? row : valid - 1);
  reduce_rows(logits + ((int64_t)b * clip_rows + t) * ld, (int64_t)b * out_stride + t, live, C, codes, nll, best, logits_out,
              sub);
}

// mol score rows (parity twin): nll_rows_kernel's grid and thread-to-row map, row_mol_nll on the row in HBM.
// SLOTS (srwn_mol_score_rows_slots): as in the score head.
template <bool SLOTS = false, typename... TABLE>
__global__ __launch_bounds__(256) void mol_score_rows_kernel(const float* __restrict__ logits, int64_t ld, int64_t clip_rows,
                                                             const float* __restrict__ x, int64_t x_stride,
                                                             float* __restrict__ nll, float* __restrict__ logits_out,
                                                             int64_t out_stride, int n, int ntiles, int M,
                                                             TABLE... table) {
  static_assert(sizeof...(TABLE) == (SLOTS ? 1 : 0), "the table, in the slot form only");
  if constexpr (SLOTS) {
    n = ran_of(table_of(table...), (int)blockIdx.x / ntiles, n);
    if (32 * ((int)blockIdx.x % ntiles) >= n) return;
  }
  const int b = (int)blockIdx.x / ntiles, t0 = 32 * ((int)blockIdx.x % ntiles);
  const int valid = n - t0 < 32 ? n - t0 : 32;
  const int row = (int)threadIdx.x / kRowLanes, sub = (int)threadIdx.x % kRowLanes;
  const bool live = row < valid;
  const int t = t0 + (live ? row : valid - 1);
  reduce_mol_rows(logits + ((int64_t)b * clip_rows + t) * ld, (int64_t)b * out_stride + t, (int64_t)b * x_stride + t, live, M,
                  x, nll, logits_out, sub);
}

int rows_args(const char* who, int32_t B, int32_t n, int32_t C, int64_t clip_rows, int64_t out_stride) {
  if (C < 1 || C > kMaxClasses) return set_error(SRWN_E_SHAPE, "%s: %d classes (1..%d)", who, C, kMaxClasses);
  if (B < 1 || n < 1) return set_error(SRWN_E_SHAPE, "%s: B=%d, a chunk of %d rows", who, B, n);
  if (clip_rows < n || out_stride < n)
    return set_error(SRWN_E_SHAPE, "%s: %d rows in buffers of %lld rows per stream, outputs of %lld", who, n,
                     (long long)clip_rows, (long long)out_stride);
  if ((int64_t)B * ((n + 31) / 32) > 0x7fffffffLL) return set_error(SRWN_E_SHAPE, "%s: too many tiles", who);
  return 0;
}

// ------------------------------------------------------------------------------------------
// Host side: one body per pair.  The softmax launches (score head, nll rows) and the mixture launches (mol score head, mol
// score rows) differ in what a row is scored against and in what the reduction leaves beside nll; HeadRows holds either.
// ------------------------------------------------------------------------------------------
struct HeadRows {
  const int32_t* codes;              // softmax: the targets
  const float* x; int64_t x_stride;  // mixture: the chunk's own audio
  float* nll; int32_t* best; float* logits_out; int64_t out_stride;      // (best: softmax only; best, logits_out may be null)
  int width;                         // C classes, or M mixtures
  const void* target(bool mol) const { return mol ? (const void*)x : (const void*)codes; }
};

template <bool MOL>
int check_rows(const char* who, const HeadRows& r, int32_t B, int32_t n, int64_t clip_rows) {
  if (MOL && (r.width < 1 || r.width > kMaxMixtures))
    return set_error(SRWN_E_SHAPE, "%s: %d mixtures (1..%d)", who, r.width, kMaxMixtures);
  if (MOL && r.x_stride < n)
    return set_error(SRWN_E_SHAPE, "%s: %d rows of audio at a stride of %lld", who, n, (long long)r.x_stride);
  return rows_args(who, B, n, MOL ? 4 * r.width : r.width, clip_rows, r.out_stride);
}

template <bool MOL, bool SLOTS, typename T, int R, int S>
int launch_score_head(const char* who, const void* z, int64_t z_layer_stride, int64_t z_clip_rows, int L, const void* wskip,
                      const float* bs_sum, const void* w1, const float* b1, const void* w2, const float* b2,
                      const HeadRows& r, int B, int n, SlotsArg<SLOTS> slots, hipStream_t st) {
  constexpr int sh = xch_bytes<T, S>() + (MOL ? kMolLogitBytes : kLogitBytes);
  const int ntiles = (n + 31) / 32;
  auto launch = [&](auto kfn, auto... rows) {      // rows: what the kernel takes behind b2
    if (sh > 32768) (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, sh);
    hipLaunchKernelGGL(kfn, dim3((unsigned)(B * ntiles)), dim3(256), sh, st, (const T*)z, z_layer_stride, z_clip_rows, L,
                       (const T*)wskip, bs_sum, (const T*)w1, b1, (const T*)w2, b2, rows...);
  };
  if constexpr (MOL && SLOTS)
    launch(mol_stream_score_head_kernel<T, R, S, true, const SrwnSynthSlot*>, r.x, r.x_stride, r.nll, r.logits_out, r.out_stride,
           n, ntiles, r.width, slots.table);
  else if constexpr (MOL)
    launch(mol_stream_score_head_kernel<T, R, S>, r.x, r.x_stride, r.nll, r.logits_out, r.out_stride, n, ntiles, r.width);
  else if constexpr (SLOTS)
    launch(stream_score_head_kernel<T, R, S, true, const SrwnSynthSlot*>, r.codes, r.nll, r.best, r.logits_out, r.out_stride, n,
           ntiles, r.width, slots.table);
  else
    launch(stream_score_head_kernel<T, R, S>, r.codes, r.nll, r.best, r.logits_out, r.out_stride, n, ntiles, r.width);
  return check_launch(who);
}

// The slot forms (SLOTS: B is the pool's capacity, `slots` its table) report empty work (capacity * n == 0) as done and, the
// softmax ones, a class count that is not built as such (-4), both before anything else of theirs.  (The mixture forms
// leave their mixture count to check_rows: -2, as in the clock forms.)
template <bool MOL>
int slot_form_first(const char* who, const SrwnSynthSlot* table, int C) {
  if (!table) return set_error(SRWN_E_NULL, "%s: null pointer (slots is the pool's device table)", who);
  if (!MOL && (C < 1 || C > kMaxClasses))
    return set_error(SRWN_E_UNSUPPORTED, "%s: %d classes (built: 1..%d)", who, C, kMaxClasses);
  return 0;
}

template <bool MOL, bool SLOTS = false>
int score_head_impl(const char* who, const void* z, int64_t z_layer_stride, int64_t z_clip_rows, int32_t nlayers,
                    const void* wskip, const float* bs_sum, const void* w1, const float* b1, const void* w2, const float* b2,
                    const HeadRows& r, int32_t B, int32_t n, int32_t max_chunk, int32_t R, int32_t S, int32_t dtype,
                    void* stream, SlotsArg<SLOTS> slots = {}) {
  if (SLOTS && (B == 0 || n == 0)) return 0;
  if (!z || !wskip || !bs_sum || !w1 || !b1 || !w2 || !b2 || !r.target(MOL) || !r.nll)
    return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if constexpr (SLOTS)
    if (const int rc = slot_form_first<MOL>(who, slots.table, r.width)) return rc;
  if ((R != 32 && R != 64) || (S != 128 && S != 256))
    return set_error(SRWN_E_UNSUPPORTED, "%s: dilation_channels %d, skip_channels %d (built: 32 / 64 x 128 / 256)", who, R, S);
  if (max_chunk < 1 || n > max_chunk || z_clip_rows < max_chunk)
    return set_error(SRWN_E_SHAPE, "%s: a chunk of %d rows in buffers of %lld rows per stream (max_chunk = %d)", who, n,
                     (long long)z_clip_rows, max_chunk);
  if (const int rc = check_rows<MOL>(who, r, B, n, z_clip_rows)) return rc;
  if (nlayers < 1 || z_layer_stride < (int64_t)B * z_clip_rows * R)
    return set_error(SRWN_E_SHAPE, "%s: %d layers at a stride of %lld", who, nlayers, (long long)z_layer_stride);
#define SRWN_SSH(TT, RR, SS)                                                                                               \
  return launch_score_head<MOL, SLOTS, TT, RR, SS>(who, z, z_layer_stride, z_clip_rows, nlayers, wskip, bs_sum, w1, b1, w2, \
                                                   b2, r, B, n, slots, (hipStream_t)stream)
#define SRWN_SSH_T(TT)                                       \
  {                                                          \
    if (R == 32 && S == 128) SRWN_SSH(TT, 32, 128);          \
    else if (R == 32) SRWN_SSH(TT, 32, 256);                 \
    else if (S == 128) SRWN_SSH(TT, 64, 128);                \
    else SRWN_SSH(TT, 64, 256);                              \
  }
  if (dtype == SRWN_BF16) SRWN_SSH_T(bf16_t)
  else if (dtype == SRWN_F32) SRWN_SSH_T(float)
#undef SRWN_SSH_T
#undef SRWN_SSH
  return set_error(SRWN_E_DTYPE, "%s: dtype %d", who, dtype);
}

template <bool MOL, bool SLOTS = false>
int score_rows_impl(const char* who, const float* logits, int64_t logits_ld, int64_t logits_clip_rows, const HeadRows& r,
                    int32_t B, int32_t n, void* stream, SlotsArg<SLOTS> slots = {}) {
  if (SLOTS && (B == 0 || n == 0)) return 0;
  if (!logits || !r.target(MOL) || !r.nll) return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if constexpr (SLOTS)
    if (const int rc = slot_form_first<MOL>(who, slots.table, r.width)) return rc;
  if (const int rc = check_rows<MOL>(who, r, B, n, logits_clip_rows)) return rc;
  if (logits_ld < (MOL ? 4 * r.width : r.width))
    return set_error(SRWN_E_SHAPE, "%s: rows of %lld logits for %d %s", who, (long long)logits_ld, r.width,
                     MOL ? "mixtures" : "classes");
  const int ntiles = (n + 31) / 32;
  const dim3 grid((unsigned)(B * ntiles));
  if constexpr (MOL && SLOTS)
    hipLaunchKernelGGL((mol_score_rows_kernel<true, const SrwnSynthSlot*>), grid, dim3(256), 0, (hipStream_t)stream, logits,
                       logits_ld, logits_clip_rows, r.x, r.x_stride, r.nll, r.logits_out, r.out_stride, n, ntiles, r.width,
                       slots.table);
  else if constexpr (MOL)
    hipLaunchKernelGGL(mol_score_rows_kernel<>, grid, dim3(256), 0, (hipStream_t)stream, logits, logits_ld, logits_clip_rows, r.x,
                       r.x_stride, r.nll, r.logits_out, r.out_stride, n, ntiles, r.width);
  else if constexpr (SLOTS)
    hipLaunchKernelGGL((nll_rows_kernel<true, const SrwnSynthSlot*>), grid, dim3(256), 0, (hipStream_t)stream, logits, logits_ld,
                       logits_clip_rows, r.codes, r.nll, r.best, r.logits_out, r.out_stride, n, ntiles, r.width, slots.table);
  else
    hipLaunchKernelGGL(nll_rows_kernel<>, grid, dim3(256), 0, (hipStream_t)stream, logits, logits_ld, logits_clip_rows, r.codes,
                       r.nll, r.best, r.logits_out, r.out_stride, n, ntiles, r.width);
  return check_launch(who);
}

// The pool entry's host body: srwn_recog_stream_in_slots' checks with the ring one sample longer (a[t - 2]) and the codes.
int score_stream_in_slots_impl(const char* who, const float* ring, int32_t ring_len, const float* init_w, const float* init_b,
                               void* out, int64_t out_clip_rows, int32_t out_hist, int32_t* codes, int64_t codes_stride,
                               int32_t capacity, int32_t n, int32_t max_chunk, int32_t R, int32_t C, int32_t dtype,
                               const SrwnSynthSlot* slots, void* stream) {
  if (capacity == 0 || n == 0) return 0;
  if (!ring || !init_w || !init_b || !out || !codes || !slots) return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if (R != 32 && R != 64) return set_error(SRWN_E_UNSUPPORTED, "%s: dilation_channels %d (built: 32, 64)", who, R);
  if (C < 2 || C > kMaxClasses) return set_error(SRWN_E_UNSUPPORTED, "%s: %d classes (built: 2..%d)", who, C, kMaxClasses);
  if (capacity < 1 || max_chunk < 1 || out_hist < 0)
    return set_error(SRWN_E_SHAPE, "%s: capacity=%d max_chunk=%d out_hist=%d", who, capacity, max_chunk, out_hist);
  if (n < 1 || n > max_chunk) return set_error(SRWN_E_SHAPE, "%s: chunk of %d rows (1..max_chunk = %d)", who, n, max_chunk);
  // (the ring also holds the two samples before a whole chunk)
  if (ring_len < (int64_t)max_chunk + 2 || out_clip_rows < (int64_t)out_hist + max_chunk || codes_stride < max_chunk)
    return set_error(SRWN_E_SHAPE, "%s: an audio ring of %d samples for max_chunk + 2 = %lld, %lld buffer rows per slot for %d + %d, "
                     "%lld codes per slot", who, ring_len, (long long)max_chunk + 2, (long long)out_clip_rows, out_hist, max_chunk,
                     (long long)codes_stride);
  if (dtype != SRWN_BF16 && dtype != SRWN_F32) return set_error(SRWN_E_DTYPE, "%s: dtype %d", who, dtype);
  const int64_t threads = (int64_t)capacity * n * (R / 8);
  dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const float mu = (float)(C - 1), l1p = (float)log1p((double)mu);      // (srwn_mu_law_encode's constants)
  if (dtype == SRWN_BF16)
    hipLaunchKernelGGL(score_stream_in_slots_kernel<bf16_t>, grid, block, 0, st, ring, ring_len, init_w, init_b, (bf16_t*)out,
                       out_clip_rows, out_hist, codes, codes_stride, capacity, n, R, mu, l1p, slots);
  else
    hipLaunchKernelGGL(score_stream_in_slots_kernel<float>, grid, block, 0, st, ring, ring_len, init_w, init_b, (float*)out,
                       out_clip_rows, out_hist, codes, codes_stride, capacity, n, R, mu, l1p, slots);
  return check_launch(who);
}

// The mixture pool entry's host body: srwn_flow_stream_in_slots' checks with the ring in the place of the staged chunk and
// its carry, and the targets.
int mol_score_stream_in_slots_impl(const char* who, const float* ring, int32_t ring_len, const float* init_w,
                                   const float* init_b, const void* cond0, int32_t cond_frames, int32_t pool_stride,
                                   int64_t cond_row_stride, void* out, int64_t out_clip_rows, int32_t out_hist, float* x_out,
                                   int64_t x_stride, int32_t capacity, int32_t n, int32_t max_chunk, int32_t R, int32_t dtype,
                                   const SrwnSynthSlot* slots, void* stream) {
  if (capacity == 0 || n == 0) return 0;
  if (!ring || !init_w || !init_b || !cond0 || !out || !x_out || !slots) return set_error(SRWN_E_NULL, "%s: null pointer", who);
  if (R != 32 && R != 64) return set_error(SRWN_E_UNSUPPORTED, "%s: dilation_channels %d (built: 32, 64)", who, R);
  if (capacity < 1 || max_chunk < 1 || out_hist < 0 || cond_frames < 1 || pool_stride < 1 || cond_row_stride < R ||
      cond_row_stride % 8)
    return set_error(SRWN_E_SHAPE, "%s: capacity=%d max_chunk=%d out_hist=%d frames=%d pool=%d cond stride %lld", who, capacity,
                     max_chunk, out_hist, cond_frames, pool_stride, (long long)cond_row_stride);
  if (n < 1 || n > max_chunk) return set_error(SRWN_E_SHAPE, "%s: chunk of %d rows (1..max_chunk = %d)", who, n, max_chunk);
  // (the ring also holds the two samples before a whole chunk)
  if (ring_len < (int64_t)max_chunk + 2 || out_clip_rows < (int64_t)out_hist + max_chunk || x_stride < max_chunk)
    return set_error(SRWN_E_SHAPE, "%s: an audio ring of %d samples for max_chunk + 2 = %lld, %lld buffer rows per slot for %d + %d, "
                     "%lld targets per slot", who, ring_len, (long long)max_chunk + 2, (long long)out_clip_rows, out_hist,
                     max_chunk, (long long)x_stride);
  if ((int64_t)capacity * ring_len > 0x7fffffffLL) return set_error(SRWN_E_SHAPE, "%s: %d rings of %d samples", who, capacity, ring_len);
  if (dtype != SRWN_BF16 && dtype != SRWN_F32) return set_error(SRWN_E_DTYPE, "%s: dtype %d", who, dtype);
  const int64_t threads = (int64_t)capacity * n * (R / 8);
  dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SRWN_BF16)
    hipLaunchKernelGGL(mol_score_stream_in_slots_kernel<bf16_t>, grid, block, 0, st, ring, ring_len, init_w, init_b,
                       (const bf16_t*)cond0, cond_frames, pool_stride, cond_row_stride, (bf16_t*)out, out_clip_rows, out_hist,
                       x_out, x_stride, capacity, n, R, slots);
  else
    hipLaunchKernelGGL(mol_score_stream_in_slots_kernel<float>, grid, block, 0, st, ring, ring_len, init_w, init_b,
                       (const float*)cond0, cond_frames, pool_stride, cond_row_stride, (float*)out, out_clip_rows, out_hist,
                       x_out, x_stride, capacity, n, R, slots);
  return check_launch(who);
}

}  // namespace

extern "C" int srwn_stream_score_head(const void* z, int64_t z_layer_stride, int64_t z_clip_rows, int32_t nlayers,
                                      const void* wskip, const float* bs_sum, const void* w1, const float* b1,
                                      const void* w2, const float* b2, const int32_t* codes, float* nll, int32_t* best,
                                      float* logits_out, int64_t out_stride, int32_t B, int32_t n, int32_t max_chunk,
                                      int32_t R, int32_t S, int32_t C, int32_t dtype, void* stream) {
  return score_head_impl<false>("stream_score_head", z, z_layer_stride, z_clip_rows, nlayers, wskip, bs_sum, w1, b1, w2, b2,
                                HeadRows{codes, nullptr, 0, nll, best, logits_out, out_stride, C}, B, n, max_chunk, R, S,
                                dtype, stream);
}

extern "C" int srwn_nll_rows(const float* logits, int64_t logits_ld, int64_t logits_clip_rows, const int32_t* codes,
                             float* nll, int32_t* best, float* logits_out, int64_t out_stride, int32_t B, int32_t n,
                             int32_t C, void* stream) {
  return score_rows_impl<false>("nll_rows", logits, logits_ld, logits_clip_rows,
                                HeadRows{codes, nullptr, 0, nll, best, logits_out, out_stride, C}, B, n, stream);
}

extern "C" int srwn_stream_mol_score_head(const void* z, int64_t z_layer_stride, int64_t z_clip_rows, int32_t nlayers,
                                          const void* wskip, const float* bs_sum, const void* w1, const float* b1,
                                          const void* w2, const float* b2, const float* x, int64_t x_stride, float* nll,
                                          float* logits_out, int64_t out_stride, int32_t B, int32_t n, int32_t max_chunk,
                                          int32_t R, int32_t S, int32_t M, int32_t dtype, void* stream) {
  return score_head_impl<true>("stream_mol_score_head", z, z_layer_stride, z_clip_rows, nlayers, wskip, bs_sum, w1, b1, w2,
                               b2, HeadRows{nullptr, x, x_stride, nll, nullptr, logits_out, out_stride, M}, B, n, max_chunk,
                               R, S, dtype, stream);
}

extern "C" int srwn_mol_score_rows(const float* logits, int64_t logits_ld, int64_t logits_clip_rows, const float* x,
                                   int64_t x_stride, float* nll, float* logits_out, int64_t out_stride, int32_t B, int32_t n,
                                   int32_t M, void* stream) {
  return score_rows_impl<true>("mol_score_rows", logits, logits_ld, logits_clip_rows,
                               HeadRows{nullptr, x, x_stride, nll, nullptr, logits_out, out_stride, M}, B, n, stream);
}

// ---- scorer pools (srwn.h, srwn_version() 118): each names itself and says which form it is
extern "C" int srwn_score_stream_in_slots(const float* audio_ring, int32_t ring_len, const float* init_w, const float* init_b,
                                          void* out, int64_t out_clip_rows, int32_t out_hist, int32_t* codes,
                                          int64_t codes_stride, int32_t capacity, int32_t n, int32_t max_chunk, int32_t R,
                                          int32_t C, int32_t dtype, const SrwnSynthSlot* slots, void* stream) {
  return score_stream_in_slots_impl("score_stream_in_slots", audio_ring, ring_len, init_w, init_b, out, out_clip_rows, out_hist,
                                    codes, codes_stride, capacity, n, max_chunk, R, C, dtype, slots, stream);
}

extern "C" int srwn_stream_score_head_slots(const void* z, int64_t z_layer_stride, int64_t z_clip_rows, int32_t nlayers,
                                            const void* wskip, const float* bs_sum, const void* w1, const float* b1,
                                            const void* w2, const float* b2, const int32_t* codes, float* nll, int32_t* best,
                                            float* logits_out, int64_t out_stride, int32_t capacity, int32_t n,
                                            int32_t max_chunk, int32_t R, int32_t S, int32_t C, int32_t dtype,
                                            const SrwnSynthSlot* slots, void* stream) {
  return score_head_impl<false, true>("stream_score_head_slots", z, z_layer_stride, z_clip_rows, nlayers, wskip, bs_sum, w1, b1,
                                      w2, b2, HeadRows{codes, nullptr, 0, nll, best, logits_out, out_stride, C}, capacity, n,
                                      max_chunk, R, S, dtype, stream, SlotsArg<true>{slots});
}

extern "C" int srwn_nll_rows_slots(const float* logits, int64_t logits_ld, int64_t logits_clip_rows, const int32_t* codes,
                                   float* nll, int32_t* best, float* logits_out, int64_t out_stride, int32_t capacity,
                                   int32_t n, int32_t C, const SrwnSynthSlot* slots, void* stream) {
  return score_rows_impl<false, true>("nll_rows_slots", logits, logits_ld, logits_clip_rows,
                                      HeadRows{codes, nullptr, 0, nll, best, logits_out, out_stride, C}, capacity, n, stream,
                                      SlotsArg<true>{slots});
}

// ---- mixture-of-logistics scorer pools (srwn.h, srwn_version() 119)
extern "C" int srwn_mol_score_stream_in_slots(const float* audio_ring, int32_t ring_len, const float* init_w,
                                              const float* init_b, const void* cond0, int32_t cond_frames, int32_t pool_stride,
                                              int64_t cond_row_stride, void* out, int64_t out_clip_rows, int32_t out_hist,
                                              float* x_out, int64_t x_stride, int32_t capacity, int32_t n, int32_t max_chunk,
                                              int32_t R, int32_t dtype, const SrwnSynthSlot* slots, void* stream) {
  return mol_score_stream_in_slots_impl("mol_score_stream_in_slots", audio_ring, ring_len, init_w, init_b, cond0, cond_frames,
                                        pool_stride, cond_row_stride, out, out_clip_rows, out_hist, x_out, x_stride, capacity, n,
                                        max_chunk, R, dtype, slots, stream);
}

extern "C" int srwn_stream_mol_score_head_slots(const void* z, int64_t z_layer_stride, int64_t z_clip_rows, int32_t nlayers,
                                                const void* wskip, const float* bs_sum, const void* w1, const float* b1,
                                                const void* w2, const float* b2, const float* x, int64_t x_stride, float* nll,
                                                float* logits_out, int64_t out_stride, int32_t capacity, int32_t n,
                                                int32_t max_chunk, int32_t R, int32_t S, int32_t M, int32_t dtype,
                                                const SrwnSynthSlot* slots, void* stream) {
  return score_head_impl<true, true>("stream_mol_score_head_slots", z, z_layer_stride, z_clip_rows, nlayers, wskip, bs_sum, w1,
                                     b1, w2, b2, HeadRows{nullptr, x, x_stride, nll, nullptr, logits_out, out_stride, M},
                                     capacity, n, max_chunk, R, S, dtype, stream, SlotsArg<true>{slots});
}

extern "C" int srwn_mol_score_rows_slots(const float* logits, int64_t logits_ld, int64_t logits_clip_rows, const float* x,
                                         int64_t x_stride, float* nll, float* logits_out, int64_t out_stride, int32_t capacity,
                                         int32_t n, int32_t M, const SrwnSynthSlot* slots, void* stream) {
  return score_rows_impl<true, true>("mol_score_rows_slots", logits, logits_ld, logits_clip_rows,
                                     HeadRows{nullptr, x, x_stride, nll, nullptr, logits_out, out_stride, M}, capacity, n, stream,
                                     SlotsArg<true>{slots});
}
