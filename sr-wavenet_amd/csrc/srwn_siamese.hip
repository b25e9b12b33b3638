// Contrastive head of class SiameseWaveNet (model.py:660-797).  Each tower is class WaveNet's network up to the last
// 1x1 and the average pool over the whole clip; both towers share one set of weights, so the engine runs them as ONE
// batch of 2P rows (rows 0..P-1 the left clips, P..2P-1 the right ones) and only the head differs from the pooled
// classifier: the time-mean of srwn_time_mean goes through the last 1x1 to an embedding, and pairs are scored with the
// Hadsell-Chopra-LeCun contrastive loss under the reference's flipped label convention (y = 1: "same", model.py:747-749).
// One small VALU kernel in one workgroup (P pairs, D output dimensions): the heavy stack below it is shared.
#include "srwn_common.h"
#include "srwn_host.h"
#include "../../include/srwn.h"

using namespace srwn;

constexpr int kChThreads = 256;   // four wave64s

__device__ __forceinline__ float wave_sum(float v) {   // butterfly over all 64 lanes of a wave
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// mean [rows,S], w2 [S,ldw] (columns >= D ignored), b2 [>= D], labels [P] or null.
//   emb[r,k]  = b2[k] + sum_s mean[r,s] w2[s,k]
//   d_p       = sqrt(1e-8 + |emb[p] - emb[P+p]|^2)                                   (model.py:736)
//   loss      = (1/P) sum_p  y_p d_p^2 / 2 + (1 - y_p) max(0, m - d_p)^2 / 2          (model.py:747-749)
//   de[p]     = g_p (emb[p] - emb[P+p]) / d_p,  de[P+p] = -de[p],   g_p = (y_p d_p - (1 - y_p) max(0, m - d_p)) / P
//   gw2[s,k]  = sum_r mean[r,s] de[r,k]  = sum_p (mean[p,s] - mean[P+p,s]) de[p,k]   (columns D..ldw-1 written 0)
//   gb2[k]    = sum_r de[r,k]            = sum_p (de[p,k] + de[P+p,k])  = 0 exactly (the loss is translation-invariant)
//   dmean[r,s]= sum_k de[r,k] w2[s,k]    (the right row of a pair is the exact negation of the left one)
// LDS: e [rows*D] (the embedding, overwritten by de for the first P rows), cp [P] (g_p / d_p), lp [P] (loss terms).
__global__ __launch_bounds__(kChThreads) void contrastive_head_kernel(
    const float* __restrict__ mean, const float* __restrict__ w2, const float* __restrict__ b2,
    const float* __restrict__ labels, float margin, float* __restrict__ emb, float* __restrict__ dist,
    float* __restrict__ loss, float* __restrict__ gw2, float* __restrict__ gb2, float* __restrict__ dmean, int rows,
    int S, int D, int ldw, int pairs) {
  extern __shared__ float sh[];
  float* e = sh;
  float* cp = e + rows * D;
  float* lp = cp + pairs;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < rows * D; i += kChThreads) {
    const int r = i / D, k = i % D;
    float acc = b2[k];
    for (int s = 0; s < S; ++s) acc = fmaf(mean[r * S + s], w2[(int64_t)s * ldw + k], acc);
    e[i] = acc;
    emb[i] = acc;
  }
  if (pairs == 0) return;
  __syncthreads();
  // one wave per pair: lanes split the D dimensions, a 64-lane butterfly sums the squares
  for (int p = wave; p < pairs; p += kChThreads / 64) {
    float ss = 0.0f;
    for (int k = lane; k < D; k += 64) {
      const float df = e[p * D + k] - e[(pairs + p) * D + k];
      ss = fmaf(df, df, ss);
    }
    ss = wave_sum(ss);
    if (lane == 0) {
      const float d = sqrtf(1e-8f + ss);
      if (dist) dist[p] = d;
      if (labels) {
        const float y = labels[p];
        const float h = fmaxf(0.0f, margin - d);
        lp[p] = 0.5f * (y * d * d + (1.0f - y) * h * h);
        cp[p] = (y * d - (1.0f - y) * h) / ((float)pairs * d);
      }
    }
  }
  if (!labels) return;
  __syncthreads();
  if (wave == 0) {   // the loss: a fixed-order lane-strided sum, then the butterfly
    float part = 0.0f;
    for (int p = lane; p < pairs; p += 64) part += lp[p];
    part = wave_sum(part);
    if (lane == 0 && loss) loss[0] = part / (float)pairs;
  }
  // de for the left rows, in place of their embeddings (each element reads only itself and its right partner)
  for (int i = tid; i < pairs * D; i += kChThreads) {
    const int p = i / D;
    e[i] = cp[p] * (e[i] - e[pairs * D + i]);
  }
  __syncthreads();
  for (int i = tid; i < S * ldw; i += kChThreads) {
    const int s = i / ldw, k = i % ldw;
    float acc = 0.0f;
    if (k < D)
      for (int p = 0; p < pairs; ++p) acc = fmaf(mean[p * S + s] - mean[(pairs + p) * S + s], e[p * D + k], acc);
    gw2[i] = acc;
  }
  for (int k = tid; k < ldw; k += kChThreads) {
    float acc = 0.0f;
    if (k < D)
      for (int p = 0; p < pairs; ++p) {   // +x then -x: every pair adds exactly zero
        const float x = e[p * D + k];
        acc += x;
        acc += -x;
      }
    gb2[k] = acc;
  }
  for (int i = tid; i < pairs * S; i += kChThreads) {
    const int p = i / S, s = i % S;
    float acc = 0.0f;
    for (int k = 0; k < D; ++k) acc = fmaf(e[p * D + k], w2[(int64_t)s * ldw + k], acc);
    dmean[i] = acc;
    dmean[(int64_t)pairs * S + i] = -acc;
  }
}

extern "C" int srwn_contrastive_head(const float* mean, const float* w2, const float* b2, const float* labels,
                                     float margin, float* emb, float* dist, float* loss, float* gw2, float* gb2,
                                     float* dmean, int32_t rows, int32_t S, int32_t D, int32_t ldw, void* stream) {
  if (rows == 0) return 0;
  if (!mean || !w2 || !b2 || !emb) return set_error(SRWN_E_NULL, "contrastive_head: null pointer");
  if (labels && (!loss || !gw2 || !gb2 || !dmean))
    return set_error(SRWN_E_NULL, "contrastive_head: labels given but loss or gradient outputs missing");
  if (rows < 0 || S < 1 || D < 1 || ldw < D)
    return set_error(SRWN_E_SHAPE, "contrastive_head: rows=%d S=%d D=%d ldw=%d", rows, S, D, ldw);
  if ((labels || dist) && rows % 2)
    return set_error(SRWN_E_SHAPE, "contrastive_head: pairs need an even row count (left rows, then right), got %d", rows);
  // pairs are scored whenever labels or dist are asked for (a forward pass without either only embeds)
  const int pairs = (labels || dist) ? rows / 2 : 0;
  const size_t sh = ((size_t)rows * D + 2 * (size_t)pairs) * sizeof(float);
  if (sh > 65536)
    return set_error(SRWN_E_SHAPE, "contrastive_head: rows*D=%lld does not fit one workgroup's LDS",
                     (long long)rows * D);
  hipLaunchKernelGGL(contrastive_head_kernel, dim3(1), dim3(kChThreads), sh, (hipStream_t)stream, mean, w2, b2, labels,
                     margin, emb, dist, loss, gw2, gb2, dmean, rows, S, D, ldw, pairs);
  return check_launch("contrastive_head");
}
