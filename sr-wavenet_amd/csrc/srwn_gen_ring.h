// What the two queue-cached generator bodies (srwn_gen.hip: throughput, srwn_gen16.hip: latency) share besides the
// sampling controls of srwn_sample.h: the layout of the layer rings, the samplers' uniform and the mu-law decode.
#pragma once
#include <cstdint>
#include "srwn_common.h"

namespace srwn {

constexpr int kGenMaxLayers = 64;   // entries of the kernels' dil[] / ring_off[] argument arrays

// The rings of one group of 32 utterances: layer l keeps its last dilations[l] + 1 inputs, [32][R] each, the layers back to
// back.  Returns the elements of one group and sets *bad to the first layer whose dilation is outside [1, max_dil] (-1:
// none; the caller reports it under its own name).  With dil / ring_off (kGenMaxLayers entries each, nlayers <=
// kGenMaxLayers) it fills the kernels' tables: the layers' dilations and element offsets, then dilation 1 at the end offset.
inline long long gen_ring_layout(const int32_t* dilations, int nlayers, int R, int max_dil, int* bad, int* dil = nullptr,
                                 long long* ring_off = nullptr) {
  long long off = 0;
  *bad = -1;
  for (int l = 0; l < nlayers; ++l) {
    if (*bad < 0 && (dilations[l] < 1 || dilations[l] > max_dil)) *bad = l;
    if (dil) { dil[l] = dilations[l]; ring_off[l] = off; }
    off += ((long long)dilations[l] + 1) * 32 * R;
  }
  for (int l = nlayers; dil && l < kGenMaxLayers; ++l) { dil[l] = 1; ring_off[l] = off; }
  return off;
}

__device__ __forceinline__ float gen_mu_law_decode(int code, int Q) {   // ops.py:96-104, as srwn_mu_law_decode
  const float mu = (float)(Q - 1);
  const float signal = __fadd_rn(__fmul_rn(2.0f, __fdiv_rn((float)code, mu)), -1.0f);
  const float p = (float)pow((double)Q, (double)fabsf(signal));
  const float magnitude = __fmul_rn((float)(1.0 / (double)(Q - 1)), __fadd_rn(p, -1.0f));
  const float sgn = (signal > 0.0f) ? 1.0f : ((signal < 0.0f) ? -1.0f : 0.0f);
  return __fmul_rn(sgn, magnitude);
}

// the samplers' uniform in (0, 1): a counter-based draw of (seed, utterance, step), so that any split of a run into launches
// and either body give the same bits
__device__ __forceinline__ float gen_uniform(unsigned long long seed, unsigned u, unsigned t) {
  unsigned long long x = seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)u * 0x100000001ull + t + 1);
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
  return (float)((x >> 40) + 0.5) * (1.0f / 16777216.0f);
}

// the live slot form: the row of a slot's own frame f in its ring of n conditioning frames -- a true modulus, inside the
// table for the negative or garbage frames an idle slot may hold
__device__ __forceinline__ int gen_ring_row(int f, int n) {
  const int r = f % n;
  return r < 0 ? r + n : r;
}

}  // namespace srwn
