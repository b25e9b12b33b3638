// Sampling controls of the generators (srwn.h, SrwnGenSampling): temperature, top-k and nucleus (top-p) filtering of one
// softmax row inside one wave, and the temperature of the mixture-of-logistics head.  One device function serves the two
// generator bodies (srwn_gen.hip, srwn_gen16.hip) and the stand-alone srwn_sample_filtered (srwn_ops.hip).
//
// A row of C <= 256 fp32 logits sits as 4 classes per lane over the 64 lanes (lane l: classes 4l .. 4l+3), as in the
// plain sampler.  The order of the rule -- logits descending, equal values by lower class first -- is taken on the
// RAW logits (z = logit / tau is monotone in the logit for tau > 0: the exact order of z, without the ties a rounded
// quotient adds) through their order-preserving integer image.  Top-k and the nucleus are radix selects over that
// image, most significant bit first, at most 32 rounds each, with no sort and no memory: a round of top-k is a compare
// per held class and a wave count (ballot + popcount, on the scalar unit), and the rounds end at the first threshold
// with exactly k keys at or above it; a round of the nucleus is a masked wave sum of exp values (four DPP steps inside
// the rows of 16 lanes, four v_readlane across them).  A class that is not kept has key 0, below every threshold.
// Classes equal to the threshold are admitted by their rank in class order (lane-prefix popcounts).  The draw is the
// plain sampler's: inclusive prefix sums in class order over exp((logit - max) / tau) of the kept classes, first class
// whose prefix sum exceeds uniform * total.
#pragma once
#include "srwn_common.h"
#include "../../include/srwn.h"

namespace srwn {
namespace samp {

// one utterance's controls as the kernels use them: out-of-range fields count as their defaults (srwn.h)
struct Ctl {
  float tau, top_p;
  int top_k;
  int on;      // any field differs from its default: the row takes the selection code
};

__device__ __forceinline__ Ctl sanitise(const SrwnGenSampling* s, int u, int C) {
  Ctl c{1.0f, 1.0f, 0, 0};
  if (s) {
    const SrwnGenSampling r = s[u];
    if (r.temperature > 0.0f && r.temperature < INFINITY) c.tau = r.temperature;      // (a NaN fails both tests)
    if (r.top_p > 0.0f && r.top_p <= 1.0f) c.top_p = r.top_p;
    if (r.top_k >= 1 && r.top_k < C) c.top_k = r.top_k;                               // (k = C keeps every class: off)
    c.on = (c.tau != 1.0f || c.top_p != 1.0f || c.top_k != 0) ? 1 : 0;
  }
  return c;
}

__device__ __forceinline__ float uniform_f(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}

template <int CTRL>
__device__ __forceinline__ float dpp(float x) {      // the value of the lane the DPP control names, inside a row of 16
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, false));
}
constexpr int kQuadXor1 = 0xB1, kQuadXor2 = 0x4E, kRowHalfMirror = 0x141, kRowMirror = 0x140;

// sum / max over the 64 lanes, the same bits in every lane (every lane of a row adds the same pairs; the four row values
// are combined in one fixed order).  All 64 lanes must be active.
__device__ __forceinline__ float wave_sum(float x) {
  x += dpp<kQuadXor1>(x);
  x += dpp<kQuadXor2>(x);
  x += dpp<kRowHalfMirror>(x);
  x += dpp<kRowMirror>(x);
  const int xi = __builtin_bit_cast(int, x);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 48));
  return (r0 + r1) + (r2 + r3);
}
__device__ __forceinline__ float wave_max(float x) {
  x = fmaxf(x, dpp<kQuadXor1>(x));
  x = fmaxf(x, dpp<kQuadXor2>(x));
  x = fmaxf(x, dpp<kRowHalfMirror>(x));
  x = fmaxf(x, dpp<kRowMirror>(x));
  const int xi = __builtin_bit_cast(int, x);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 48));
  return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

__device__ __forceinline__ unsigned long long ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// a > b as floats  <=>  order_key(a) > order_key(b)   (-0 is folded into +0 by the caller)
__device__ __forceinline__ unsigned order_key(float x) {
  const unsigned b = __builtin_bit_cast(unsigned, x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// The code of one row under (tau, top_k, top_p) -- sanitised: tau finite > 0, top_k in [0, C), 0 < top_p <= 1 -- and the
// step's uniform.  lg: the lane's four logits (classes 4 lane + e; entries at or beyond C are ignored).  Called by all 64
// lanes with wave-uniform (C, tau, top_k, top_p, uni); returns the same code in every lane, always a kept class in [0, C).
__device__ __forceinline__ int filtered_code(const f32x4& lg, int C, float tau_, int top_k_, float top_p_, float uni_,
                                             int lane) {
  const float tau = uniform_f(tau_), top_p = uniform_f(top_p_), uni = uniform_f(uni_);
  const int top_k = __builtin_amdgcn_readfirstlane(top_k_);
  float v[4];
  unsigned key[4];
  bool keep[4];
  float m = -INFINITY;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    keep[e] = 4 * lane + e < C;
    v[e] = lg[e] + 0.0f;                                   // (-0 -> +0: equal values, equal keys)
    key[e] = keep[e] ? order_key(v[e]) : 0u;               // (0: below every threshold the selects try)
    if (keep[e]) m = fmaxf(m, v[e]);
  }
  m = wave_max(m);
  const unsigned long long below = (1ull << lane) - 1ull;  // the lanes of lower classes

  if (top_k > 0) {
    // T = the k-th largest key: the largest T with at least k keys >= T, one bit a round; a T with exactly k keys >= T
    // already names the set, and the rounds end there (they run to the last bit only where keys tie at the k-th place)
    unsigned T = 0;
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      const unsigned cand = T | (1u << b);
      int cnt = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) cnt += __popcll(ballot(key[e] >= cand));
      if (cnt >= top_k) T = cand;
      if (cnt == top_k) break;
    }
    int above = 0, rank = 0;                               // keys above T; keys equal to T in lower lanes
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      above += __popcll(ballot(key[e] > T));
      rank += __popcll(ballot(keep[e] && key[e] == T) & below);
    }
    const int need = top_k - above;                        // >= 1 of the classes equal to T, the lower classes first
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool eq = keep[e] && key[e] == T;
      keep[e] = keep[e] && (key[e] > T || (eq && rank < need));
      if (eq) ++rank;
      if (!keep[e]) key[e] = 0u;
    }
  }

  float ev[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) ev[e] = keep[e] ? __expf((v[e] - m) / tau) : 0.0f;

  if (top_p < 1.0f) {
    // the shortest prefix of the order whose mass reaches top_p of the kept mass: T = the largest key with
    // mass(keys >= T) >= want, then as many of the classes equal to T (equal logits: equal masses) as it still takes
    const float total = wave_sum((ev[0] + ev[1]) + (ev[2] + ev[3]));
    const float want = top_p * total;
    unsigned T = 0;
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      const unsigned cand = T | (1u << b);
      float part[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) part[e] = key[e] >= cand ? ev[e] : 0.0f;
      const float s = uniform_f(wave_sum((part[0] + part[1]) + (part[2] + part[3])));
      if (s >= want) T = cand;
    }
    float part[4];
    int rank = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      part[e] = key[e] > T ? ev[e] : 0.0f;                 // (T >= the smallest kept key > 0)
      rank += __popcll(ballot(keep[e] && key[e] == T) & below);
    }
    const float over = wave_sum((part[0] + part[1]) + (part[2] + part[3]));      // the mass strictly above T: < want
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool eq = keep[e] && key[e] == T;
      // the class of rank r among the equals stays while the prefix before it has not reached want (the first always)
      keep[e] = keep[e] && (key[e] > T || (eq && (rank == 0 || over + (float)rank * ev[e] < want)));
      if (eq) ++rank;
      if (!keep[e]) ev[e] = 0.0f;
    }
  }

  // the plain sampler's draw over the kept classes, in class order (dropped classes count 0)
  const float loc = ev[0] + ev[1] + ev[2] + ev[3];
  float inc = loc;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  const float total = __shfl(inc, 63);
  const float target = uni * total;
  const unsigned long long hit = ballot(inc > target);
  int code;
  if (hit) {
    const int src = __ffsll((long long)hit) - 1;
    const float run = inc - loc;
    int pick = -1, last = 4 * lane;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (keep[e]) last = 4 * lane + e;                    // the lane's last kept class
#pragma unroll
    for (int e = 3; e >= 0; --e) {
      if (keep[e] &&
          run + ev[0] + (e > 0 ? ev[1] : 0.f) + (e > 1 ? ev[2] : 0.f) + (e > 2 ? ev[3] : 0.f) > target)
        pick = 4 * lane + e;
    }
    if (pick < 0) pick = last;                             // (the re-added sums fell short of the scan's: the last kept one)
    code = __shfl(pick, src);
  } else {
    // uniform * total rounded up to the total (or a row without finite mass): the last kept class
    code = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned long long kb = ballot(keep[e]);
      if (kb) {
        const int c = 4 * (63 - __clzll((long long)kb)) + e;
        code = c > code ? c : code;
      }
    }
  }
  code = code < 0 ? 0 : (code >= C ? C - 1 : code);
  return __builtin_amdgcn_readfirstlane(code);
}

}  // namespace samp
}  // namespace srwn
