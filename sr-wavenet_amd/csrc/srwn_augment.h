// What the augmenting draw launches share (csrc/srwn_augment.hip, csrc/srwn_resample.hip, csrc/srwn_room.hip): a row's draws as
// dataset.augment_plan states them, the sample rule's mix and clamp (dataset.augment_rows), the right record of a pair
// (dataset.pair_plan) and the host-side check of the augmentation block, so that a row has one plan wherever it is drawn.
#pragma once
#include "srwn_common.h"
#include "srwn_draw_common.h"
#include "srwn_host.h"
#include "../../include/srwn.h"

namespace srwn {

constexpr unsigned long long kAugShiftSalt = 0x6175677368696674ull;    // dataset.AUG_SHIFT_SALT
constexpr unsigned long long kAugGainSalt = 0x6175676761696E21ull;     // dataset.AUG_GAIN_SALT
constexpr unsigned long long kAugCoinSalt = 0x617567636F696E21ull;     // dataset.AUG_COIN_SALT
constexpr unsigned long long kAugPickSalt = 0x6175677069636B21ull;     // dataset.AUG_PICK_SALT: the noise record
constexpr unsigned long long kAugOffsetSalt = 0x6175676F66667374ull;   // dataset.AUG_OFFSET_SALT: where its window starts
constexpr unsigned long long kAugVolumeSalt = 0x617567766F6C2121ull;   // dataset.AUG_VOLUME_SALT

struct AugArgs {
  const float* noise; int64_t noise_len; unsigned long long threshold;
  int32_t noise_n, shift;
  float gain_lo, gain_hi, vol_lo, vol_hi;
};

// one row's plan, as the sample rule reads it: nz is the noise window's first sample, null where the row is not mixed
struct AugRow { const float* src; const float* nz; int shift; float gain, vol; };

// lo + u (hi - lo) at u = (h >> 40) 2^-24 (exact), three roundings
__device__ __forceinline__ float aug_amplitude(unsigned long long h, float lo, float hi) {
  const float u = __fmul_rn((float)(unsigned)(h >> 40), 1.0f / 16777216.0f);
  return __fadd_rn(lo, __fmul_rn(u, __fsub_rn(hi, lo)));
}

// dataset.augment_plan for position p and side
__device__ __forceinline__ AugRow aug_row(const AugArgs& g, unsigned long long seed, unsigned long long p, int side,
                                          const float* src, int T) {
  const unsigned long long key = kGolden * (2ull * p + (unsigned long long)side + 1ull);
  AugRow r;
  r.src = src;
  const unsigned long long hs = mix64((seed ^ kAugShiftSalt) + key);
  r.shift = (int)(((hs >> 32) * (2ull * (unsigned long long)g.shift + 1ull)) >> 32) - g.shift;
  r.gain = aug_amplitude(mix64((seed ^ kAugGainSalt) + key), g.gain_lo, g.gain_hi);
  r.nz = nullptr;
  r.vol = 0.0f;
  if (g.noise_n > 0 && (mix64((seed ^ kAugCoinSalt) + key) >> 32) < g.threshold) {
    const unsigned long long rec = ((mix64((seed ^ kAugPickSalt) + key) >> 32) * (unsigned long long)g.noise_n) >> 32;
    const unsigned long long off = ((mix64((seed ^ kAugOffsetSalt) + key) >> 32) * (unsigned long long)(g.noise_len - T + 1)) >> 32;
    r.nz = g.noise + (int64_t)rec * g.noise_len + (int64_t)off;
    r.vol = aug_amplitude(mix64((seed ^ kAugVolumeSalt) + key), g.vol_lo, g.vol_hi);
  }
  return r;
}

// dataset.augment_rows for one sample: x the shifted signal (+0 outside the row), n the noise (+0 where not mixed)
__device__ __forceinline__ float aug_mix(const AugRow& r, float x, float n) {
  const float y = __fadd_rn(__fmul_rn(r.gain, x), __fmul_rn(r.vol, n));
  return y < -1.0f ? -1.0f : (y > 1.0f ? 1.0f : y);                // (NaN passes)
}

// dataset.pair_plan (srwn_pair_draw's rule): the right record of the left record `k` of position p, its crop offset and
// the left record's label
struct PairPick { unsigned rec; int64_t off; int32_t c; };
__device__ __forceinline__ PairPick pair_pick(const PairArgs& a, unsigned long long seed, unsigned long long p, const Pick& k) {
  PairPick r;
  const int32_t c = a.labels[k.rec];
  const bool known = (unsigned)c < (unsigned)a.num_classes;       // (a PairSampler refuses labels outside the classes)
  const unsigned long long s0 = known ? (unsigned long long)a.start[c] : 0ull;
  const unsigned long long m = known ? (unsigned long long)a.start[c + 1] - s0 : 1ull;
  const unsigned long long q = known ? (unsigned long long)a.place[k.rec] - s0 : 0ull;
  const unsigned long long N = known ? (unsigned long long)a.N : 1ull;   // ... such a record is paired with itself
  const unsigned long long h1 = mix64((seed ^ kPairSalt) + kGolden * (p + 1ull));
  const unsigned long long h2 = mix64((seed ^ kPairPickSalt) + kGolden * (p + 1ull)) >> 32;
  bool same = (h1 >> 32) < a.threshold;
  if (m == 1ull) same = false;                                    // a singleton has no partner in its class
  if (N == m) same = true;                                        // one class only
  if (N == 1ull) {
    r.rec = k.rec;                                                // the only record, paired with itself
  } else if (same) {
    unsigned long long kk = (h2 * (m - 1ull)) >> 32;
    kk += (kk >= q) ? 1ull : 0ull;                                // never the left clip itself
    r.rec = (unsigned)a.order[s0 + kk];
  } else {
    const unsigned long long kk = (h2 * (N - m)) >> 32;
    r.rec = (unsigned)a.order[kk < s0 ? kk : kk + m];
  }
  r.off = 0;
  if (a.crop) {
    const unsigned long long h3 = mix64((seed ^ kPairCropSalt) + kGolden * (p + 1ull));
    r.off = (int64_t)(((h3 >> 32) * (unsigned long long)(a.clip_len - a.T + 1)) >> 32);
  }
  r.c = c;
  return r;
}

// a range [lo, hi] of amplitudes: finite, 0 <= lo <= hi (a NaN fails the comparisons)
inline bool range_ok(float lo, float hi) { return lo >= 0.0f && lo <= hi && hi <= 3.4028234664e38f; }

// the augmentation block of the augmenting entries, checked before any launch
inline int check_augment(const char* who, int32_t T, int32_t max_shift, float gain_lo, float gain_hi, const float* noise,
                         int32_t noise_clips, int64_t noise_len, int64_t noise_threshold, float volume_lo, float volume_hi,
                         AugArgs* g) {
  if (max_shift < 0 || max_shift >= T) return set_error(SRWN_E_SHAPE, "%s: shift bound %d outside [0, T=%d)", who, max_shift, T);
  if (!range_ok(gain_lo, gain_hi)) return set_error(SRWN_E_SHAPE, "%s: gain range [%g, %g]", who, gain_lo, gain_hi);
  if (!range_ok(volume_lo, volume_hi))
    return set_error(SRWN_E_SHAPE, "%s: noise volume range [%g, %g]", who, volume_lo, volume_hi);
  if (noise_clips < 0) return set_error(SRWN_E_SHAPE, "%s: %d noise clips", who, noise_clips);
  if (noise_threshold < 0 || noise_threshold > (1ll << 32))
    return set_error(SRWN_E_SHAPE, "%s: noise_threshold %lld outside [0, 2^32]", who, (long long)noise_threshold);
  if (noise_clips > 0) {
    if (!noise) return set_error(SRWN_E_NULL, "%s: %d noise clips behind a null pointer", who, noise_clips);
    if (noise_len < (int64_t)T || noise_len - T >= (1ll << 32))
      return set_error(SRWN_E_SHAPE, "%s: noise clips of %lld samples, T=%d", who, (long long)noise_len, T);
    if ((uintptr_t)noise & 3) return set_error(SRWN_E_SHAPE, "%s: the fp32 buffers must be 4-byte aligned", who);
  }
  g->noise = noise_clips > 0 ? noise : nullptr; g->noise_len = noise_clips > 0 ? noise_len : 0;
  g->threshold = (unsigned long long)noise_threshold; g->noise_n = noise_clips; g->shift = max_shift;
  g->gain_lo = gain_lo; g->gain_hi = gain_hi; g->vol_lo = volume_lo; g->vol_hi = volume_hi;
  return 0;
}

}  // namespace srwn
