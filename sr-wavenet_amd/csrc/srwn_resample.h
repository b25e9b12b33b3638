// What the resampling draw launches share (csrc/srwn_resample.hip, csrc/srwn_room.hip): a row's step as
// dataset.speed_plan states it, dataset.resample_rows for a few outputs at once, a destination's position against the
// 16-byte boundaries, and the host-side check of the resampling block.
#pragma once
#include "srwn_common.h"
#include "srwn_augment.h"
#include "srwn_draw_common.h"
#include "srwn_host.h"
#include "srwn_mulaw.h"
#include "../../include/srwn.h"

namespace srwn {

constexpr unsigned long long kAugSpeedSalt = 0x6175677370656564ull;    // dataset.AUG_SPEED_SALT
constexpr int kSpeedBits = 24;                                         // dataset.SPEED_BITS
constexpr int kPhases = SRWN_RESAMPLE_PHASES;                          // dataset.RESAMPLE_PHASES
constexpr int kPhaseBits = __builtin_ctz(kPhases);
static_assert((kPhases & (kPhases - 1)) == 0 && kPhaseBits <= kSpeedBits, "a power of two of at most 2^24 phases");

struct WarpArgs { const float* table; int32_t taps, step_lo, step_hi; };

// one row's resampling: its step (dataset.speed_plan) and the table
struct WarpRow { const float* table; unsigned long long step; int taps; };

__device__ __forceinline__ WarpRow warp_row(const WarpArgs& w, unsigned long long seed, unsigned long long p, int side) {
  const unsigned long long key = kGolden * (2ull * p + (unsigned long long)side + 1ull);
  const unsigned long long h = mix64((seed ^ kAugSpeedSalt) + key);
  WarpRow r;
  r.table = w.table;
  r.taps = w.taps;
  r.step = (unsigned long long)w.step_lo + (((h >> 32) * (unsigned long long)(w.step_hi - w.step_lo + 1)) >> 32);
  return r;
}

// dataset.resample_rows for kN outputs at once, jj[u] each in [0, T), of the row at src.  The tap loop is the restatement's:
// all `taps` taps in order, a sample outside the row read as +0 (its index is clamped for the load, the value selected), so
// the loop's trip count is the same in every lane and the loads of kN outputs and several taps are in flight together --
// one tap at a time, the launch waits for one cache round trip per tap and output.
template <int kN>
__device__ __forceinline__ void warp_samples(const float* __restrict__ src, const WarpRow& w, const int (&jj)[kN], int T,
                                             float (&acc)[kN]) {
  long long first[kN];                                            // the source sample under tap 0
  const float* h[kN];                                             // the output's table row
#pragma unroll
  for (int u = 0; u < kN; ++u) {
    const unsigned long long q = (unsigned long long)jj[u] * w.step;                 // < 2^31 * 2^25
    first[u] = (long long)(q >> kSpeedBits) - (long long)(w.taps / 2 - 1);
    const unsigned f = (unsigned)(q >> (kSpeedBits - kPhaseBits)) & (unsigned)(kPhases - 1);
    h[u] = w.table + (size_t)f * (size_t)w.taps;
    acc[u] = 0.0f;
  }
#pragma unroll 2
  for (int k = 0; k < w.taps; k += 2) {                           // (taps is even)
#pragma unroll
    for (int u = 0; u < kN; ++u) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const long long at = first[u] + k + e;
        const int m = (at >= 0 && at < (long long)T) ? -1 : 0;   // all ones inside the row: a mask in a vector register
        const float x = src[at & (long long)m];                   // (index 0 outside: always inside the row)
        acc[u] = __fadd_rn(acc[u], __fmul_rn(h[u][k + e], __int_as_float(__float_as_int(x) & m)));   // +0 outside
      }
    }
  }
}

__device__ __forceinline__ int phase16(const void* p) { return (int)(((uintptr_t)p >> 2) & 3); }

// the resampling block of both entries, checked before any launch
inline int check_resample(const char* who, const float* table, int32_t taps, int32_t step_lo, int32_t step_hi, WarpArgs* w) {
  if (taps < 2 || taps > 64 || (taps & 1)) return set_error(SRWN_E_SHAPE, "%s: %d taps (even, 2 to 64)", who, taps);
  if (step_lo > step_hi || step_lo < (1 << (kSpeedBits - 1)) || step_hi > (1 << (kSpeedBits + 1)))
    return set_error(SRWN_E_SHAPE, "%s: steps [%d, %d] outside 2^23 <= lo <= hi <= 2^25", who, step_lo, step_hi);
  if (!table) return set_error(SRWN_E_NULL, "%s: null resampling table", who);
  if ((uintptr_t)table & 3) return set_error(SRWN_E_SHAPE, "%s: the fp32 buffers must be 4-byte aligned", who);
  w->table = table; w->taps = taps; w->step_lo = step_lo; w->step_hi = step_hi;
  return 0;
}

}  // namespace srwn
