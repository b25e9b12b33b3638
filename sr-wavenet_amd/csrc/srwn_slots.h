// What the serving launches share between their clock forms and their slot forms (srwn_stream.hip, srwn_recog.hip).  The
// slot forms are the same kernels with a template flag: the clock argument becomes the pool's table (srwn.h
// SrwnSynthSlot), slot b's chunk starts at slots[b].t and has slot_rows(slots[b], n) rows.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/srwn.h"

namespace srwn {

// the clock or the table: what a kernel's SLOTS instantiation takes in the place of the clock (`in`: read only; `out`: the
// launch that advances it)
template <bool SLOTS> struct ClockArg { typedef const long long* in; typedef long long* __restrict__ out; };
template <> struct ClockArg<true> { typedef const SrwnSynthSlot* in; struct out { SrwnSynthSlot* slots; int* arrive; }; };

// rows slot `s` has in a chunk of n: clamp(t_end - t, 0, n)
__device__ __forceinline__ int slot_rows(const SrwnSynthSlot& s, int n) {
  const long long left = s.t_end - s.t;
  return left <= 0 ? 0 : (left < n ? (int)left : n);
}

// a boundary buffer of a history roll: int64 triples, as the host's roll tables hold them
struct RollEntry { void* buf; long long clip_rows; long long hist; };
static_assert(sizeof(RollEntry) == 24, "the roll table is int64 triples");

}  // namespace srwn
