// The mu-law encode of one sample (ops.py:82-93), once: srwn_mu_law_encode's kernel (srwn_util.hip) and the scorer pool's
// entry (srwn_score.hip: srwn_score_stream_in_slots) call this routine, so a target code has the same bits wherever it
// was made.  mu = Q - 1 and log1p_mu = (float)log1p((double)mu) come from the host.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace srwn {

__device__ __forceinline__ int32_t mu_law_encode_one(float a, float mu, float log1p_mu) {
  float safe = fminf(fabsf(a), 1.0f);                              // ops.py:88
  float lm = (float)log1p((double)__fmul_rn(mu, safe));             // correctly rounded f32 log1p
  float magnitude = __fdiv_rn(lm, log1p_mu);                        // ops.py:89
  float sgn = (a > 0.0f) ? 1.0f : ((a < 0.0f) ? -1.0f : 0.0f);      // tf.sign
  float signal = __fmul_rn(sgn, magnitude);                         // ops.py:90
  float q = __fadd_rn(__fmul_rn(__fdiv_rn(__fadd_rn(signal, 1.0f), 2.0f), mu), 0.5f);  // ops.py:92
  return (int32_t)q;                                                // tf.to_int32 truncates
}

}  // namespace srwn
