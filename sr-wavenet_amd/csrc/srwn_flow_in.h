// The flow entry's arithmetic on one row (RightShift, the K = 2 entry conv and the first layer's conditioning bias), once:
// flow_stream_in_kernel (srwn_stream.hip: srwn_flow_stream_in and its slot form) and the mixture-of-logistics scorer pool's
// entry (srwn_score.hip: srwn_mol_score_stream_in_slots) call this routine, so the first stack row of a sample has the same
// bits whether its two taps came from a staged chunk and its carry or from a pool's audio ring.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "srwn_common.h"

namespace srwn {

template <typename T> struct Row8s;
template <> struct Row8s<bf16_t> {
  static __device__ __forceinline__ void load(const bf16_t* p, float (&v)[8]) {
    const bf16x8 r = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)r[j];
  }
};
template <> struct Row8s<float> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
  }
};

// Channels [8 * sub, 8 * sub + 8) of the row at absolute time tabs of stream b, row out_row of `out` [rows][R], x0 =
// x[tabs - 2] and x1 = x[tabs - 1]:
//   v = b; v = fma(x0, w[0], v); v = fma(x1, w[1], v); round to T        (srwn_causal_conv1d_fwd, shift 1)
//   d = round to T ((float)v + cond[b, tabs / pool])                      (srwn_add_frame_bias)
// The conditioning table is a ring of cond_frames rows per stream (srwn.h): frame q of the stream lives in row
// q mod cond_frames.  A stream that got its whole encoding at the start has q < cond_frames: the identity.
template <typename T>
__device__ __forceinline__ void flow_entry_row(float x0, float x1, const float* w, const float* bias, const T* cond,
                                               int cond_frames, int pool, int64_t cond_stride, int b, long long tabs, T* out,
                                               int64_t out_row, int R, int sub) {
  long long f = tabs / pool;
  if (f >= cond_frames) f %= cond_frames;
  float c[8];
  Row8s<T>::load(cond + ((int64_t)b * cond_frames + f) * cond_stride + 8 * sub, c);
  T* d = out + out_row * R + 8 * sub;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = bias[8 * sub + j];
    v = fmaf(x0, w[8 * sub + j], v);
    v = fmaf(x1, w[R + 8 * sub + j], v);
    const T vr = (T)v;
    d[j] = (T)((float)vr + c[j]);
  }
}

}  // namespace srwn
