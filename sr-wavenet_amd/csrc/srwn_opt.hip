// Optimizer: tf.train.AdamOptimizer semantics (model.py:31,117,382) on the flat fp32 parameter buffer.
#include "srwn_common.h"
#include "srwn_host.h"
#include "../../include/srwn.h"

using namespace srwn;

// The step counter lives on the device so that a captured hipGraph replays with the right bias correction.  It is ticked
// INSIDE the update launch (it used to be a one-thread launch of its own in front of it: ~5 us + a launch boundary per
// step): every block reads t = count + 1 when it starts; each block adds one to an arrival counter when it is done, and
// the block whose add comes last -- every other block has read the count by then -- stores the new count.  No payload
// crosses workgroups: the arrival counter is the upper half of the 64-bit step word, zero again when the launch ends
// (the final store writes the whole word), so the word reads as a plain int64 step count between launches.
constexpr int kAdamBlocks = 256;      // one block per CU
static unsigned adam_grid(int64_t n) {
  const int64_t b = (n + 1023) / 1024;
  return (unsigned)(b < kAdamBlocks ? b : kAdamBlocks);
}
static int adam_vec(const void* a, const void* b, const void* c, const void* d, const void* e = nullptr) {
  return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d) | ((uintptr_t)e)) & 15) == 0;
}

// One parameter's update: the arithmetic of both kernels below (same expressions, same contraction, same bits).
__device__ __forceinline__ void adam_one(float gi, float& mi, float& vi, float& th, float grad_scale, float b1, float b2,
                                         float lr_t, float eps) {
  gi *= grad_scale;
  mi = b1 * mi + (1.0f - b1) * gi;
  vi = b2 * vi + (1.0f - b2) * gi * gi;
  th -= lr_t * mi / (sqrtf(vi) + eps);
}
// lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t); epsilon is added to the UNcorrected sqrt(v) (TF formula)
__device__ __forceinline__ float adam_lr_t(float lr, float b1, float b2, int t_) {
  const double t = (double)t_;
  return (float)((double)lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
}
// tf's assign_moving_average behind the update, as three separately rounded fp32 operations: separate STATEMENTS, since
// -ffp-contract=on fuses inside one expression only (v_mul_f32 + v_sub_f32 here; `e - s * (e - th)` gives v_fma_f32)
__device__ __forceinline__ float ema_one(float e, float th, float s) {
  const float diff = e - th;
  const float p = s * diff;
  const float out = e - p;
  return out;
}
// The arrival half of the tick (see the top of the file): thread 0 of every block, after its block's last store.
__device__ __forceinline__ void adam_arrive(int64_t* step, int t) {
  unsigned* arrived = reinterpret_cast<unsigned*>(step) + 1;
  const unsigned prev = __hip_atomic_fetch_add(arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (prev == gridDim.x - 1)      // the last block: the new count, the arrival counter back to zero, in one 8-byte store
    __hip_atomic_store(step, (int64_t)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Four parameters per thread; the bias-corrected step size (two fp64 pow per call of the TF formula) is computed once
// per block and broadcast -- every thread used to evaluate it for itself, which made a 28-MB streaming kernel
// instruction-bound (18 us for 1 M parameters).  Same expression, same bits.
__global__ __launch_bounds__(256) void adam_step_kernel(float* __restrict__ theta, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                        int64_t* step, int tick, float lr, float b1, float b2,
                                                        float eps, float grad_scale,
                                                        const float* __restrict__ scale_dev, int vec) {
  __shared__ float s_lr;
  __shared__ int s_t;
  if (threadIdx.x == 0) {
    // (an sc1 load: the low word only -- the upper one is the arrival counter of this very launch)
    const int count = __hip_atomic_load(reinterpret_cast<int*>(step), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_t = count + (tick ? 1 : 0);
    s_lr = adam_lr_t(lr, b1, b2, s_t);
  }
  __syncthreads();
  const float lr_t = s_lr;
  if (scale_dev) grad_scale *= scale_dev[0];
  auto one = [&](float gi, float& mi, float& vi, float& th) { adam_one(gi, mi, vi, th, grad_scale, b1, b2, lr_t, eps); };
  // at most kAdamBlocks blocks walk the buffer (grid stride): every block is one arrival on ONE counter, and arrivals on
  // one address are served one after the other at the memory side (~12 ns each: 980 blocks -- one per 1024 parameters --
  // made this a 18-us kernel; 256 arrivals cost ~3 us)
  for (int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i0 < n; i0 += (int64_t)gridDim.x * blockDim.x * 4) {
    if (vec && i0 + 4 <= n) {      // vec: all four buffers 16-byte aligned (host check)
      typedef float f4 __attribute__((ext_vector_type(4)));
      f4 gg = *reinterpret_cast<const f4*>(g + i0), mm = *reinterpret_cast<f4*>(m + i0), vv = *reinterpret_cast<f4*>(v + i0),
         tt = *reinterpret_cast<f4*>(theta + i0);
#pragma unroll
      for (int j = 0; j < 4; ++j) { float a = mm[j], b = vv[j], c = tt[j]; one(gg[j], a, b, c); mm[j] = a; vv[j] = b; tt[j] = c; }
      *reinterpret_cast<f4*>(m + i0) = mm;
      *reinterpret_cast<f4*>(v + i0) = vv;
      *reinterpret_cast<f4*>(theta + i0) = tt;
    } else {
      for (int64_t i = i0; i < n && i < i0 + 4; ++i) one(g[i], m[i], v[i], theta[i]);
    }
  }
  if (tick && threadIdx.x == 0) adam_arrive(step, s_t);      // (thread 0 read the count before this point: program order)
}

// The same update under training controls: the learning rate and the EMA decay of step t (the count after the tick) come
// from row min(t - 1, H - 1) of a device table [H][2] = {lr, ema_decay}, H itself from device memory, so that a captured
// graph follows a table rewritten in place; the shadow `ema` (or null) is updated right behind theta, from the theta this
// thread has just computed: no second pass over the parameters, no second launch.  `cap` is the allocated row count: H is
// held to [1, cap] so that a stale length can never read past the table.  Every thread derives the row for itself from
// the two shared scalars (uniform loads), which keeps the LDS at those two.
__global__ __launch_bounds__(256) void adam_step_ctl_kernel(float* __restrict__ theta, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v,
                                                            float* __restrict__ ema, int64_t n, int64_t* step, int tick,
                                                            const float* __restrict__ ctl, const int* __restrict__ ctl_len,
                                                            int cap, float b1, float b2, float eps, float grad_scale,
                                                            const float* __restrict__ scale_dev, int vec) {
  __shared__ float s_lr;
  __shared__ int s_t;
  int H = ctl_len[0];
  H = H < 1 ? 1 : (H > cap ? cap : H);
  if (threadIdx.x == 0) {
    const int count = __hip_atomic_load(reinterpret_cast<int*>(step), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_t = count + (tick ? 1 : 0);
    int row = s_t - 1 < H - 1 ? s_t - 1 : H - 1;
    row = row < 0 ? 0 : row;
    s_lr = adam_lr_t(ctl[2 * row], b1, b2, s_t);
  }
  __syncthreads();
  const float lr_t = s_lr;
  int row = s_t - 1 < H - 1 ? s_t - 1 : H - 1;
  row = row < 0 ? 0 : row;
  const float s = 1.0f - ctl[2 * row + 1];
  if (scale_dev) grad_scale *= scale_dev[0];
  for (int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i0 < n; i0 += (int64_t)gridDim.x * blockDim.x * 4) {
    if (vec && i0 + 4 <= n) {      // vec: all buffers 16-byte aligned (host check)
      typedef float f4 __attribute__((ext_vector_type(4)));
      f4 gg = *reinterpret_cast<const f4*>(g + i0), mm = *reinterpret_cast<f4*>(m + i0), vv = *reinterpret_cast<f4*>(v + i0),
         tt = *reinterpret_cast<f4*>(theta + i0), ee = {0.f, 0.f, 0.f, 0.f};
      if (ema) ee = *reinterpret_cast<f4*>(ema + i0);
#pragma unroll
      for (int j = 0; j < 4; ++j) { float a = mm[j], b = vv[j], c = tt[j]; adam_one(gg[j], a, b, c, grad_scale, b1, b2, lr_t, eps); mm[j] = a; vv[j] = b; tt[j] = c; }
      *reinterpret_cast<f4*>(m + i0) = mm;
      *reinterpret_cast<f4*>(v + i0) = vv;
      *reinterpret_cast<f4*>(theta + i0) = tt;
      if (ema) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ee[j] = ema_one(ee[j], tt[j], s);
        *reinterpret_cast<f4*>(ema + i0) = ee;
      }
    } else {
      for (int64_t i = i0; i < n && i < i0 + 4; ++i) {
        float a = m[i], b = v[i], c = theta[i];
        adam_one(g[i], a, b, c, grad_scale, b1, b2, lr_t, eps);
        m[i] = a; v[i] = b; theta[i] = c;
        if (ema) ema[i] = ema_one(ema[i], c, s);
      }
    }
  }
  if (tick && threadIdx.x == 0) adam_arrive(step, s_t);
}

extern "C" int srwn_adam_step(float* params, const float* grads, float* m, float* v, int64_t n, int64_t* step,
                              float lr, float beta1, float beta2, float eps, float grad_scale, void* stream) {
  if (n == 0) return 0;
  if (!params || !grads || !m || !v || !step) return set_error(SRWN_E_NULL, "adam_step: null pointer");
  if (n < 0) return set_error(SRWN_E_SHAPE, "adam_step: n=%lld", (long long)n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adam_step_kernel, dim3(adam_grid(n)), dim3(256), 0, st, params, grads, m, v, n,
                     step, 1, lr, beta1, beta2, eps, grad_scale, (const float*)nullptr, adam_vec(params, grads, m, v));
  return check_launch("adam_step");
}

// Same update with the gradient scale read from device memory (the clip factor of srwn_clip_scale);
// `tick` = 0 lets several parameter buffers share one step counter (tick it on the first call only).
extern "C" int srwn_adam_step_scaled(float* params, const float* grads, float* m, float* v, int64_t n, int64_t* step,
                                     float lr, float beta1, float beta2, float eps, const float* grad_scale_dev,
                                     int32_t tick, void* stream) {
  if (n == 0) return 0;
  if (!params || !grads || !m || !v || !step || !grad_scale_dev)
    return set_error(SRWN_E_NULL, "adam_step_scaled: null pointer");
  if (n < 0) return set_error(SRWN_E_SHAPE, "adam_step_scaled: n=%lld", (long long)n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adam_step_kernel, dim3(adam_grid(n)), dim3(256), 0, st, params, grads, m, v, n,
                     step, tick ? 1 : 0, lr, beta1, beta2, eps, 1.0f, grad_scale_dev, adam_vec(params, grads, m, v));
  return check_launch("adam_step_scaled");
}

// The update under training controls (srwn.h): lr and EMA decay from the device table, the clip factor from device memory
// (or null), the shadow in the same pass (or null).
extern "C" int srwn_adam_step_ctl(float* params, const float* grads, float* m, float* v, float* ema, int64_t n,
                                  int64_t* step, const float* ctl, const int32_t* ctl_len, int32_t ctl_capacity,
                                  float beta1, float beta2, float eps, float grad_scale, const float* grad_scale_dev,
                                  int32_t tick, void* stream) {
  if (n == 0) return 0;
  if (!params || !grads || !m || !v || !step) return set_error(SRWN_E_NULL, "adam_step_ctl: null pointer");
  if (!ctl || !ctl_len) return set_error(SRWN_E_NULL, "adam_step_ctl: null control table or length");
  if (n < 0) return set_error(SRWN_E_SHAPE, "adam_step_ctl: n=%lld", (long long)n);
  if (ctl_capacity < 1) return set_error(SRWN_E_SHAPE, "adam_step_ctl: ctl_capacity=%d", (int)ctl_capacity);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adam_step_ctl_kernel, dim3(adam_grid(n)), dim3(256), 0, st, params, grads, m, v, ema, n, step,
                     tick ? 1 : 0, ctl, (const int*)ctl_len, (int)ctl_capacity, beta1, beta2, eps, grad_scale,
                     grad_scale_dev, adam_vec(params, grads, m, v, ema));
  return check_launch("adam_step_ctl");
}
