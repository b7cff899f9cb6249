// The fused Adam update over one flat buffer, shared by the plain kernels (train.hip) and the guarded ones (grad_guard.hip).
// torch.optim.Adam semantics: no amsgrad, optional L2 weight decay.  step_size = lr / (1 - b1^t);  denom = sqrt(v)/sqrt(1 - b2^t) + eps
//
// GUARD = false: exactly the arithmetic the plain kernels always had (`rec` is not read).
// GUARD = true : `rec` is the guard record (layout: hrviton_hip.h, hrv_grad_guard_finalize).  apply == 0 -> the whole grid returns
// without touching w, m or v (one wave-uniform word); otherwise gi = (g[i] * gscale) * scale, so that scale == 1.0f gives the
// bits of the plain kernel.
// ``first`` / ``stride``: the thread's first element and the grid's thread count, formed IN THE KERNEL (the compiler folds
// blockDim against the launch bounds only in a kernel's own body: formed here, the plain kernels would gain a load).
#pragma once
#include "hrv_common.h"

namespace hrv {

template <bool GUARD>
__device__ __forceinline__ void adam_update(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, size_t n, size_t first, size_t stride, float lr, float b1, float b2, float eps, float wd,
                                            float bc1, float bc2_sqrt, float gscale, const int32_t* __restrict__ rec) {
  float scale = 1.f;
  if constexpr (GUARD) {
    if (rec[HRV_GUARD_APPLY] == 0) return;
    scale = __builtin_bit_cast(float, rec[HRV_GUARD_SCALE]);
  }
  for (size_t i = first; i < n; i += stride) {
    float gi = g[i] * gscale;
    if constexpr (GUARD) gi *= scale;
    const float wi = w[i];
    if (wd != 0.f) gi += wd * wi;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    w[i] = wi - (lr / bc1) * (mi / denom);
  }
}

// grid of the flat-buffer kernels: 256-thread blocks, at most 4096 of them, grid-stride over the rest
static inline int adam_grid(size_t n) {
  const size_t g = (n + 255) / 256, cap = 256 * 16;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace hrv
