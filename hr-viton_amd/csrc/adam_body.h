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

// One element of the update, shared by adam_update and the averaging kernels (adam_ema.hip) so that both produce the same bits.
// It reads and writes element i of the four arrays (global memory here, a thread's registers there) with the statements, in the
// order, adam_update always had: the plain kernels' code is what it was.  Returns the new weight.  ``scale`` is read with GUARD only.
// Which products fuse with the sum behind them is pinned here, to what the compiler chose for the scalar loop (every product
// and sum of g, m, v and denom rounded on its own; the weight one fused multiply-add): left to the optimizer, the four-element
// body of the averaging kernels fuses others, and its moments differ from the plain kernel's in the last bit.
template <bool GUARD>
__device__ __forceinline__ float adam_elem(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                           float* __restrict__ v, size_t i, float lr, float b1, float b2, float eps, float wd, float bc1,
                                           float bc2_sqrt, float gscale, float scale) {
  float wi, mi, denom;
  {
#pragma clang fp contract(off)
    float gi = g[i] * gscale;
    if constexpr (GUARD) gi *= scale;
    wi = w[i];
    if (wd != 0.f) gi += wd * wi;
    mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    denom = sqrtf(vi) / bc2_sqrt + eps;
  }
  const float wn = wi - (lr / bc1) * (mi / denom);      // (one product under one sum: it fuses in every instance)
  w[i] = wn;
  return wn;
}

template <bool GUARD>
__device__ __forceinline__ void adam_update(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, size_t n, size_t first, size_t stride, float lr, float b1, float b2, float eps, float wd,
                                            float bc1, float bc2_sqrt, float gscale, const int32_t* __restrict__ rec) {
  float scale = 1.f;
  if constexpr (GUARD) {
    if (rec[HRV_GUARD_APPLY] == 0) return;
    scale = __builtin_bit_cast(float, rec[HRV_GUARD_SCALE]);
  }
  for (size_t i = first; i < n; i += stride) adam_elem<GUARD>(w, g, m, v, i, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, scale);
}

// grid of the flat-buffer kernels: 256-thread blocks, at most 4096 of them, grid-stride over the rest
static inline int adam_grid(size_t n) {
  const size_t g = (n + 255) / 256, cap = 256 * 16;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace hrv
