// Adam step that also keeps an exponential moving average of the weights (ABI and contract: include/hrviton_hip.h), and the
// in-place exchange of two flat buffers that serves evaluation with the averaged weights.
//   w', m', v' : adam_elem of adam_body.h, the arithmetic of the plain / guarded kernels: the same bits
//   d   = warmup ? fminf(decay, (1 + t) / (10 + t)) : decay      t = the step count of this launch, as float
//   omd = 1.f - d
//   e'  = omd == 1.f ? w' : fmaf(omd, w' - e, e)
// d and omd are formed by every thread from launch arguments (or from the device step count): wave-uniform, no extra launch.
// A guarded launch with apply == 0 returns before it touches anything, e included.
// Geometry: 256-thread blocks, at most EMA_CAP of them (8 per CU of a 256-CU part: all resident at once), grid-stride.  With all
// pointers on 16-byte boundaries a thread moves one 16-byte group of each array per trip (EMA_CAP * 256 * 4 elements per pass of
// the grid) and threads 0 .. n % 4 - 1 of the grid take the tail; otherwise (VEC = false, chosen on the host from the pointers)
// the whole launch moves 4 bytes per thread and trip.
#include "adam_body.h"
#include "hrv_common.h"

namespace hrv {

constexpr int EMA_BLOCK = 256;
constexpr int EMA_CAP = 2048;

struct alignas(16) quad {
  float x[4];
};

static inline int ema_grid(size_t n, bool vec) {
  const size_t work = vec ? n / 4 : n, g = (work + EMA_BLOCK - 1) / EMA_BLOCK;
  return (int)(g < 1 ? 1 : (g > (size_t)EMA_CAP ? (size_t)EMA_CAP : g));
}

static inline bool aligned16(const void* a, const void* b, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 15) == 0;
}

__device__ __forceinline__ float ema_elem(float wn, float e, float omd) { return omd == 1.f ? wn : __builtin_fmaf(omd, wn - e, e); }

// DEV: lr and the bias corrections come from hyper[3], the step count from step_dev[0] (already advanced for this step)
template <bool GUARD, bool DEV, bool VEC>
__global__ __launch_bounds__(EMA_BLOCK) void adam_ema_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ v, float* __restrict__ ema, size_t n, float lr, float b1,
                                                             float b2, float eps, float wd, float bc1, float bc2_sqrt, float gscale,
                                                             const float* __restrict__ hyper, const int32_t* __restrict__ rec, float decay,
                                                             int warmup, int step, const int32_t* __restrict__ step_dev) {
  float scale = 1.f;
  if constexpr (GUARD) {
    if (rec[HRV_GUARD_APPLY] == 0) return;
    scale = __builtin_bit_cast(float, rec[HRV_GUARD_SCALE]);
  }
  if constexpr (DEV) {
    lr = hyper[0];
    bc1 = hyper[1];
    bc2_sqrt = hyper[2];
    step = step_dev[0];
  }
  const float t = (float)step;
  const float d = warmup ? fminf(decay, (1.f + t) / (10.f + t)) : decay;
  const float omd = 1.f - d;
  const size_t first = (size_t)blockIdx.x * EMA_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * EMA_BLOCK;
  if constexpr (VEC) {
    const size_t n4 = n / 4;
    for (size_t i = first; i < n4; i += stride) {
      quad w4 = reinterpret_cast<const quad*>(w)[i], m4 = reinterpret_cast<const quad*>(m)[i], v4 = reinterpret_cast<const quad*>(v)[i];
      const quad g4 = reinterpret_cast<const quad*>(g)[i];
      quad e4 = reinterpret_cast<const quad*>(ema)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float wn = adam_elem<GUARD>(w4.x, g4.x, m4.x, v4.x, k, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, scale);
        e4.x[k] = ema_elem(wn, e4.x[k], omd);
      }
      reinterpret_cast<quad*>(m)[i] = m4;
      reinterpret_cast<quad*>(v)[i] = v4;
      reinterpret_cast<quad*>(w)[i] = w4;
      reinterpret_cast<quad*>(ema)[i] = e4;
    }
    const size_t i = 4 * n4 + first;
    if (i < n) ema[i] = ema_elem(adam_elem<GUARD>(w, g, m, v, i, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, scale), ema[i], omd);
  } else {
    for (size_t i = first; i < n; i += stride)
      ema[i] = ema_elem(adam_elem<GUARD>(w, g, m, v, i, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, scale), ema[i], omd);
  }
}

template <bool VEC>
__global__ __launch_bounds__(EMA_BLOCK) void swap_kernel(float* __restrict__ a, float* __restrict__ b, size_t n) {
  const size_t first = (size_t)blockIdx.x * EMA_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * EMA_BLOCK;
  if constexpr (VEC) {
    const size_t n4 = n / 4;
    for (size_t i = first; i < n4; i += stride) {
      const quad x = reinterpret_cast<const quad*>(a)[i], y = reinterpret_cast<const quad*>(b)[i];
      reinterpret_cast<quad*>(a)[i] = y;
      reinterpret_cast<quad*>(b)[i] = x;
    }
    const size_t i = 4 * n4 + first;
    if (i < n) {
      const float x = a[i];
      a[i] = b[i];
      b[i] = x;
    }
  } else {
    for (size_t i = first; i < n; i += stride) {
      const float x = a[i];
      a[i] = b[i];
      b[i] = x;
    }
  }
}

template <bool GUARD, bool DEV>
static int launch_adam_ema(const char* what, float* w, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float b1,
                           float b2, float eps, float wd, int32_t step, float gscale, const float* hyper, const int32_t* rec, float decay,
                           int32_t warmup, const int32_t* step_dev, hrv_stream_t stream) {
  HRV_REQUIRE(w && g && m && v && ema && n > 0 && (((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 3) == 0,
              "%s: bad args (null pointer, n <= 0 or misaligned)", what);
  HRV_REQUIRE(decay >= 0.f && decay < 1.f, "%s: decay must lie in [0, 1), got %g", what, (double)decay);
  HRV_REQUIRE(!GUARD || rec, "%s: null guard record", what);
  HRV_REQUIRE(DEV ? (hyper && step_dev) : step >= 1, "%s: bad step count (host: step >= 1; device: hyper_dev and step_dev)", what);
  float bc1 = 0.f, bc2s = 0.f;
  if (!DEV) {
    bc1 = 1.f - powf(b1, (float)step);
    bc2s = sqrtf(1.f - powf(b2, (float)step));
  }
  const bool vec = aligned16(w, g, m, v, ema);
  const dim3 grid(ema_grid((size_t)n, vec)), block(EMA_BLOCK);
  if (vec)
    hipLaunchKernelGGL((adam_ema_kernel<GUARD, DEV, true>), grid, block, 0, (hipStream_t)stream, w, g, m, v, ema, (size_t)n, lr, b1, b2, eps,
                       wd, bc1, bc2s, gscale, hyper, rec, decay, (int)warmup, (int)step, step_dev);
  else
    hipLaunchKernelGGL((adam_ema_kernel<GUARD, DEV, false>), grid, block, 0, (hipStream_t)stream, w, g, m, v, ema, (size_t)n, lr, b1, b2, eps,
                       wd, bc1, bc2s, gscale, hyper, rec, decay, (int)warmup, (int)step, step_dev);
  return check_launch(what);
}

}  // namespace hrv

using namespace hrv;

extern "C" int hrv_adam_ema_f32(float* w, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1, float beta2,
                                float eps, float weight_decay, int32_t step, float grad_scale, float decay, int32_t warmup,
                                hrv_stream_t stream) {
  return launch_adam_ema<false, false>("adam_ema", w, g, m, v, ema, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, nullptr, nullptr,
                                       decay, warmup, nullptr, stream);
}

extern "C" int hrv_adam_dev_ema_f32(float* w, const float* g, float* m, float* v, float* ema, int64_t n, const float* hyper_dev, float beta1,
                                    float beta2, float eps, float weight_decay, float grad_scale, float decay, int32_t warmup,
                                    const int32_t* step_dev, hrv_stream_t stream) {
  return launch_adam_ema<false, true>("adam_dev_ema", w, g, m, v, ema, n, 0.f, beta1, beta2, eps, weight_decay, 0, grad_scale, hyper_dev, nullptr,
                                      decay, warmup, step_dev, stream);
}

extern "C" int hrv_adam_guarded_ema_f32(float* w, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1,
                                        float beta2, float eps, float weight_decay, int32_t step, float grad_scale, const int32_t* record,
                                        float decay, int32_t warmup, hrv_stream_t stream) {
  return launch_adam_ema<true, false>("adam_guarded_ema", w, g, m, v, ema, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, nullptr,
                                      record, decay, warmup, nullptr, stream);
}

extern "C" int hrv_adam_dev_guarded_ema_f32(float* w, const float* g, float* m, float* v, float* ema, int64_t n, const float* hyper_dev,
                                            float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                            const int32_t* record, float decay, int32_t warmup, const int32_t* step_dev,
                                            hrv_stream_t stream) {
  return launch_adam_ema<true, true>("adam_dev_guarded_ema", w, g, m, v, ema, n, 0.f, beta1, beta2, eps, weight_decay, 0, grad_scale, hyper_dev,
                                     record, decay, warmup, step_dev, stream);
}

extern "C" int hrv_swap_f32(float* a, float* b, int64_t n, hrv_stream_t stream) {
  HRV_REQUIRE(a && b && n > 0 && (((uintptr_t)a | (uintptr_t)b) & 3) == 0, "swap: bad args (null pointer, n <= 0 or misaligned)");
  const size_t lo = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)a : (uintptr_t)b, hi = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)b : (uintptr_t)a;
  HRV_REQUIRE(hi - lo >= 4 * (size_t)n, "swap: the two buffers overlap");
  const bool vec = aligned16(a, b);
  const dim3 grid(ema_grid((size_t)n, vec)), block(EMA_BLOCK);
  if (vec)
    hipLaunchKernelGGL(swap_kernel<true>, grid, block, 0, (hipStream_t)stream, a, b, (size_t)n);
  else
    hipLaunchKernelGGL(swap_kernel<false>, grid, block, 0, (hipStream_t)stream, a, b, (size_t)n);
  return check_launch("swap_kernel");
}
