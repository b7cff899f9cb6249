// Guarded Adam step (ABI and record layout: include/hrviton_hip.h).  Three pieces, all consumed on the device so that the
// decision costs no host synchronisation and lives inside a hipGraph-captured iteration:
//   grad_sumsq_kernel    one streaming pass over the flat gradient buffer -> GUARD_SLOTS (sum of squares, non-finite count) partials
//   grad_finalize_kernel one block: partials -> guard record {norm, scale, apply, counts}; optionally the device step count / hyper
//   adam_*_guarded       the Adam update of adam_body.h reading the record
// Determinism: the slot count is a compile-time constant (never the CU count), block b IS slot b, the element -> thread rule
// depends only on (pointer alignment, n), and every sum has a fixed order: per thread over its trips in turn (then its head and
// tail element, block 0 only), a 64-lane shuffle tree, the four waves through LDS in wave order, the slots in a fixed tree.
// No atomics.  Squares are taken in fp64 (an element of 1e30 has a finite norm; fp32 squares would overflow).
#include "adam_body.h"
#include "hrv_common.h"

namespace hrv {

constexpr int GUARD_SLOTS = 1024;      // P: blocks of the partial pass = slots of the workspace
constexpr int GUARD_BLOCK = 256;

__device__ __forceinline__ void guard_acc(float x, double& s, int& c) {
  const double d = (double)x;
  s += d * d;
  c += (__builtin_bit_cast(unsigned, x) & 0x7f800000u) == 0x7f800000u;
}
__device__ __forceinline__ void guard_acc4(f32x4 x, double& s, int& c) {
#pragma unroll
  for (int e = 0; e < 4; ++e) guard_acc(x[e], s, c);
}

// (s, c) of the 256 threads -> thread 0, fixed order: shuffle tree inside each wave, then waves 0..3 in turn
__device__ __forceinline__ void guard_block_reduce(double& s, int& c) {
  __shared__ double red_s[GUARD_BLOCK / 64];
  __shared__ int red_c[GUARD_BLOCK / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_down(s, o, 64);
    c += __shfl_down(c, o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red_s[wave] = s;
    red_c[wave] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s = red_s[0];
    c = red_c[0];
#pragma unroll
    for (int k = 1; k < GUARD_BLOCK / 64; ++k) {
      s += red_s[k];
      c += red_c[k];
    }
  }
}

// g[0, head) scalar | n4 float4 groups from the first 16-byte boundary | the scalar tail up to n.  Group i belongs to thread
// i mod (GUARD_SLOTS * 256) of the grid; head and tail elements (at most 3 each) to threads 0..2 of block 0.
__global__ __launch_bounds__(GUARD_BLOCK) void grad_sumsq_kernel(const float* __restrict__ g, size_t n, size_t head, size_t n4,
                                                                double* __restrict__ part, int32_t* __restrict__ cnt) {
  const f32x4* __restrict__ body = reinterpret_cast<const f32x4*>(g + head);
  const size_t stride = (size_t)GUARD_SLOTS * GUARD_BLOCK;
  double s = 0.0;
  int c = 0;
  // one 16-byte load per thread and trip, 4 MiB of the buffer per pass of the grid.  Measured on the generator's 402 MB buffer:
  // unrolling the trips (2 / 4 / 8 loads in flight per thread, 4 MiB apart) LOSES bandwidth, 5.9 -> 5.9 / 5.5 / 4.9 TB/s, and 512- or
  // 1024-thread blocks change nothing: the plain loop is at the read rate of the part
  for (size_t i = (size_t)blockIdx.x * GUARD_BLOCK + threadIdx.x; i < n4; i += stride) guard_acc4(body[i], s, c);
  if (blockIdx.x == 0) {
    const size_t t = threadIdx.x, tail0 = head + 4 * n4;
    if (t < head) guard_acc(g[t], s, c);
    if (tail0 + t < n) guard_acc(g[tail0 + t], s, c);
  }
  guard_block_reduce(s, c);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = s;
    cnt[blockIdx.x] = c;
  }
}

template <bool HYPER>
__global__ __launch_bounds__(GUARD_BLOCK) void grad_finalize_kernel(const double* __restrict__ part, const int32_t* __restrict__ cnt,
                                                                   float gscale, float max_norm, int skip_nonfinite,
                                                                   int32_t* __restrict__ rec, int32_t* __restrict__ step,
                                                                   const float* __restrict__ lr, float b1, float b2,
                                                                   float* __restrict__ hyper) {
  double s = 0.0;
  int c = 0;
  for (int k = threadIdx.x; k < GUARD_SLOTS; k += GUARD_BLOCK) {
    s += part[k];
    c += cnt[k];
  }
  guard_block_reduce(s, c);
  if (threadIdx.x != 0) return;
  const float norm = (float)((double)gscale * sqrt(s));
  float scale = 1.f;
  if (max_norm > 0.f) {
    const float coef = max_norm / (norm + 1e-6f);
    scale = coef < 1.f ? coef : (coef != coef ? coef : 1.f);      // clamp(max = 1) that keeps a NaN, as torch's does
  }
  const bool finite = (__builtin_bit_cast(unsigned, norm) & 0x7f800000u) != 0x7f800000u;
  const int apply = (skip_nonfinite && (c != 0 || !finite)) ? 0 : 1;
  rec[HRV_GUARD_NORM] = __builtin_bit_cast(int32_t, norm);
  rec[HRV_GUARD_SCALE] = __builtin_bit_cast(int32_t, scale);
  rec[HRV_GUARD_APPLY] = apply;
  rec[HRV_GUARD_NONFINITE] = c;
  rec[HRV_GUARD_STEPS] += 1;
  rec[HRV_GUARD_SKIPPED] += apply ? 0 : 1;
  rec[HRV_GUARD_CLIPPED] += (apply && scale < 1.f) ? 1 : 0;
  *reinterpret_cast<double*>(rec + HRV_GUARD_SUMSQ) = s;
  if constexpr (HYPER) {
    if (apply) {      // adam_hyper_kernel (train.hip), for applied steps only
      const int t = step[0] + 1;
      step[0] = t;
      hyper[0] = lr[0];
      hyper[1] = 1.f - powf(b1, (float)t);
      hyper[2] = sqrtf(1.f - powf(b2, (float)t));
    }
  }
}

__global__ void adam_guarded_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                    float* __restrict__ v, size_t n, float lr, float b1, float b2, float eps, float wd, float bc1,
                                    float bc2_sqrt, float gscale, const int32_t* __restrict__ rec) {
  adam_update<true>(w, g, m, v, n, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, rec);
}

__global__ void adam_dev_guarded_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                        float* __restrict__ v, size_t n, const float* __restrict__ hyper, float b1, float b2,
                                        float eps, float wd, float gscale, const int32_t* __restrict__ rec) {
  // (hyper holds zeros if every step so far was skipped: adam_update returns on apply == 0 before it uses them)
  const float lr = hyper[0], bc1 = hyper[1], bc2_sqrt = hyper[2];
  adam_update<true>(w, g, m, v, n, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, rec);
}

}  // namespace hrv

using namespace hrv;

extern "C" int hrv_grad_guard_slots(void) { return GUARD_SLOTS; }

extern "C" int hrv_grad_sumsq_f32(const float* g, int64_t n, double* part, int32_t* cnt, hrv_stream_t stream) {
  HRV_REQUIRE(g && part && cnt && n > 0 && ((uintptr_t)g & 3) == 0 && ((uintptr_t)part & 7) == 0 && ((uintptr_t)cnt & 3) == 0,
              "grad_sumsq: bad args (null pointer, n <= 0 or misaligned)");
  size_t head = ((16 - ((uintptr_t)g & 15)) & 15) / 4;
  if (head > (size_t)n) head = (size_t)n;
  const size_t n4 = ((size_t)n - head) / 4;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(GUARD_SLOTS), dim3(GUARD_BLOCK), 0, (hipStream_t)stream, g, (size_t)n, head, n4, part,
                     cnt);
  return check_launch("grad_sumsq_kernel");
}

extern "C" int hrv_grad_guard_finalize(const double* part, const int32_t* cnt, float grad_scale, float max_norm,
                                       int32_t skip_nonfinite, int32_t* record, hrv_stream_t stream) {
  HRV_REQUIRE(part && cnt && record && ((uintptr_t)record & 7) == 0, "grad_guard_finalize: bad args");
  hipLaunchKernelGGL((grad_finalize_kernel<false>), dim3(1), dim3(GUARD_BLOCK), 0, (hipStream_t)stream, part, cnt, grad_scale, max_norm,
                     (int)skip_nonfinite, record, (int32_t*)nullptr, (const float*)nullptr, 0.f, 0.f, (float*)nullptr);
  return check_launch("grad_finalize_kernel");
}

extern "C" int hrv_grad_guard_finalize_hyper(const double* part, const int32_t* cnt, float grad_scale, float max_norm,
                                             int32_t skip_nonfinite, int32_t* record, int32_t* step_dev, const float* lr_dev,
                                             float beta1, float beta2, float* hyper_dev, hrv_stream_t stream) {
  HRV_REQUIRE(part && cnt && record && ((uintptr_t)record & 7) == 0 && step_dev && lr_dev && hyper_dev,
              "grad_guard_finalize_hyper: bad args");
  hipLaunchKernelGGL((grad_finalize_kernel<true>), dim3(1), dim3(GUARD_BLOCK), 0, (hipStream_t)stream, part, cnt, grad_scale, max_norm,
                     (int)skip_nonfinite, record, step_dev, lr_dev, beta1, beta2, hyper_dev);
  return check_launch("grad_finalize_kernel[hyper]");
}

extern "C" int hrv_adam_guarded_f32(float* w, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                                    float eps, float weight_decay, int32_t step, float grad_scale, const int32_t* record,
                                    hrv_stream_t stream) {
  HRV_REQUIRE(w && g && m && v && record && n > 0 && step >= 1, "adam_guarded: bad args");
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.f - powf(beta2, (float)step));
  hipLaunchKernelGGL(adam_guarded_kernel, dim3(adam_grid((size_t)n)), dim3(256), 0, (hipStream_t)stream, w, g, m, v, (size_t)n, lr,
                     beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale, record);
  return check_launch("adam_guarded_kernel");
}

extern "C" int hrv_adam_dev_guarded_f32(float* w, const float* g, float* m, float* v, int64_t n, const float* hyper_dev, float beta1,
                                        float beta2, float eps, float weight_decay, float grad_scale, const int32_t* record,
                                        hrv_stream_t stream) {
  HRV_REQUIRE(w && g && m && v && hyper_dev && record && n > 0, "adam_dev_guarded: bad args");
  hipLaunchKernelGGL(adam_dev_guarded_kernel, dim3(adam_grid((size_t)n)), dim3(256), 0, (hipStream_t)stream, w, g, m, v, (size_t)n,
                     hyper_dev, beta1, beta2, eps, weight_decay, grad_scale, record);
  return check_launch("adam_dev_guarded_kernel");
}
