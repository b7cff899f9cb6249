// Training-side HBM-bound kernels (NHWC fp32): loss reductions with their gradients,
// 2x2 gradient down-sum (nearest-upsample backward), avg-pool backward, 2x2 max-pool
// forward/backward (VGG19), fused Adam, and the GEMVs of the spectral-norm power
// iteration.  All reductions are two-stage with a fixed summation order (deterministic).
// (The InstanceNorm / SPADE backward is norm_bwd.hip.)
#include <string.h>

#include "adam_body.h"
#include "hrv_common.h"

namespace hrv {

static inline int grid_for(size_t work, int block = 256) {
  size_t g = (work + block - 1) / block;
  const size_t cap = 256 * 16;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ---------------------------------------------------------------------------
// losses: value + gradient in one pass.  mode: 0 L1 |a-b| ; 1 hinge-D fake max(1+a,0) ;
// 2 hinge-D real max(1-a,0) ; 3 -a (generator hinge / wgan) ; 4 (a-b)^2 (LSGAN/MSE)
// grad[i] = gscale * dl/da ; loss = lscale * sum(l)   (callers pass 1/numel etc.)
// ---------------------------------------------------------------------------
template <bool AB>
__global__ __launch_bounds__(256) void loss_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n,
                                                   int mode_flags, float gscale, float* __restrict__ grad,
                                                   float* __restrict__ part, int vec) {
  __shared__ float red[256];
  float s = 0.f;
  const int mode = mode_flags & 15;
  const bool relu_mask = (mode_flags & 16) != 0;   // a = ReLU(pre): the gradient is handed back w.r.t. pre (x (a > 0))
  const bool grad_bf16 = (mode_flags & 32) != 0;   // the gradient is stored as bf16 (its readers: matrix cores, pool backward)
  auto term = [&](float x, float y, float& g) -> float {
    float l;
    if (mode == 0) { const float d = x - y; l = fabsf(d); g = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
    else if (mode == 1) { l = fmaxf(1.f + x, 0.f); g = x > -1.f ? 1.f : 0.f; }
    else if (mode == 2) { l = fmaxf(1.f - x, 0.f); g = x < 1.f ? -1.f : 0.f; }
    else if (mode == 3) { l = -x; g = -1.f; }
    else { const float d = x - y; l = d * d; g = 2.f * d; }
    g = (relu_mask && !(x > 0.f)) ? 0.f : gscale * g;
    return l;
  };
  typedef unsigned short u16x4v __attribute__((ext_vector_type(4)));
  auto ld4v = [](const float* p, size_t k) -> f32x4 {      // 4 consecutive elements starting at element k
    if constexpr (AB) {
      const u16x4v h = *reinterpret_cast<const u16x4v*>(reinterpret_cast<const unsigned short*>(p) + k);
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = __builtin_bit_cast(float, (unsigned)h[e] << 16);
      return v;
    } else {
      return *reinterpret_cast<const f32x4*>(p + k);
    }
  };
  // 16-byte (fp32) / 8-byte (bf16) accesses: four consecutive elements per thread and iteration
  const size_t n4 = vec ? n / 4 : 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4 x4 = ld4v(a, 4 * i);
    const f32x4 y4 = b ? ld4v(b, 4 * i) : (f32x4)(0.f);
    f32x4 g4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float g;
      s += term(x4[e], y4[e], g);
      g4[e] = g;
    }
    if (grad) {
      if (grad_bf16) st4_bf16(grad, 4 * i, g4);
      else *reinterpret_cast<f32x4*>(grad + 4 * i) = g4;
    }
  }
  for (size_t i = 4 * n4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float x, y = 0.f, g;
    if constexpr (AB) {
      x = __builtin_bit_cast(float, (unsigned)reinterpret_cast<const unsigned short*>(a)[i] << 16);
      if (b) y = __builtin_bit_cast(float, (unsigned)reinterpret_cast<const unsigned short*>(b)[i] << 16);
    } else {
      x = a[i];
      if (b) y = b[i];
    }
    s += term(x, y, g);
    if (grad) {
      if (grad_bf16) reinterpret_cast<unsigned short*>(grad)[i] = (unsigned short)(__builtin_bit_cast(unsigned, __builtin_bit_cast(unsigned, g) + 0x7fffu + ((__builtin_bit_cast(unsigned, g) >> 16) & 1u)) >> 16);
      else grad[i] = g;
    }
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// one wave: lane l sums part[l], part[l + 64], ... in double, then a fixed butterfly (deterministic).  (One thread walking
// up to 1024 partials took 25 us; 44 of these per training step.)
__global__ void loss_final_kernel(const float* __restrict__ part, int nb, float lscale, float* __restrict__ out,
                                  int accumulate) {
  if (blockIdx.x != 0 || threadIdx.x >= 64) return;
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 64) s += (double)part[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if (threadIdx.x == 0) {
    const float v = (float)(s * (double)lscale);
    out[0] = accumulate ? out[0] + v : v;
  }
}

// x *= s_host * (s_dev ? s_dev[0] : 1)   (upstream loss-gradient scalar without a host sync)
__global__ void scale_kernel(float* __restrict__ x, size_t n, float s_host, const float* __restrict__ s_dev) {
  const float s = s_dev ? s_host * s_dev[0] : s_host;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) x[i] *= s;
}

// out = dy * (1 - y*y)   (tanh backward through its output)   /   out (+)= a  (gradient accumulation)
__global__ void tanh_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, size_t n, float* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float t = y[i];
    out[i] = dy[i] * (1.f - t * t);
  }
}

// d <- d * act'(y)  in place (activation derivative through the activation's output)
__global__ void act_bwd_kernel(float* __restrict__ d, int dcs, int dco, const float* __restrict__ y, int ycs, int yco, int C4,
                               size_t npix, int act, float slope) {
  const size_t total = npix * C4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int g = (int)(i % C4);
    const size_t pix = i / C4;
    float* o = d + pix * dcs + dco + g * 4;
    f32x4 v = ld4(o);
    const f32x4 yy = ld4(y + pix * ycs + yco + g * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] *= dact(yy[e], act, slope);
    *reinterpret_cast<f32x4*>(o) = v;
  }
}

__global__ void add_slice_kernel(const float* __restrict__ a, int acs, int aco, float* __restrict__ out, int ocs, int oco,
                                 int C4, size_t npix, int accumulate) {
  const size_t total = npix * C4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int g = (int)(i % C4);
    const size_t pix = i / C4;
    f32x4 v = ld4(a + pix * acs + aco + g * 4);
    float* o = out + pix * ocs + oco + g * 4;
    if (accumulate) v += ld4(o);
    *reinterpret_cast<f32x4*>(o) = v;
  }
}

// ---------------------------------------------------------------------------
// nearest-x2 upsample backward: dlo[n,h,w,c] = sum of the 2x2 block of dhi
// ---------------------------------------------------------------------------
__global__ void downsum2x2_kernel(const float* __restrict__ dhi, int N, int Hl, int Wl, int C4, int hcs, int hco,
                                  float* __restrict__ dlo, int lcs, int lco, int accumulate) {
  const size_t total = (size_t)N * Hl * Wl * C4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int g = (int)(i % C4);
    const size_t pix = i / C4;
    const int w = (int)(pix % Wl);
    const size_t t = pix / Wl;
    const int h = (int)(t % Hl);
    const int n = (int)(t / Hl);
    const float* s = dhi + (((size_t)n * 2 * Hl + 2 * h) * 2 * Wl + 2 * w) * hcs + hco + g * 4;
    f32x4 v = ld4(s) + ld4(s + hcs) + ld4(s + (size_t)2 * Wl * hcs) + ld4(s + (size_t)2 * Wl * hcs + hcs);
    if (accumulate == 2) {      // bf16 result (element strides): a gradient only matrix cores read
      st4_bf16(dlo, pix * lcs + lco + g * 4, v);
      continue;
    }
    float* o = dlo + pix * lcs + lco + g * 4;
    if (accumulate) v += ld4(o);
    *reinterpret_cast<f32x4*>(o) = v;
  }
}

// avg_pool2d(3, s2, p1, count_include_pad=False) backward: dx[h,w] = sum over the (<= 4) windows that
// contain (h,w) of dy[ho,wo] / count(ho,wo)
__global__ void avgpool3s2_bwd_kernel(const float* __restrict__ dy, int N, int H, int W, int C4, int Ho, int Wo,
                                      int ycs, int yco, float* __restrict__ dx, int xcs, int xco, int accumulate) {
  const size_t total = (size_t)N * H * W * C4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int g = (int)(i % C4);
    const size_t pix = i / C4;
    const int w = (int)(pix % W);
    const size_t t = pix / W;
    const int h = (int)(t % H);
    const int n = (int)(t / H);
    f32x4 s = (f32x4)(0.f);
    for (int ho = h / 2; ho <= (h + 1) / 2; ++ho) {
      if (ho >= Ho) continue;
      const int ch = min(2 * ho + 1, H - 1) - max(2 * ho - 1, 0) + 1;
      for (int wo = w / 2; wo <= (w + 1) / 2; ++wo) {
        if (wo >= Wo) continue;
        const int cw = min(2 * wo + 1, W - 1) - max(2 * wo - 1, 0) + 1;
        s += ld4(dy + ((size_t)(n * Ho + ho) * Wo + wo) * ycs + yco + g * 4) / (float)(ch * cw);
      }
    }
    float* o = dx + pix * xcs + xco + g * 4;
    if (accumulate) s += ld4(o);
    *reinterpret_cast<f32x4*>(o) = s;
  }
}

// ---------------------------------------------------------------------------
// VGG19: 2x2 stride-2 max pool, forward and backward (first maximum in (0,0),(0,1),(1,0),(1,1)
// scan order takes the gradient, like torch)
// ---------------------------------------------------------------------------
// XB: x (and y) are bf16-stored (mixed-precision VGG activations: matrix cores, pools and the L1 taps are the only readers)
template <bool XB>
__device__ __forceinline__ f32x4 ldg4(const float* base, size_t idx) {
  if constexpr (XB) {
    // loaded as a vector of the STORED element type: reading the bf16 data through uint2 / f32x2 lvalues here came out of the
    // compiler as one dword load with every lane a copy of element 0 (type-punned access)
    typedef unsigned short u16x4v __attribute__((ext_vector_type(4)));
    const u16x4v h = *reinterpret_cast<const u16x4v*>(reinterpret_cast<const unsigned short*>(base) + idx);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = __builtin_bit_cast(float, (unsigned)h[e] << 16);
    return v;
  } else {
    return ld4(base + idx);
  }
}

template <bool XB>
__global__ void maxpool2_kernel(const float* __restrict__ x, int N, int Ho, int Wo, int C4, int xcs, float* __restrict__ y,
                                int ycs) {
  const size_t total = (size_t)N * Ho * Wo * C4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int g = (int)(i % C4);
    const size_t pix = i / C4;
    const int wo = (int)(pix % Wo);
    const size_t t = pix / Wo;
    const int ho = (int)(t % Ho);
    const int n = (int)(t / Ho);
    const size_t s = (((size_t)n * 2 * Ho + 2 * ho) * 2 * Wo + 2 * wo) * xcs + g * 4;
    if constexpr (XB) {
      // bf16 storage: the inputs are ReLU outputs (>= 0, never NaN), for which the order of the 16-bit patterns read as SIGNED
      // integers IS the order of the values (-0 = 0x8000 = -32768 sorts below every +x: a ReLU written as max(v, v * 0) stores
      // -0 for v < 0) -- an integer max on the stored elements, exact, no conversion
      typedef short u16x4v __attribute__((ext_vector_type(4)));
      const unsigned short* xs = reinterpret_cast<const unsigned short*>(x);
      const u16x4v a = *reinterpret_cast<const u16x4v*>(xs + s), b = *reinterpret_cast<const u16x4v*>(xs + s + xcs),
                   c = *reinterpret_cast<const u16x4v*>(xs + s + (size_t)2 * Wo * xcs),
                   d = *reinterpret_cast<const u16x4v*>(xs + s + (size_t)2 * Wo * xcs + xcs);
      u16x4v o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const short p = a[e] > b[e] ? a[e] : b[e], q = c[e] > d[e] ? c[e] : d[e];
        o[e] = p > q ? p : q;
      }
      *reinterpret_cast<u16x4v*>(reinterpret_cast<unsigned short*>(y) + pix * ycs + g * 4) = o;
    } else {
      const f32x4 a = ld4(x + s), b = ld4(x + s + xcs), c = ld4(x + s + (size_t)2 * Wo * xcs), d = ld4(x + s + (size_t)2 * Wo * xcs + xcs);
      f32x4 m;
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = fmaxf(fmaxf(a[e], b[e]), fmaxf(c[e], d[e]));
      *reinterpret_cast<f32x4*>(y + pix * ycs + g * 4) = m;
    }
  }
}

// XB: x is bf16-stored; GB: dy and dx are bf16-stored too (mixed-precision VGG backward: gradients that only matrix cores
// and this routing read)
template <bool XB, bool GB = false>
__global__ void maxpool2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, int N, int Ho, int Wo,
                                    int C4, int xcs, int ycs, float* __restrict__ dx, int relu) {
  const size_t total = (size_t)N * Ho * Wo * C4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int g = (int)(i % C4);
    const size_t pix = i / C4;
    const int wo = (int)(pix % Wo);
    const size_t t = pix / Wo;
    const int ho = (int)(t % Ho);
    const int n = (int)(t / Ho);
    const size_t base = (((size_t)n * 2 * Ho + 2 * ho) * 2 * Wo + 2 * wo) * xcs + g * 4;
    const size_t o01 = xcs, o10 = (size_t)2 * Wo * xcs, o11 = o10 + xcs;
    const f32x4 a = ldg4<XB>(x, base), b = ldg4<XB>(x, base + o01), c = ldg4<XB>(x, base + o10), d = ldg4<XB>(x, base + o11);
    const f32x4 gy = GB ? ld4_bf16(dy, pix * ycs + g * 4) : ld4(dy + pix * ycs + g * 4);
    f32x4 ga = (f32x4)(0.f), gb = ga, gc = ga, gd = ga;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float m = fmaxf(fmaxf(a[e], b[e]), fmaxf(c[e], d[e]));
      const float gv = (relu && !(m > 0.f)) ? 0.f : gy[e];      // relu: x = ReLU(pre), the gradient goes on to pre
      if (a[e] == m) ga[e] = gv;
      else if (b[e] == m) gb[e] = gv;
      else if (c[e] == m) gc[e] = gv;
      else gd[e] = gv;
    }
    if constexpr (GB) {
      st4_bf16(dx, base, ga); st4_bf16(dx, base + o01, gb); st4_bf16(dx, base + o10, gc); st4_bf16(dx, base + o11, gd);
    } else {
      *reinterpret_cast<f32x4*>(dx + base) = ga;
      *reinterpret_cast<f32x4*>(dx + base + o01) = gb;
      *reinterpret_cast<f32x4*>(dx + base + o10) = gc;
      *reinterpret_cast<f32x4*>(dx + base + o11) = gd;
    }
  }
}

// out (+)= a over bf16-stored tensors (fp32 sum, one rounding)
__global__ void add_slice_bf16_kernel(const unsigned short* __restrict__ a, int acs, int aco, unsigned short* __restrict__ out,
                                      int ocs, int oco, int C4, size_t npix, int accumulate) {
  const size_t total = npix * C4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int g = (int)(i % C4);
    const size_t pix = i / C4;
    f32x4 v = ld4_bf16(a, pix * acs + aco + g * 4);
    const size_t oe = pix * ocs + oco + g * 4;
    if (accumulate) v += ld4_bf16(out, oe);
    st4_bf16(out, oe, v);
  }
}

// ---------------------------------------------------------------------------
// Adam (torch.optim.Adam semantics: no amsgrad, optional L2 weight decay), fused over one
// flat buffer.  The update itself is adam_body.h (shared with the guarded kernels of grad_guard.hip).
// ---------------------------------------------------------------------------
__global__ void adam_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, size_t n, float lr, float b1, float b2, float eps, float wd,
                            float bc1, float bc2_sqrt, float gscale) {
  adam_update<false>(w, g, m, v, n, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, nullptr);
}

// The same update with its step-dependent scalars on the DEVICE (hipGraph-capturable training iteration: a replay must not
// freeze the step count or the learning rate into the launch arguments).  adam_hyper_kernel: ++step; hyper = {lr, 1 - b1^t,
// sqrt(1 - b2^t)} (the same expressions the host evaluates for hrv_adam_f32, here with the device's powf / sqrtf).
__global__ void adam_hyper_kernel(int* __restrict__ step, const float* __restrict__ lr, float b1, float b2,
                                  float* __restrict__ hyper) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const int t = step[0] + 1;
    step[0] = t;
    hyper[0] = lr[0];
    hyper[1] = 1.f - powf(b1, (float)t);
    hyper[2] = sqrtf(1.f - powf(b2, (float)t));
  }
}

__global__ void adam_dev_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                float* __restrict__ v, size_t n, const float* __restrict__ hyper, float b1, float b2, float eps,
                                float wd, float gscale) {
  const float lr = hyper[0], bc1 = hyper[1], bc2_sqrt = hyper[2];
  adam_update<false>(w, g, m, v, n, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, nullptr);
}

// ---------------------------------------------------------------------------
// Spectral-norm power iteration GEMVs on W [R][K] (row-major):  y = W x  and  y = W^T x
// (one block per row / per 64-column strip; fixed order => deterministic)
// ---------------------------------------------------------------------------
__device__ __forceinline__ void gemv_rows_body(const float* __restrict__ Wm, const float* __restrict__ x, int K,
                                               float* __restrict__ y, int r) {
  __shared__ float red[256];
  float s = 0.f;
  for (int k = threadIdx.x; k < K; k += 256) s += Wm[(size_t)r * K + k] * x[k];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) y[r] = red[0];
}

__global__ __launch_bounds__(256) void gemv_rows_kernel(const float* __restrict__ Wm, const float* __restrict__ x, int R,
                                                        int K, float* __restrict__ y) {
  gemv_rows_body(Wm, x, K, y, blockIdx.x);
}

__device__ __forceinline__ void gemv_cols_body(const float* __restrict__ Wm, const float* __restrict__ x, int R, int K,
                                               float* __restrict__ y, int blk) {
  // block = 64 columns; 16 row-groups x 16 lanes of 4 columns (16-byte loads when K % 4 == 0), four rows in flight
  // per thread (a 4-row-group version with one scalar load per iteration was pure latency: 51 us per call, 2.8 ms per
  // training step); partial sums are combined in row-group order => deterministic
  __shared__ float red[16][64];
  const int cq = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int c0 = blk * 64 + cq * 4;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if ((K & 3) == 0 && c0 + 3 < K) {
    int r = rg;
    for (; r + 48 < R; r += 64) {
      f32x4 v[4];
      float xr[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        v[u] = *reinterpret_cast<const f32x4*>(Wm + (size_t)(r + 16 * u) * K + c0);
        xr[u] = x[r + 16 * u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += v[u][e] * xr[u];
    }
    for (; r < R; r += 16) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(Wm + (size_t)r * K + c0);
      const float xr = x[r];
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += v[e] * xr;
    }
  } else {
    for (int r = rg; r < R; r += 16) {
      const float xr = x[r];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c0 + e < K) s[e] += Wm[(size_t)r * K + c0 + e] * xr;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[rg][cq * 4 + e] = s[e];
  __syncthreads();
  if (threadIdx.x < 64) {
    const int c = blk * 64 + threadIdx.x;
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) t += red[g][threadIdx.x];
    if (c < K) y[c] = t;
  }
}

__global__ __launch_bounds__(256) void gemv_cols_kernel(const float* __restrict__ Wm, const float* __restrict__ x, int R,
                                                        int K, float* __restrict__ y) {
  gemv_cols_body(Wm, x, R, K, y, blockIdx.x);
}

// ---------------------------------------------------------------------------
// Batched spectral norm: the power iteration of EVERY spectral-normalised convolution of a network in four launches
// (the per-layer sequence above is eight launches of a few microseconds each; the generator has 27 such layers and runs
// twice per training step).  The job table travels in the kernel arguments; a block finds its job by a scan of the
// block-offset prefix (<= SN_MAX entries, wave-uniform).
// ---------------------------------------------------------------------------
constexpr int SN_MAX = 40;
struct SnJob {
  const float* w;
  float *u, *v, *wv, *sigma, *u_keep, *v_keep;
  int R, K;
};
struct SnBatch {
  SnJob job[SN_MAX];
  int col_blk[SN_MAX + 1], row_blk[SN_MAX + 1];
  int n;
  float eps;
};

__device__ __forceinline__ int sn_find(const int* __restrict__ prefix, int n, int b) {
  int j = 0;
  while (j + 1 < n && prefix[j + 1] <= b) ++j;
  return j;
}

__global__ __launch_bounds__(256) void sn_gemv_cols_batched_kernel(const SnBatch B) {   // v' = W^T u
  const int j = sn_find(B.col_blk, B.n, blockIdx.x);
  const SnJob& J = B.job[j];
  gemv_cols_body(J.w, J.u, J.R, J.K, J.v, blockIdx.x - B.col_blk[j]);
}

__global__ __launch_bounds__(256) void sn_gemv_rows_batched_kernel(const SnBatch B) {   // wv = W v
  const int j = sn_find(B.row_blk, B.n, blockIdx.x);
  const SnJob& J = B.job[j];
  gemv_rows_body(J.w, J.v, J.K, J.wv, blockIdx.x - B.row_blk[j]);
}

__device__ __forceinline__ float block_sum256(float s) {
  __shared__ float red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const float t = red[0];
  __syncthreads();
  return t;
}

// one block per job: v <- v / max(||v||, eps), copy kept for the backward
__global__ __launch_bounds__(256) void sn_normalize_v_batched_kernel(const SnBatch B) {
  const SnJob& J = B.job[blockIdx.x];
  float s = 0.f;
  for (int i = threadIdx.x; i < J.K; i += 256) s += J.v[i] * J.v[i];
  const float inv = 1.f / fmaxf(sqrtf(block_sum256(s)), B.eps);
  for (int i = threadIdx.x; i < J.K; i += 256) {
    const float t = J.v[i] * inv;
    J.v[i] = t;
    if (J.v_keep) J.v_keep[i] = t;
  }
}

// one block per job: (iterate) u <- wv / max(||wv||, eps); sigma = u . wv; copies kept for the backward
__global__ __launch_bounds__(256) void sn_finish_batched_kernel(const SnBatch B, int iterate) {
  const SnJob& J = B.job[blockIdx.x];
  if (iterate) {
    float s = 0.f;
    for (int i = threadIdx.x; i < J.R; i += 256) s += J.wv[i] * J.wv[i];
    const float inv = 1.f / fmaxf(sqrtf(block_sum256(s)), B.eps);
    for (int i = threadIdx.x; i < J.R; i += 256) J.u[i] = J.wv[i] * inv;
  }
  float d = 0.f;
  for (int i = threadIdx.x; i < J.R; i += 256) {
    const float ui = J.u[i];            // each thread re-reads the elements it wrote
    d += ui * J.wv[i];
    if (J.u_keep) J.u_keep[i] = ui;
  }
  if (!iterate && J.v_keep)
    for (int i = threadIdx.x; i < J.K; i += 256) J.v_keep[i] = J.v[i];
  d = block_sum256(d);
  if (threadIdx.x == 0) J.sigma[0] = d;
}

// x <- x / max(||x||, eps); also returns ||x|| in out_norm (single block)
__global__ __launch_bounds__(256) void normalize_kernel(float* __restrict__ x, int n, float eps, float* __restrict__ out_norm) {
  __shared__ float red[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += x[i] * x[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const float nrm = sqrtf(red[0]);
  const float inv = 1.f / fmaxf(nrm, eps);
  for (int i = threadIdx.x; i < n; i += 256) x[i] *= inv;
  if (threadIdx.x == 0 && out_norm) out_norm[0] = nrm;
}

// dot(a, b) over n elements -> out[0] (two-stage)
__global__ __launch_bounds__(256) void dot_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          size_t n, float* __restrict__ part) {
  __shared__ float red[256];
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) s += a[i] * b[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// spectral-norm weight-gradient transform (torch SpectralNorm backward with u, v constants):
//   dW_orig[r][k] = (G[r][k] - c * u[r] * v[k]) / sigma,   c = <G, W_orig> / sigma = <G, W_sn>
__global__ void sn_grad_kernel(const float* __restrict__ G, const float* __restrict__ u, const float* __restrict__ v,
                               const float* __restrict__ dotGW, const float* __restrict__ sigma, int R, int K,
                               float* __restrict__ out, int accumulate) {
  const size_t total = (size_t)R * K;
  const float sg = sigma[0];
  const float c = dotGW[0] / sg;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / K), k = (int)(i - (size_t)r * K);
    const float d = (G[i] - c * u[r] * v[k]) / sg;
    out[i] = accumulate ? out[i] + d : d;
  }
}

// ---------------------------------------------------------------------------
// Per-step parameter staging of a SPADE norm / a SPADE block in ONE launch each (they were 5-9 torch fill / index_copy /
// cat launches per norm and forward: ~750 launches of a few microseconds per training step).
// ---------------------------------------------------------------------------
// bias of the fused gamma|beta convolution in its interleaved column order (64g + l: gamma[32g + l] | beta[32g + l - 32])
// and the noise scale padded to the channel stride
__global__ __launch_bounds__(256) void spade_vec_prep_kernel(const float* __restrict__ gb, const float* __restrict__ bb,
                                                             const float* __restrict__ ns, int C, int ncols, int Cp,
                                                             float* __restrict__ bc, float* __restrict__ ns_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < ncols) {
    const int l = i & 63, c = (i >> 6) * 32 + (l & 31);
    bc[i] = c < C ? (l < 32 ? gb[c] : bb[c]) : 0.f;
  }
  if (i < Cp) ns_out[i] = i < C ? ns[i] : 0.f;
}

// ... for every SPADE norm of a network in ONE launch (blockIdx.y = the norm): 58 launches of 4 us per training iteration otherwise
constexpr int VEC_MAXJOBS = 32;
struct VecJobs {
  const float* gb[VEC_MAXJOBS]; const float* bb[VEC_MAXJOBS]; const float* ns[VEC_MAXJOBS];
  int C[VEC_MAXJOBS], off_bc[VEC_MAXJOBS], off_ns[VEC_MAXJOBS];
};
__global__ __launch_bounds__(256) void spade_vec_prep_multi_kernel(const VecJobs j, float* __restrict__ bc_all, float* __restrict__ ns_all) {
  const int q = blockIdx.y, C = j.C[q];
  const int ncols = (C + 31) / 32 * 64, Cp = (C + 3) / 4 * 4;
  float* const bc = bc_all + j.off_bc[q];
  float* const nso = ns_all + j.off_ns[q];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < ncols; i += gridDim.x * 256) {
    const int l = i & 63, c = (i >> 6) * 32 + (l & 31);
    bc[i] = c < C ? (l < 32 ? j.gb[q][c] : j.bb[q][c]) : 0.f;
    if (i < Cp) nso[i] = i < C ? j.ns[q][i] : 0.f;
  }
}

// conv_shared (label_nc -> hid, 3x3) of the n norms of a block as ONE 1x1 weight over the tap-expanded label map
// (ops.tap_expand: tap-major, cp channels per tap): wt[(i*hid + o)][tap*cp + ch] = w_i[o][ch][tap]; bt = concat of biases
struct SharedTaps {
  const float* w[4];
  const float* b[4];
  float* gw[4];
  float* gb[4];
  int n, hid, c, cp;
};
__global__ __launch_bounds__(256) void shared_taps_prep_kernel(const SharedTaps p, float* __restrict__ wt, float* __restrict__ bt) {
  const int K = 9 * p.cp, total = p.n * p.hid * K;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int k = i % K, row = i / K;
    const int tap = k / p.cp, ch = k - tap * p.cp;
    const int j = row / p.hid, o = row - j * p.hid;
    wt[i] = ch < p.c ? p.w[j][((size_t)o * p.c + ch) * 9 + tap] : 0.f;
  }
  for (int i = blockIdx.x * 256 + threadIdx.x; i < p.n * p.hid; i += gridDim.x * 256) bt[i] = p.b[i / p.hid][i % p.hid];
}
// the inverse map for the gradients: gw_i[o][ch][tap] = dw[(i*hid + o)][tap*cp + ch], gb_i = db[i*hid ..]
__global__ __launch_bounds__(256) void shared_taps_grad_kernel(const SharedTaps p, const float* __restrict__ dw,
                                                               const float* __restrict__ db) {
  const int per = p.hid * p.c * 9, total = p.n * per, K = 9 * p.cp;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int j = i / per, r = i - j * per;
    const int tap = r % 9, ch = (r / 9) % p.c, o = r / (9 * p.c);
    p.gw[j][r] = dw[(size_t)(j * p.hid + o) * K + tap * p.cp + ch];
  }
  for (int i = blockIdx.x * 256 + threadIdx.x; i < p.n * p.hid; i += gridDim.x * 256) p.gb[i / p.hid][i % p.hid] = db[i];
}

}  // namespace hrv

using namespace hrv;

extern "C" int hrv_spade_vec_prep_f32(const float* gamma_bias, const float* beta_bias, const float* noise_scale, int32_t C,
                                      float* bias_interleaved, float* noise_scale_padded, hrv_stream_t stream) {
  HRV_REQUIRE(gamma_bias && beta_bias && noise_scale && bias_interleaved && noise_scale_padded && C > 0, "spade_vec_prep: bad args");
  const int ncols = (C + 31) / 32 * 64, Cp = (C + 3) / 4 * 4;
  hipLaunchKernelGGL(spade_vec_prep_kernel, dim3((ncols + 255) / 256), dim3(256), 0, (hipStream_t)stream, gamma_bias, beta_bias,
                     noise_scale, C, ncols, Cp, bias_interleaved, noise_scale_padded);
  return check_launch("spade_vec_prep_kernel");
}

extern "C" int hrv_spade_vec_prep_multi_f32(int32_t n, const float* const* gamma_bias, const float* const* beta_bias,
                                            const float* const* noise_scale, const int32_t* C, const int32_t* off_bias, const int32_t* off_noise,
                                            float* bias_interleaved_all, float* noise_scale_padded_all, hrv_stream_t stream) {
  HRV_REQUIRE(n > 0 && n <= VEC_MAXJOBS && gamma_bias && beta_bias && noise_scale && C && off_bias && off_noise && bias_interleaved_all &&
                  noise_scale_padded_all, "spade_vec_prep_multi: 1 .. %d norms", VEC_MAXJOBS);
  VecJobs j;
  memset(&j, 0, sizeof(j));
  int cmax = 0;
  for (int i = 0; i < n; ++i) {
    HRV_REQUIRE(gamma_bias[i] && beta_bias[i] && noise_scale[i] && C[i] > 0 && off_bias[i] >= 0 && off_noise[i] >= 0 && off_bias[i] % 4 == 0 &&
                    off_noise[i] % 4 == 0, "spade_vec_prep_multi: job %d", i);
    j.gb[i] = gamma_bias[i]; j.bb[i] = beta_bias[i]; j.ns[i] = noise_scale[i];
    j.C[i] = C[i]; j.off_bc[i] = off_bias[i]; j.off_ns[i] = off_noise[i];
    if (C[i] > cmax) cmax = C[i];
  }
  const int ncols = (cmax + 31) / 32 * 64;
  hipLaunchKernelGGL(spade_vec_prep_multi_kernel, dim3((ncols + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, j, bias_interleaved_all,
                     noise_scale_padded_all);
  return check_launch("spade_vec_prep_multi_kernel");
}

static int shared_taps_fill(SharedTaps& p, const float* const* w, const float* const* b, float* const* gw, float* const* gb,
                            int32_t n, int32_t hid, int32_t c, int32_t cp) {
  HRV_REQUIRE(n >= 1 && n <= 4 && hid > 0 && c > 0 && cp >= c, "shared_taps: n in 1..4, cp >= c");
  memset(&p, 0, sizeof(p));
  for (int i = 0; i < n; ++i) {
    if (w) { HRV_REQUIRE(w[i] && b[i], "shared_taps: null weight"); p.w[i] = w[i]; p.b[i] = b[i]; }
    if (gw) { HRV_REQUIRE(gw[i] && gb[i], "shared_taps: null gradient"); p.gw[i] = gw[i]; p.gb[i] = gb[i]; }
  }
  p.n = n; p.hid = hid; p.c = c; p.cp = cp;
  return HRV_OK;
}

extern "C" int hrv_shared_taps_prep_f32(const float* const* w, const float* const* b, int32_t n, int32_t hid, int32_t c,
                                        int32_t cp, float* wt, float* bt, hrv_stream_t stream) {
  HRV_REQUIRE(w && b && wt && bt, "shared_taps_prep: null pointer");
  SharedTaps p;
  const int rc = shared_taps_fill(p, w, b, nullptr, nullptr, n, hid, c, cp);
  if (rc) return rc;
  hipLaunchKernelGGL(shared_taps_prep_kernel, dim3(grid_for((size_t)n * hid * 9 * cp)), dim3(256), 0, (hipStream_t)stream, p, wt, bt);
  return check_launch("shared_taps_prep_kernel");
}

extern "C" int hrv_shared_taps_grad_f32(const float* dw, const float* db, int32_t n, int32_t hid, int32_t c, int32_t cp,
                                        float* const* gw, float* const* gb, hrv_stream_t stream) {
  HRV_REQUIRE(dw && db && gw && gb, "shared_taps_grad: null pointer");
  SharedTaps p;
  const int rc = shared_taps_fill(p, nullptr, nullptr, gw, gb, n, hid, c, cp);
  if (rc) return rc;
  hipLaunchKernelGGL(shared_taps_grad_kernel, dim3(grid_for((size_t)n * hid * c * 9)), dim3(256), 0, (hipStream_t)stream, p, dw, db);
  return check_launch("shared_taps_grad_kernel");
}

extern "C" int hrv_loss_f32(const float* a, const float* b, int64_t n, int32_t mode, float lscale, float gscale,
                            float* grad, float* workspace, float* loss_out, int32_t accumulate, hrv_stream_t stream) {
  HRV_REQUIRE(a && workspace && loss_out && n > 0 && mode >= 0 && (mode & 15) <= 4 && (mode & ~31) == 0, "loss: bad args");
  HRV_REQUIRE(((mode & 15) != 0 && (mode & 15) != 4) || b, "loss: mode needs a target tensor");
  const int nb = grid_for((size_t)n) > 1024 ? 1024 : grid_for((size_t)n);
  hipStream_t st = (hipStream_t)stream;
  const int vec = (((uintptr_t)a | (uintptr_t)b | (uintptr_t)grad) & 15) == 0;
  hipLaunchKernelGGL(loss_kernel<false>, dim3(nb), dim3(256), 0, st, a, b, (size_t)n, mode, gscale, grad, workspace, vec);
  int rc = check_launch("loss_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(64), 0, st, workspace, nb, lscale, loss_out, accumulate);
  return check_launch("loss_final_kernel");
}

// the same over bf16-stored a and b (mixed-precision VGG taps); loss and gradient stay fp32
extern "C" int hrv_loss_bf16in_f32(const uint16_t* a, const uint16_t* b, int64_t n, int32_t mode, float lscale, float gscale,
                                   float* grad, float* workspace, float* loss_out, int32_t accumulate, hrv_stream_t stream) {
  HRV_REQUIRE(a && workspace && loss_out && n > 0 && mode >= 0 && (mode & 15) <= 4 && (mode & ~63) == 0, "loss_bf16in: bad args");
  HRV_REQUIRE(((mode & 15) != 0 && (mode & 15) != 4) || b, "loss_bf16in: mode needs a target tensor");
  const int nb = grid_for((size_t)n) > 1024 ? 1024 : grid_for((size_t)n);
  hipStream_t st = (hipStream_t)stream;
  const int vec = ((((uintptr_t)a | (uintptr_t)b) & 7) | ((uintptr_t)grad & 15)) == 0;
  hipLaunchKernelGGL(loss_kernel<true>, dim3(nb), dim3(256), 0, st, (const float*)a, (const float*)b, (size_t)n, mode, gscale, grad,
                     workspace, vec);
  int rc = check_launch("loss_kernel[bf16 in]");
  if (rc) return rc;
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(64), 0, st, workspace, nb, lscale, loss_out, accumulate);
  return check_launch("loss_final_kernel");
}

extern "C" int hrv_downsum2x2_nhwc_f32(const float* dhi, int32_t N, int32_t Hl, int32_t Wl, int32_t C, int32_t hi_cstride,
                                       int32_t hi_coff, float* dlo, int32_t lo_cstride, int32_t lo_coff,
                                       int32_t accumulate, hrv_stream_t stream) {
  HRV_REQUIRE(dhi && dlo && N > 0 && Hl > 0 && Wl > 0 && C > 0 && C % 4 == 0 &&
                  ((hi_cstride | hi_coff | lo_cstride | lo_coff) & 3) == 0, "downsum2x2: bad args");
  const size_t total = (size_t)N * Hl * Wl * (C / 4);
  hipLaunchKernelGGL(downsum2x2_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, dhi, N, Hl, Wl, C / 4,
                     hi_cstride, hi_coff, dlo, lo_cstride, lo_coff, accumulate);
  return check_launch("downsum2x2_kernel");
}

extern "C" int hrv_avgpool3x3s2_bwd_nhwc_f32(const float* dy, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dy_cstride,
                                             int32_t dy_coff, float* dx, int32_t dx_cstride, int32_t dx_coff,
                                             int32_t accumulate, hrv_stream_t stream) {
  HRV_REQUIRE(dy && dx && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 &&
                  ((dy_cstride | dy_coff | dx_cstride | dx_coff) & 3) == 0, "avgpool_bwd: bad args");
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  const size_t total = (size_t)N * H * W * (C / 4);
  hipLaunchKernelGGL(avgpool3s2_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, dy, N, H, W, C / 4,
                     Ho, Wo, dy_cstride, dy_coff, dx, dx_cstride, dx_coff, accumulate);
  return check_launch("avgpool3s2_bwd_kernel");
}

extern "C" int hrv_maxpool2x2_nhwc_f32(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, float* y,
                                       hrv_stream_t stream) {
  HRV_REQUIRE(x && y && N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 4 == 0, "maxpool: bad args");
  const size_t total = (size_t)N * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(maxpool2_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, N, H / 2, W / 2, C / 4, C,
                     y, C);
  return check_launch("maxpool2_kernel");
}

// bf16-stored x and y (mixed-precision VGG activations)
extern "C" int hrv_maxpool2x2_nhwc_bf16(const uint16_t* x, int32_t N, int32_t H, int32_t W, int32_t C, uint16_t* y,
                                        hrv_stream_t stream) {
  HRV_REQUIRE(x && y && N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 8 == 0, "maxpool_bf16: bad args");
  const size_t total = (size_t)N * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(maxpool2_kernel<true>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const float*)x, N, H / 2,
                     W / 2, C / 4, C, (float*)y, C);
  return check_launch("maxpool2_kernel[bf16]");
}

extern "C" int hrv_maxpool2x2_bwd_nhwc_f32(const float* x, const float* dy, int32_t N, int32_t H, int32_t W, int32_t C,
                                           float* dx, hrv_stream_t stream) {
  HRV_REQUIRE(x && dy && dx && N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 4 == 0, "maxpool_bwd: bad args");
  const size_t total = (size_t)N * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(maxpool2_bwd_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, dy, N, H / 2, W / 2,
                     C / 4, C, C, dx, 0);
  return check_launch("maxpool2_bwd_kernel");
}

// the same with the ReLU derivative of the pooled tensor fused (x = ReLU(pre): dx is the gradient w.r.t. pre)
extern "C" int hrv_maxpool2x2_bwd_relu_nhwc_f32(const float* x, const float* dy, int32_t N, int32_t H, int32_t W, int32_t C,
                                                float* dx, hrv_stream_t stream) {
  HRV_REQUIRE(x && dy && dx && N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 4 == 0, "maxpool_bwd_relu: bad args");
  const size_t total = (size_t)N * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(maxpool2_bwd_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, dy, N, H / 2, W / 2,
                     C / 4, C, C, dx, 1);
  return check_launch("maxpool2_bwd_kernel[relu]");
}

// ... with a bf16-stored x (dy, dx fp32)
extern "C" int hrv_maxpool2x2_bwd_relu_nhwc_xbf16(const uint16_t* x, const float* dy, int32_t N, int32_t H, int32_t W, int32_t C,
                                                  float* dx, hrv_stream_t stream) {
  HRV_REQUIRE(x && dy && dx && N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 8 == 0, "maxpool_bwd_xbf16: bad args");
  const size_t total = (size_t)N * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(maxpool2_bwd_kernel<true>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const float*)x, dy, N,
                     H / 2, W / 2, C / 4, C, C, dx, 1);
  return check_launch("maxpool2_bwd_kernel[relu, bf16 x]");
}

// ... with bf16-stored x, dy AND dx
extern "C" int hrv_maxpool2x2_bwd_relu_nhwc_bf16(const uint16_t* x, const uint16_t* dy, int32_t N, int32_t H, int32_t W, int32_t C,
                                                 uint16_t* dx, hrv_stream_t stream) {
  HRV_REQUIRE(x && dy && dx && N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 8 == 0, "maxpool_bwd_bf16: bad args");
  const size_t total = (size_t)N * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL((maxpool2_bwd_kernel<true, true>), dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                     (const float*)dy, N, H / 2, W / 2, C / 4, C, C, (float*)dx, 1);
  return check_launch("maxpool2_bwd_kernel[relu, bf16]");
}

extern "C" int hrv_add_slice_nhwc_bf16(const uint16_t* a, int32_t a_cstride, int32_t a_coff, uint16_t* out, int32_t out_cstride,
                                       int32_t out_coff, int32_t C, int64_t npix, int32_t accumulate, hrv_stream_t stream) {
  HRV_REQUIRE(a && out && npix > 0 && C > 0 && C % 4 == 0 && ((a_cstride | a_coff | out_cstride | out_coff) & 3) == 0,
              "add_slice_bf16: bad args");
  hipLaunchKernelGGL(add_slice_bf16_kernel, dim3(grid_for((size_t)npix * (C / 4))), dim3(256), 0, (hipStream_t)stream, a, a_cstride,
                     a_coff, out, out_cstride, out_coff, C / 4, (size_t)npix, accumulate);
  return check_launch("add_slice_bf16_kernel");
}

extern "C" int hrv_adam_f32(float* w, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                            float eps, float weight_decay, int32_t step, float grad_scale, hrv_stream_t stream) {
  HRV_REQUIRE(w && g && m && v && n > 0 && step >= 1, "adam: bad args");
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.f - powf(beta2, (float)step));
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, (hipStream_t)stream, w, g, m, v, (size_t)n, lr,
                     beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale);
  return check_launch("adam_kernel");
}

extern "C" int hrv_adam_hyper_f32(int32_t* step_dev, const float* lr_dev, float beta1, float beta2, float* hyper_dev,
                                  hrv_stream_t stream) {
  HRV_REQUIRE(step_dev && lr_dev && hyper_dev, "adam_hyper: null pointer");
  hipLaunchKernelGGL(adam_hyper_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step_dev, lr_dev, beta1, beta2, hyper_dev);
  return check_launch("adam_hyper_kernel");
}

extern "C" int hrv_adam_dev_f32(float* w, const float* g, float* m, float* v, int64_t n, const float* hyper_dev, float beta1,
                                float beta2, float eps, float weight_decay, float grad_scale, hrv_stream_t stream) {
  HRV_REQUIRE(w && g && m && v && hyper_dev && n > 0, "adam_dev: bad args");
  hipLaunchKernelGGL(adam_dev_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, (hipStream_t)stream, w, g, m, v, (size_t)n, hyper_dev,
                     beta1, beta2, eps, weight_decay, grad_scale);
  return check_launch("adam_dev_kernel");
}

extern "C" int hrv_spectral_norm_f32(const float* w, int32_t R, int32_t K, float* u, float* v, int32_t power_iterations,
                                     float eps, float* wv_scratch, float* sigma_out, hrv_stream_t stream) {
  HRV_REQUIRE(w && u && v && wv_scratch && sigma_out && R > 0 && K > 0 && power_iterations >= 0, "spectral_norm: bad args");
  hipStream_t st = (hipStream_t)stream;
  for (int it = 0; it < power_iterations; ++it) {
    // v <- normalize(W^T u) ; u <- normalize(W v)    (torch SpectralNorm.compute_weight)
    hipLaunchKernelGGL(gemv_cols_kernel, dim3((K + 63) / 64), dim3(256), 0, st, w, u, R, K, v);
    hipLaunchKernelGGL(normalize_kernel, dim3(1), dim3(256), 0, st, v, K, eps, (float*)nullptr);
    hipLaunchKernelGGL(gemv_rows_kernel, dim3(R), dim3(256), 0, st, w, v, R, K, u);
    hipLaunchKernelGGL(normalize_kernel, dim3(1), dim3(256), 0, st, u, R, eps, (float*)nullptr);
  }
  // sigma = u . (W v)
  hipLaunchKernelGGL(gemv_rows_kernel, dim3(R), dim3(256), 0, st, w, v, R, K, wv_scratch);
  hipLaunchKernelGGL(dot_partial_kernel, dim3(1), dim3(256), 0, st, u, wv_scratch, (size_t)R, sigma_out);
  return check_launch("spectral_norm kernels");
}

extern "C" int hrv_spectral_norm_batched_f32(const hrv_sn_job_t* jobs, int32_t n_jobs, int32_t power_iterations, float eps,
                                             float* wv_scratch, hrv_stream_t stream) {
  HRV_REQUIRE(jobs && n_jobs > 0 && wv_scratch && power_iterations >= 0, "spectral_norm_batched: bad args");
  hipStream_t st = (hipStream_t)stream;
  float* scratch = wv_scratch;
  for (int j0 = 0; j0 < n_jobs; j0 += SN_MAX) {
    SnBatch B;
    B.n = n_jobs - j0 < SN_MAX ? n_jobs - j0 : SN_MAX;
    B.eps = eps;
    B.col_blk[0] = B.row_blk[0] = 0;
    for (int j = 0; j < B.n; ++j) {
      const hrv_sn_job_t& s = jobs[j0 + j];
      HRV_REQUIRE(s.w && s.u && s.v && s.sigma && s.R > 0 && s.K > 0, "spectral_norm_batched: job %d", j0 + j);
      SnJob& J = B.job[j];
      J.w = s.w; J.u = s.u; J.v = s.v; J.sigma = s.sigma; J.u_keep = s.u_keep; J.v_keep = s.v_keep; J.R = s.R; J.K = s.K;
      J.wv = scratch;
      scratch += s.R;
      B.col_blk[j + 1] = B.col_blk[j] + (s.K + 63) / 64;
      B.row_blk[j + 1] = B.row_blk[j] + s.R;
    }
    for (int it = 0; it < power_iterations; ++it) {
      // v <- normalize(W^T u) ; u <- normalize(W v)    (torch SpectralNorm.compute_weight); the last pass also yields sigma
      hipLaunchKernelGGL(sn_gemv_cols_batched_kernel, dim3(B.col_blk[B.n]), dim3(256), 0, st, B);
      hipLaunchKernelGGL(sn_normalize_v_batched_kernel, dim3(B.n), dim3(256), 0, st, B);
      hipLaunchKernelGGL(sn_gemv_rows_batched_kernel, dim3(B.row_blk[B.n]), dim3(256), 0, st, B);
      // sigma = u . (W v) with the normalised u and the SAME W v (torch recomputes it: identical operands)
      hipLaunchKernelGGL(sn_finish_batched_kernel, dim3(B.n), dim3(256), 0, st, B, 1);
    }
    if (power_iterations == 0) {
      hipLaunchKernelGGL(sn_gemv_rows_batched_kernel, dim3(B.row_blk[B.n]), dim3(256), 0, st, B);
      hipLaunchKernelGGL(sn_finish_batched_kernel, dim3(B.n), dim3(256), 0, st, B, 0);
    }
  }
  return check_launch("spectral_norm_batched kernels");
}

extern "C" int hrv_spectral_norm_bwd_f32(const float* G, const float* w_orig, const float* u, const float* v,
                                         const float* sigma, int32_t R, int32_t K, float* workspace, float* dw_orig,
                                         int32_t accumulate, hrv_stream_t stream) {
  HRV_REQUIRE(G && w_orig && u && v && sigma && workspace && dw_orig && R > 0 && K > 0, "spectral_norm_bwd: bad args");
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)R * K;
  const int nb = grid_for(n) > 512 ? 512 : grid_for(n);
  hipLaunchKernelGGL(dot_partial_kernel, dim3(nb), dim3(256), 0, st, G, w_orig, n, workspace);
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(64), 0, st, workspace, nb, 1.0f, workspace + 512, 0);
  hipLaunchKernelGGL(sn_grad_kernel, dim3(grid_for(n)), dim3(256), 0, st, G, u, v, workspace + 512, sigma, R, K, dw_orig,
                     accumulate);
  return check_launch("spectral_norm_bwd kernels");
}

extern "C" int hrv_tanh_bwd_f32(const float* dy, const float* y, int64_t n, float* out, hrv_stream_t stream) {
  HRV_REQUIRE(dy && y && out && n > 0, "tanh_bwd: bad args");
  hipLaunchKernelGGL(tanh_bwd_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, (hipStream_t)stream, dy, y, (size_t)n, out);
  return check_launch("tanh_bwd_kernel");
}

extern "C" int hrv_add_slice_nhwc_f32(const float* a, int32_t a_cstride, int32_t a_coff, float* out, int32_t out_cstride,
                                      int32_t out_coff, int32_t C, int64_t npix, int32_t accumulate, hrv_stream_t stream) {
  HRV_REQUIRE(a && out && npix > 0 && C > 0 && C % 4 == 0 && ((a_cstride | a_coff | out_cstride | out_coff) & 3) == 0,
              "add_slice: bad args");
  hipLaunchKernelGGL(add_slice_kernel, dim3(grid_for((size_t)npix * (C / 4))), dim3(256), 0, (hipStream_t)stream, a,
                     a_cstride, a_coff, out, out_cstride, out_coff, C / 4, (size_t)npix, accumulate);
  return check_launch("add_slice_kernel");
}

extern "C" int hrv_act_bwd_nhwc_f32(float* d, int32_t d_cstride, int32_t d_coff, const float* y, int32_t y_cstride,
                                    int32_t y_coff, int32_t C, int64_t npix, int32_t act, float act_slope,
                                    hrv_stream_t stream) {
  HRV_REQUIRE(d && y && npix > 0 && C > 0 && C % 4 == 0 && ((d_cstride | d_coff | y_cstride | y_coff) & 3) == 0,
              "act_bwd: bad args");
  hipLaunchKernelGGL(act_bwd_kernel, dim3(grid_for((size_t)npix * (C / 4))), dim3(256), 0, (hipStream_t)stream, d, d_cstride,
                     d_coff, y, y_cstride, y_coff, C / 4, (size_t)npix, act, act_slope);
  return check_launch("act_bwd_kernel");
}

extern "C" int hrv_scale_f32(float* x, int64_t n, float s_host, const float* s_dev, hrv_stream_t stream) {
  HRV_REQUIRE(x && n > 0, "scale: bad args");
  hipLaunchKernelGGL(scale_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, (hipStream_t)stream, x, (size_t)n, s_host, s_dev);
  return check_launch("scale_kernel");
}
