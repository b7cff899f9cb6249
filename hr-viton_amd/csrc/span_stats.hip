// Per-parameter statistics of the optimizer's flat buffers (ABI and record layout: include/hrviton_hip.h): a segmented reduction
// in the store-and-sum form, read-only, no atomics, nothing read back.
//   span_stats_kernel           one 256-thread BLOCK per piece (<= SPAN_PIECE elements of one span), grid-strided over the piece
//                               table: reads g, w (and m, v) over the piece's elements only, stores one partial record per piece
//   span_stats_finalize_kernel  one WAVE per span: adds the span's partials in index order, stores the span's record
// Determinism: the piece table is built by the host from the spans alone (never from the CU count), a piece is reduced by one
// block whatever the grid, the element -> thread rule depends only on (the piece's first address, its length), and every sum has a
// fixed order: per thread over its float4 trips in turn, then its head and its tail elements; a 64-lane shuffle tree; waves 0..3
// through LDS in wave order; in the second launch lane l over partials l, l + 64, ... in turn, then the shuffle tree.
// Squares are taken and added in fp64, as the guard does (csrc/grad_guard.hip).
#include "hrv_common.h"

namespace hrv {

constexpr int SPAN_PIECE = 16384;      // elements per piece: 16 float4 trips of a block; the generator's 100.5 M elements -> ~6.4 k pieces
constexpr int SPAN_BLOCK = 256;
constexpr int SPAN_GRID_CAP = 1 << 16;

struct SpanAcc {
  double gs, ws, us;
  float gm, wm, um;
  int gn, wn, un, gz;
};

__device__ __forceinline__ bool span_nonfinite(float x) { return (__builtin_bit_cast(unsigned, x) & 0x7f800000u) == 0x7f800000u; }

__device__ __forceinline__ void span_acc1(float x, double& s, float& mx, int& nf) {
  if (span_nonfinite(x)) {
    nf += 1;
  } else {
    const double d = (double)x;
    s += d * d;
    mx = fmaxf(mx, fabsf(x));
  }
}

// the Adam update's direction, rounded like adam_elem's mi / denom (csrc/adam_body.h): every operation on its own
__device__ __forceinline__ float span_update(float m, float v, float bc2_sqrt, float eps) {
#pragma clang fp contract(off)
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  return m / denom;
}

template <bool MV>
__device__ __forceinline__ void span_elem(float g, float w, float m, float v, float bc2_sqrt, float eps, SpanAcc& a) {
  span_acc1(g, a.gs, a.gm, a.gn);
  a.gz += g == 0.f;
  span_acc1(w, a.ws, a.wm, a.wn);
  if constexpr (MV) {
    const float u = span_update(m, v, bc2_sqrt, eps);
    if (span_nonfinite(m) || span_nonfinite(v) || span_nonfinite(u)) {
      a.un += 1;
    } else {
      const double d = (double)u;
      a.us += d * d;
      a.um = fmaxf(a.um, fabsf(u));
    }
  }
}

template <bool MV>
__device__ __forceinline__ void span_scalar(const float* __restrict__ g, const float* __restrict__ w, const float* __restrict__ m,
                                            const float* __restrict__ v, size_t i, float bc2_sqrt, float eps, SpanAcc& a) {
  float mi = 0.f, vi = 0.f;
  if constexpr (MV) {
    mi = m[i];
    vi = v[i];
  }
  span_elem<MV>(g[i], w[i], mi, vi, bc2_sqrt, eps, a);
}

__device__ __forceinline__ void span_wave_reduce(SpanAcc& a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.gs += __shfl_down(a.gs, o, 64);
    a.ws += __shfl_down(a.ws, o, 64);
    a.us += __shfl_down(a.us, o, 64);
    a.gm = fmaxf(a.gm, __shfl_down(a.gm, o, 64));
    a.wm = fmaxf(a.wm, __shfl_down(a.wm, o, 64));
    a.um = fmaxf(a.um, __shfl_down(a.um, o, 64));
    a.gn += __shfl_down(a.gn, o, 64);
    a.wn += __shfl_down(a.wn, o, 64);
    a.un += __shfl_down(a.un, o, 64);
    a.gz += __shfl_down(a.gz, o, 64);
  }
}

__device__ __forceinline__ void span_add(SpanAcc& a, const SpanAcc& b) {
  a.gs += b.gs;
  a.ws += b.ws;
  a.us += b.us;
  a.gm = fmaxf(a.gm, b.gm);
  a.wm = fmaxf(a.wm, b.wm);
  a.um = fmaxf(a.um, b.um);
  a.gn += b.gn;
  a.wn += b.wn;
  a.un += b.un;
  a.gz += b.gz;
}

__device__ __forceinline__ void span_store(int32_t* __restrict__ rec, const SpanAcc& a) {
  double* d = reinterpret_cast<double*>(rec);
  d[HRV_SPAN_G_SUMSQ / 2] = a.gs;
  d[HRV_SPAN_W_SUMSQ / 2] = a.ws;
  d[HRV_SPAN_U_SUMSQ / 2] = a.us;
  rec[HRV_SPAN_G_MAXABS] = __builtin_bit_cast(int32_t, a.gm);
  rec[HRV_SPAN_W_MAXABS] = __builtin_bit_cast(int32_t, a.wm);
  rec[HRV_SPAN_U_MAXABS] = __builtin_bit_cast(int32_t, a.um);
  rec[HRV_SPAN_G_NONFINITE] = a.gn;
  rec[HRV_SPAN_W_NONFINITE] = a.wn;
  rec[HRV_SPAN_U_NONFINITE] = a.un;
  rec[HRV_SPAN_G_ZEROS] = a.gz;
  rec[13] = rec[14] = rec[15] = 0;
}

__device__ __forceinline__ SpanAcc span_load(const int32_t* __restrict__ rec) {
  const double* d = reinterpret_cast<const double*>(rec);
  SpanAcc a;
  a.gs = d[HRV_SPAN_G_SUMSQ / 2];
  a.ws = d[HRV_SPAN_W_SUMSQ / 2];
  a.us = d[HRV_SPAN_U_SUMSQ / 2];
  a.gm = __builtin_bit_cast(float, rec[HRV_SPAN_G_MAXABS]);
  a.wm = __builtin_bit_cast(float, rec[HRV_SPAN_W_MAXABS]);
  a.um = __builtin_bit_cast(float, rec[HRV_SPAN_U_MAXABS]);
  a.gn = rec[HRV_SPAN_G_NONFINITE];
  a.wn = rec[HRV_SPAN_W_NONFINITE];
  a.un = rec[HRV_SPAN_U_NONFINITE];
  a.gz = rec[HRV_SPAN_G_ZEROS];
  return a;
}

// piece = [first, first + len): ``head`` scalar elements up to the first 16-byte boundary the arrays share | n4 float4 groups, group
// i to thread i mod 256 | the scalar tail.  Arrays whose 16-byte phases differ share no boundary: the whole piece is head.
template <bool MV>
__global__ __launch_bounds__(SPAN_BLOCK) void span_stats_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                               const float* __restrict__ m, const float* __restrict__ v,
                                                               const int64_t* __restrict__ pieces, int n_pieces,
                                                               const float* __restrict__ hyper, float bc2_arg, float eps,
                                                               int32_t* __restrict__ part) {
  __shared__ SpanAcc red[SPAN_BLOCK / 64];
  const float bc2_sqrt = hyper ? hyper[2] : bc2_arg;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int p = blockIdx.x; p < n_pieces; p += gridDim.x) {
    const size_t first = (size_t)pieces[2 * (size_t)p], len = (size_t)pieces[2 * (size_t)p + 1];
    const float *gp = g + first, *wp = w + first, *mp = MV ? m + first : nullptr, *vp = MV ? v + first : nullptr;
    const unsigned ph = ((uintptr_t)gp >> 2) & 3;
    bool same = ph == (((uintptr_t)wp >> 2) & 3);
    if constexpr (MV) same = same && ph == (((uintptr_t)mp >> 2) & 3) && ph == (((uintptr_t)vp >> 2) & 3);
    size_t head = same ? (size_t)((4 - ph) & 3) : len;
    if (head > len) head = len;
    const size_t n4 = (len - head) / 4, tail0 = head + 4 * n4;
    SpanAcc a = {0.0, 0.0, 0.0, 0.f, 0.f, 0.f, 0, 0, 0, 0};
    const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(gp + head);
    const f32x4* __restrict__ w4 = reinterpret_cast<const f32x4*>(wp + head);
    const f32x4* __restrict__ m4 = reinterpret_cast<const f32x4*>(MV ? mp + head : nullptr);
    const f32x4* __restrict__ v4 = reinterpret_cast<const f32x4*>(MV ? vp + head : nullptr);
    for (size_t i = threadIdx.x; i < n4; i += SPAN_BLOCK) {
      const f32x4 gx = g4[i], wx = w4[i];
      f32x4 mx = {0.f, 0.f, 0.f, 0.f}, vx = {0.f, 0.f, 0.f, 0.f};
      if constexpr (MV) {
        mx = m4[i];
        vx = v4[i];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) span_elem<MV>(gx[e], wx[e], mx[e], vx[e], bc2_sqrt, eps, a);
    }
    for (size_t i = threadIdx.x; i < head; i += SPAN_BLOCK) span_scalar<MV>(gp, wp, mp, vp, i, bc2_sqrt, eps, a);
    for (size_t i = tail0 + threadIdx.x; i < len; i += SPAN_BLOCK) span_scalar<MV>(gp, wp, mp, vp, i, bc2_sqrt, eps, a);
    span_wave_reduce(a);
    if (lane == 0) red[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
      SpanAcc t = red[0];
#pragma unroll
      for (int k = 1; k < SPAN_BLOCK / 64; ++k) span_add(t, red[k]);
      span_store(part + (size_t)p * HRV_SPAN_WORDS, t);
    }
    __syncthreads();      // (red is written again by the block's next piece)
  }
}

// wave (blockIdx.x * 4 + threadIdx.x / 64) owns one span
__global__ __launch_bounds__(SPAN_BLOCK) void span_stats_finalize_kernel(const int32_t* __restrict__ part,
                                                                        const int32_t* __restrict__ span_first, int n_spans,
                                                                        int32_t* __restrict__ rec) {
  const int s = blockIdx.x * (SPAN_BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= n_spans) return;      // (wave-uniform; no barrier below)
  const int p0 = span_first[s], p1 = span_first[s + 1];
  SpanAcc a = {0.0, 0.0, 0.0, 0.f, 0.f, 0.f, 0, 0, 0, 0};
  for (int p = p0 + lane; p < p1; p += 64) span_add(a, span_load(part + (size_t)p * HRV_SPAN_WORDS));
  span_wave_reduce(a);
  if (lane == 0) span_store(rec + (size_t)s * HRV_SPAN_WORDS, a);
}

}  // namespace hrv

using namespace hrv;

extern "C" int hrv_span_stats_piece(void) { return SPAN_PIECE; }

extern "C" int hrv_span_stats_f32(const float* g, const float* w, const float* m, const float* v, const int64_t* pieces,
                                  int32_t n_pieces, const float* hyper_dev, float bc2_sqrt, float eps, void* part,
                                  hrv_stream_t stream) {
  HRV_REQUIRE(g && w && pieces && part && n_pieces >= 1 && (m != nullptr) == (v != nullptr),
              "span_stats: bad args (null pointer, n_pieces < 1, or only one of m / v)");
  HRV_REQUIRE((((uintptr_t)g | (uintptr_t)w | (uintptr_t)m | (uintptr_t)v | (uintptr_t)hyper_dev) & 3) == 0 &&
                  (((uintptr_t)pieces | (uintptr_t)part) & 7) == 0,
              "span_stats: misaligned pointer (4 bytes for the arrays, 8 for the piece table and the partials)");
  const int grid = n_pieces < SPAN_GRID_CAP ? n_pieces : SPAN_GRID_CAP;
  if (m)
    hipLaunchKernelGGL((span_stats_kernel<true>), dim3(grid), dim3(SPAN_BLOCK), 0, (hipStream_t)stream, g, w, m, v, pieces,
                       (int)n_pieces, hyper_dev, bc2_sqrt, eps, (int32_t*)part);
  else
    hipLaunchKernelGGL((span_stats_kernel<false>), dim3(grid), dim3(SPAN_BLOCK), 0, (hipStream_t)stream, g, w, m, v, pieces,
                       (int)n_pieces, hyper_dev, bc2_sqrt, eps, (int32_t*)part);
  return check_launch("span_stats_kernel");
}

extern "C" int hrv_span_stats_finalize(const void* part, const int32_t* span_first, int32_t n_spans, int32_t* records,
                                       hrv_stream_t stream) {
  HRV_REQUIRE(part && span_first && records && n_spans >= 1 && (((uintptr_t)part | (uintptr_t)records) & 7) == 0 &&
                  ((uintptr_t)span_first & 3) == 0,
              "span_stats_finalize: bad args (null pointer, n_spans < 1 or misaligned)");
  const int per = SPAN_BLOCK / 64;
  hipLaunchKernelGGL(span_stats_finalize_kernel, dim3((n_spans + per - 1) / per), dim3(SPAN_BLOCK), 0, (hipStream_t)stream,
                     (const int32_t*)part, span_first, (int)n_spans, records);
  return check_launch("span_stats_finalize_kernel");
}
