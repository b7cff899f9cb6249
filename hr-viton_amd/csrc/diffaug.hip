// DiffAugment (color, translation, cutout) inside the PatchGAN input assembly (ABI and the definition of the transform:
// include/hrviton_hip.h).  Four pieces, all decided on the device from the caller's uniforms u [N][8]:
//   diffaug_mean_kernel    per-sample mean of the un-translated NCHW images of both halves (color only)
//   diffaug_concat_kernel  the augmenting twin of concat_nhwc_nchw_v4_kernel (sample.hip): gather, select, color
//   diffaug_gsum_kernel    per-sample sum of the selected gradient over the three image channels (color only)
//   diffaug_bwd_kernel     the augmenting twin of the to_nchw slice that extracts d(fake): the adjoint, every element written
// The three kernels that read the policy are templates (template <bool GATED, typename... Gate>): the gated instances (ADA, Karras
// et al. 2020) take two more arguments and narrow the policy per sample from the gate uniforms ug [N][4] and the probability p[0]
// in the scalar decode at the top; the ungated instances have an empty pack, the parameters and the body they always had.
//   ada_update_kernel      the controller that moves p from the loss head's r_t (one thread, eight fp64 words of state)
// Geometry is a pure gather and select: a masked pixel is never loaded and the address of an out-of-range source is never
// formed, so nothing a masked source (forward) or a masked destination gradient (backward) holds can reach the result.
// Color is evaluated in fp64 from the fp32 decode and rounded once.  Determinism of the two reductions as in grad_guard.hip:
// the slot count is a compile-time constant, block (s, j) IS slot s of sample j, the element -> thread rule depends only on
// (pointer alignment, extents), every sum has a fixed order (per thread over its trips, a 64-lane shuffle tree, the four waves
// through LDS in wave order, the slots in the same tree).  No atomics.
#include "hrv_common.h"

namespace hrv {

constexpr int AUG_SLOTS = HRV_DIFFAUG_SLOTS;      // partial sums per sample
constexpr int AUG_BLOCK = 256;
static_assert(AUG_SLOTS <= AUG_BLOCK, "the finalisation reads one slot per thread");

// the decoded transform of one sample: source = destination + (ty, tx); box rows [y0, y1), columns [x0, x1), clipped (empty: no box)
struct AugGeom {
  int ty, tx, y0, y1, x0, x1;
};

__device__ __forceinline__ int aug_shift(float u, int extent) {
  const int S = (extent + 4) / 8;
  return min((int)(u * (float)(2 * S + 1)), 2 * S) - S;
}

__device__ __forceinline__ void aug_box(float u, int extent, int& lo, int& hi) {
  const int c = extent / 2, odd = c & 1;
  const int o = min((int)(u * (float)(extent + 1 - odd)), extent - odd);
  lo = max(o - c / 2, 0);
  hi = min(o - c / 2 + c, extent);
}

__device__ __forceinline__ AugGeom aug_geom(const float* __restrict__ un, int flags, int H, int W) {
  AugGeom g = {0, 0, 0, 0, 0, 0};
  if (flags & HRV_DIFFAUG_TRANSLATION) {
    g.ty = aug_shift(un[3], H);
    g.tx = aug_shift(un[4], W);
  }
  if (flags & HRV_DIFFAUG_CUTOUT) {
    aug_box(un[5], H, g.y0, g.y1);
    aug_box(un[6], W, g.x0, g.x1);
  }
  return g;
}

__device__ __forceinline__ bool aug_in_box(const AugGeom& g, int y, int x) { return y >= g.y0 && y < g.y1 && x >= g.x0 && x < g.x1; }
__device__ __forceinline__ bool aug_inside(int y, int x, int H, int W) { return (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W; }

// The effective policy of sample n.  An ungated instance has no gate arguments (an empty pack: the parameter list it always had)
// and takes the policy as it is; a gated one gets (ug [N][4], p) and keeps a transform only where (double)ug < p[0], strict, in
// fp64 -- block-uniform like u's row: scalar loads, a scalar result.
template <bool GATED>
__device__ __forceinline__ int aug_flags(int policy, int) {
  static_assert(!GATED, "a gated instance takes (ug, p)");
  return policy;
}
template <bool GATED>
__device__ __forceinline__ int aug_flags(int policy, int n, const float* __restrict__ ug, const double* __restrict__ p) {
  static_assert(GATED, "an ungated instance takes no gate");
  const float* __restrict__ gn = ug + (size_t)n * 4;
  const double pv = p[0];
  return policy & (((double)gn[0] < pv ? HRV_DIFFAUG_COLOR : 0) | ((double)gn[1] < pv ? HRV_DIFFAUG_TRANSLATION : 0) |
                   ((double)gn[2] < pv ? HRV_DIFFAUG_CUTOUT : 0));
}

// the 256 partial sums of a block -> thread 0, fixed order: shuffle tree inside each wave, then waves 0..3 in turn
__device__ __forceinline__ void aug_block_sum(double& s) {
  __shared__ double red[AUG_BLOCK / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    s = red[0];
#pragma unroll
    for (int k = 1; k < AUG_BLOCK / 64; ++k) s += red[k];
  }
}

// sample j of [fake ; real] (n = 3HW floats each): x[0, head) scalar | n4 float4 groups from the first 16-byte boundary | the
// scalar tail.  A sample's base is only 4-byte aligned when 3HW % 4 != 0, so head is worked out per sample.  Group i belongs to
// thread i mod (AUG_SLOTS * 256) of the sample's row of blocks; head and tail elements (at most 3 each) to threads 0..2 of slot 0.
__global__ __launch_bounds__(AUG_BLOCK) void diffaug_mean_kernel(const float* __restrict__ fake, const float* __restrict__ real,
                                                                 int N, size_t n, double* __restrict__ part) {
  const int j = blockIdx.y;
  const float* __restrict__ x = j < N ? fake + (size_t)j * n : real + (size_t)(j - N) * n;
  size_t head = ((16 - ((uintptr_t)x & 15)) & 15) / 4;
  if (head > n) head = n;
  const size_t n4 = (n - head) / 4;
  const f32x4* __restrict__ body = reinterpret_cast<const f32x4*>(x + head);
  double s = 0.0;
  for (size_t i = (size_t)blockIdx.x * AUG_BLOCK + threadIdx.x; i < n4; i += (size_t)AUG_SLOTS * AUG_BLOCK) {
    const f32x4 v = body[i];
    s += ((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3]);
  }
  if (blockIdx.x == 0) {
    const size_t t = threadIdx.x, tail0 = head + 4 * n4;
    if (t < head) s += (double)x[t];
    if (tail0 + t < n) s += (double)x[tail0 + t];
  }
  aug_block_sum(s);
  if (threadIdx.x == 0) part[(size_t)j * AUG_SLOTS + blockIdx.x] = s;
}

// one block per sample: the slots in a fixed tree; mean (fp32) = sum / count, or the raw sum (fp64)
__global__ __launch_bounds__(AUG_BLOCK) void diffaug_finalize_kernel(const double* __restrict__ part, double count, float* __restrict__ mean,
                                                                     double* __restrict__ sum) {
  double s = threadIdx.x < AUG_SLOTS ? part[(size_t)blockIdx.x * AUG_SLOTS + threadIdx.x] : 0.0;
  aug_block_sum(s);
  if (threadIdx.x != 0) return;
  if (mean) mean[blockIdx.x] = (float)(s / count);
  if (sum) sum[blockIdx.x] = s;
}

// channels [ca, ca + 3) of a 12-float row held as three float4: compile-time positions, run-time ca (selects, no indexing)
__device__ __forceinline__ void aug_pick3(const f32x4 r0, const f32x4 r1, const f32x4 r2, int ca, float v[3]) {
  const float r[12] = {r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], r1[2], r1[3], r2[0], r2[1], r2[2], r2[3]};
  v[0] = v[1] = v[2] = 0.f;
#pragma unroll
  for (int c = 0; c < 12; ++c) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = (c == ca + k) ? r[c] : v[k];
  }
}

// One thread per DESTINATION pixel: the parse row of the source as two 16-byte loads, the three plane reads coalesced across the
// wave (the source is the destination shifted by whole pixels), three 16-byte stores.  V == 0: twelve zeros, nothing loaded.
template <bool GATED, typename... Gate>
__global__ __launch_bounds__(AUG_BLOCK) void diffaug_concat_kernel(const float* __restrict__ a, int Ca, const float* __restrict__ b,
                                                                   const float* __restrict__ u, const float* __restrict__ M,
                                                                   int policy, int H, int W, float* __restrict__ out, Gate... gate) {
  const int n = blockIdx.y, HW = H * W;      // (the sample is uniform over the block: its decode lives in scalar registers)
  const float* __restrict__ un = u + (size_t)n * 8;
  const int flags = aug_flags<GATED>(policy, n, gate...);
  const AugGeom g = aug_geom(un, flags, H, W);
  for (int p = blockIdx.x * AUG_BLOCK + threadIdx.x; p < HW; p += gridDim.x * AUG_BLOCK) {
    const int y = p / W, x = p - y * W;
    const int sy = y + g.ty, sx = x + g.tx;
    float o[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) o[c] = 0.f;
    if (aug_inside(sy, sx, H, W) && !aug_in_box(g, y, x)) {
      const size_t q = (size_t)n * HW + (size_t)sy * W + sx;
      const f32x4 a0 = ld4(a + q * 8), a1 = ld4(a + q * 8 + 4);
      const float av[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
      const float* __restrict__ bp = b + (size_t)n * 3 * HW + (size_t)sy * W + sx;
      float v[3] = {bp[0], bp[(size_t)HW], bp[2 * (size_t)HW]};
      if (flags & HRV_DIFFAUG_COLOR) {
        // k s x_c + k (1 - s) m + (1 - k) M + beta, in fp64 from the fp32 decode, one rounding
        const float beta = un[0] - 0.5f, s = 2.f * un[1], k = un[2] + 0.5f;
        const double kd = (double)k, sd = (double)s;
        const double m = ((double)v[0] + (double)v[1] + (double)v[2]) / 3.0;
        const double rest = kd * (1.0 - sd) * m + (1.0 - kd) * (double)M[n] + (double)beta;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (float)(kd * sd * (double)v[c] + rest);
      }
#pragma unroll
      for (int c = 0; c < 12; ++c) {
        const int k = c - Ca;
        o[c] = c < Ca ? av[c < 8 ? c : 7] : (k == 0 ? v[0] : (k == 1 ? v[1] : (k == 2 ? v[2] : 0.f)));
      }
    }
    f32x4* op = reinterpret_cast<f32x4*>(out + ((size_t)n * HW + p) * 12);
    op[0] = f32x4{o[0], o[1], o[2], o[3]};
    op[1] = f32x4{o[4], o[5], o[6], o[7]};
    op[2] = f32x4{o[8], o[9], o[10], o[11]};
  }
}

// G = V ? g : 0 summed over the destination pixels and the three image channels of sample blockIdx.y (slot blockIdx.x)
template <bool GATED, typename... Gate>
__global__ __launch_bounds__(AUG_BLOCK) void diffaug_gsum_kernel(const float* __restrict__ gr, int Ca, const float* __restrict__ u,
                                                                 int policy, int H, int W, double* __restrict__ part, Gate... gate) {
  const int n = blockIdx.y, HW = H * W;
  const int flags = aug_flags<GATED>(policy, n, gate...);
  const AugGeom g = aug_geom(u + (size_t)n * 8, flags, H, W);
  double s = 0.0;
  for (int p = blockIdx.x * AUG_BLOCK + threadIdx.x; p < HW; p += AUG_SLOTS * AUG_BLOCK) {
    const int y = p / W, x = p - y * W;
    if (aug_inside(y + g.ty, x + g.tx, H, W) && !aug_in_box(g, y, x)) {
      const float* __restrict__ row = gr + ((size_t)n * HW + p) * 12;
      float v[3];
      aug_pick3(ld4(row), ld4(row + 4), ld4(row + 8), Ca, v);
      s += ((double)v[0] + (double)v[1]) + (double)v[2];
    }
  }
  aug_block_sum(s);
  if (threadIdx.x == 0) part[(size_t)n * AUG_SLOTS + blockIdx.x] = s;
}

// One thread per SOURCE pixel (y', x') of d(image): the destination that read it is (y' - ty, x' - tx).  Reads that destination's
// gradient row (48 contiguous bytes a lane), writes the three planes coalesced.  Every element of d_img is written.
template <bool GATED, typename... Gate>
__global__ __launch_bounds__(AUG_BLOCK) void diffaug_bwd_kernel(const float* __restrict__ gr, int Ca, const float* __restrict__ u,
                                                                const double* __restrict__ gsum, int policy, int H, int W,
                                                                float* __restrict__ d_img, Gate... gate) {
  const int n = blockIdx.y, HW = H * W;
  const float* __restrict__ un = u + (size_t)n * 8;
  const int flags = aug_flags<GATED>(policy, n, gate...);
  const AugGeom g = aug_geom(un, flags, H, W);
  for (int p = blockIdx.x * AUG_BLOCK + threadIdx.x; p < HW; p += gridDim.x * AUG_BLOCK) {
    const int y = p / W, x = p - y * W;
    const int dy = y - g.ty, dx = x - g.tx;
    float v[3] = {0.f, 0.f, 0.f};
    if (aug_inside(dy, dx, H, W) && !aug_in_box(g, dy, dx)) {
      const float* __restrict__ row = gr + ((size_t)n * HW + (size_t)dy * W + dx) * 12;
      aug_pick3(ld4(row), ld4(row + 4), ld4(row + 8), Ca, v);
    }
    if (flags & HRV_DIFFAUG_COLOR) {
      // k s G_c + (k (1 - s) / 3) sum_c' G_c' + ((1 - k) / (3 HW)) sum G: fp64 from the fp32 decode, one rounding
      const float s = 2.f * un[1], k = un[2] + 0.5f;
      const double kd = (double)k, sd = (double)s;
      const double rest = kd * (1.0 - sd) * (((double)v[0] + (double)v[1] + (double)v[2]) / 3.0) +
                          (1.0 - kd) * (gsum[n] / (3.0 * (double)HW));
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = (float)(kd * sd * (double)v[c] + rest);
    }
    float* __restrict__ dp = d_img + (size_t)n * 3 * HW + p;
    dp[0] = v[0];
    dp[(size_t)HW] = v[1];
    dp[2 * (size_t)HW] = v[2];
  }
}

// The ADA controller (the order of every operation is the header's): one thread, all words fp64.  s * step is exact (s is -1, 0 or
// 1), so a contraction into a fused multiply-add gives the same bits.
__global__ void ada_update_kernel(const double* __restrict__ rec, int num_d, double target, double step, int interval, double p_max,
                                  double* __restrict__ st) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  st[HRV_ADA_STEPS] += 1.0;
  if (rec[HRV_DHEAD_NONFINITE] != 0.0) return;
  double sum = 0.0;
  for (int k = 0; k < num_d; ++k) sum += rec[HRV_DHEAD_STATE + HRV_DHEAD_SCALE_WORDS * k + HRV_DHEAD_RT];
  const double r = sum / (double)num_d;
  st[HRV_ADA_RT_LAST] = r;
  const double acc = st[HRV_ADA_ACC] + r, seen = st[HRV_ADA_SEEN] + 1.0;
  if (seen != (double)interval) {
    st[HRV_ADA_ACC] = acc;
    st[HRV_ADA_SEEN] = seen;
    return;
  }
  const double m = acc / (double)interval;
  const double s = (double)((m > target) - (m < target));
  st[HRV_ADA_RT_WINDOW] = m;
  st[HRV_ADA_P] = fmin(fmax(st[HRV_ADA_P] + s * step, 0.0), p_max);
  st[HRV_ADA_ACC] = 0.0;
  st[HRV_ADA_SEEN] = 0.0;
  st[HRV_ADA_UPDATES] += 1.0;
}

// blocks over the pixels of ONE sample (the grid's y is the sample): 256 CUs x 16 blocks over the batch, grid-stride the rest
static inline dim3 aug_grid_for(int HW, int N) {
  const int g = (HW + AUG_BLOCK - 1) / AUG_BLOCK, cap = (256 * 16 + N - 1) / N;
  return dim3((unsigned)(g > cap ? cap : g), (unsigned)N);
}

// the PatchGAN shape only; H * W and N * H * W * 12 stay far inside int / size_t
static inline bool aug_shape_ok(int32_t N, int32_t H, int32_t W) {
  return N > 0 && H > 0 && W > 0 && (int64_t)H * W <= (1 << 28) && (int64_t)N * H * W <= ((int64_t)1 << 31) && N <= 65535;
}
static inline bool aug_policy_ok(int32_t policy) {
  return policy >= 0 && policy <= (HRV_DIFFAUG_COLOR | HRV_DIFFAUG_TRANSLATION | HRV_DIFFAUG_CUTOUT);
}

}  // namespace hrv

using namespace hrv;

extern "C" int hrv_diffaug_mean_f32(const float* fake, const float* real, int32_t N, int32_t H, int32_t W, double* part, float* mean,
                                    hrv_stream_t stream) {
  HRV_REQUIRE(fake && part && mean && aug_shape_ok(N, H, W) && 2 * (int64_t)N <= 65535, "diffaug_mean: bad args");
  HRV_REQUIRE(((uintptr_t)fake & 3) == 0 && ((uintptr_t)real & 3) == 0 && ((uintptr_t)part & 7) == 0 && ((uintptr_t)mean & 3) == 0,
              "diffaug_mean: misaligned pointer");
  const int rows = real ? 2 * N : N;
  const size_t n = (size_t)3 * H * W;
  hipLaunchKernelGGL(diffaug_mean_kernel, dim3(AUG_SLOTS, rows), dim3(AUG_BLOCK), 0, (hipStream_t)stream, fake, real, N, n, part);
  int rc = check_launch("diffaug_mean_kernel");
  if (rc != HRV_OK) return rc;
  hipLaunchKernelGGL(diffaug_finalize_kernel, dim3(rows), dim3(AUG_BLOCK), 0, (hipStream_t)stream, (const double*)part, (double)n, mean,
                     (double*)nullptr);
  return check_launch("diffaug_finalize_kernel");
}

extern "C" int hrv_diffaug_concat_f32(const float* a, int32_t Ca, int32_t a_cstride, const float* b, const float* u, const float* mean,
                                      int32_t policy, int32_t N, int32_t H, int32_t W, float* out, int32_t out_cstride,
                                      hrv_stream_t stream) {
  HRV_REQUIRE(a && b && u && out && aug_shape_ok(N, H, W) && aug_policy_ok(policy), "diffaug_concat: bad args");
  HRV_REQUIRE(Ca >= 1 && Ca <= 8 && a_cstride == 8 && out_cstride == 12,
              "diffaug_concat: serves the PatchGAN shape only (parse stride 8 with C <= 8, 3 image channels, output stride 12)");
  HRV_REQUIRE((((uintptr_t)a | (uintptr_t)out) & 15) == 0 && (((uintptr_t)b | (uintptr_t)u | (uintptr_t)mean) & 3) == 0,
              "diffaug_concat: misaligned pointer");
  HRV_REQUIRE(mean || !(policy & HRV_DIFFAUG_COLOR), "diffaug_concat: color needs the per-sample means");
  hipLaunchKernelGGL(diffaug_concat_kernel<false>, aug_grid_for(H * W, N), dim3(AUG_BLOCK), 0, (hipStream_t)stream, a, (int)Ca, b, u, mean, (int)policy,
                     (int)H, (int)W, out);
  return check_launch("diffaug_concat_kernel");
}

extern "C" int hrv_diffaug_gsum_f32(const float* g, int32_t g_cstride, int32_t Ca, const float* u, int32_t policy, int32_t N, int32_t H,
                                    int32_t W, double* part, double* sum, hrv_stream_t stream) {
  HRV_REQUIRE(g && u && part && sum && aug_shape_ok(N, H, W) && aug_policy_ok(policy), "diffaug_gsum: bad args");
  HRV_REQUIRE(Ca >= 1 && Ca <= 8 && g_cstride == 12, "diffaug_gsum: serves the PatchGAN shape only (gradient stride 12, C <= 8 + 3)");
  HRV_REQUIRE(((uintptr_t)g & 15) == 0 && ((uintptr_t)u & 3) == 0 && (((uintptr_t)part | (uintptr_t)sum) & 7) == 0,
              "diffaug_gsum: misaligned pointer");
  hipLaunchKernelGGL(diffaug_gsum_kernel<false>, dim3(AUG_SLOTS, N), dim3(AUG_BLOCK), 0, (hipStream_t)stream, g, (int)Ca, u, (int)policy, (int)H,
                     (int)W, part);
  int rc = check_launch("diffaug_gsum_kernel");
  if (rc != HRV_OK) return rc;
  hipLaunchKernelGGL(diffaug_finalize_kernel, dim3(N), dim3(AUG_BLOCK), 0, (hipStream_t)stream, (const double*)part, 1.0, (float*)nullptr,
                     sum);
  return check_launch("diffaug_finalize_kernel");
}

extern "C" int hrv_diffaug_bwd_f32(const float* g, int32_t g_cstride, int32_t Ca, const float* u, const double* gsum, int32_t policy,
                                   int32_t N, int32_t H, int32_t W, float* d_img, hrv_stream_t stream) {
  HRV_REQUIRE(g && u && d_img && aug_shape_ok(N, H, W) && aug_policy_ok(policy), "diffaug_bwd: bad args");
  HRV_REQUIRE(Ca >= 1 && Ca <= 8 && g_cstride == 12, "diffaug_bwd: serves the PatchGAN shape only (gradient stride 12, C <= 8 + 3)");
  HRV_REQUIRE(((uintptr_t)g & 15) == 0 && (((uintptr_t)u | (uintptr_t)d_img) & 3) == 0 && ((uintptr_t)gsum & 7) == 0,
              "diffaug_bwd: misaligned pointer");
  HRV_REQUIRE(gsum || !(policy & HRV_DIFFAUG_COLOR), "diffaug_bwd: color needs the per-sample gradient sums");
  hipLaunchKernelGGL(diffaug_bwd_kernel<false>, aug_grid_for(H * W, N), dim3(AUG_BLOCK), 0, (hipStream_t)stream, g, (int)Ca, u, gsum, (int)policy, (int)H,
                     (int)W, d_img);
  return check_launch("diffaug_bwd_kernel");
}

static inline bool aug_gate_ok(const float* ug, const double* p) {
  return ug && p && ((uintptr_t)ug & 3) == 0 && ((uintptr_t)p & 7) == 0;
}

extern "C" int hrv_diffaug_concat_gated_f32(const float* a, int32_t Ca, int32_t a_cstride, const float* b, const float* u,
                                            const float* mean, int32_t policy, int32_t N, int32_t H, int32_t W, float* out,
                                            int32_t out_cstride, const float* ug, const double* p, hrv_stream_t stream) {
  HRV_REQUIRE(a && b && u && out && aug_shape_ok(N, H, W) && aug_policy_ok(policy), "diffaug_concat_gated: bad args");
  HRV_REQUIRE(Ca >= 1 && Ca <= 8 && a_cstride == 8 && out_cstride == 12,
              "diffaug_concat_gated: serves the PatchGAN shape only (parse stride 8 with C <= 8, 3 image channels, output stride 12)");
  HRV_REQUIRE((((uintptr_t)a | (uintptr_t)out) & 15) == 0 && (((uintptr_t)b | (uintptr_t)u | (uintptr_t)mean) & 3) == 0 &&
                  aug_gate_ok(ug, p),
              "diffaug_concat_gated: misaligned or missing pointer");
  HRV_REQUIRE(mean || !(policy & HRV_DIFFAUG_COLOR), "diffaug_concat_gated: color needs the per-sample means");
  hipLaunchKernelGGL((diffaug_concat_kernel<true, const float*, const double*>), aug_grid_for(H * W, N), dim3(AUG_BLOCK), 0, (hipStream_t)stream, a, (int)Ca, b, u, mean,
                     (int)policy, (int)H, (int)W, out, ug, p);
  return check_launch("diffaug_concat_kernel<gated>");
}

extern "C" int hrv_diffaug_gsum_gated_f32(const float* g, int32_t g_cstride, int32_t Ca, const float* u, int32_t policy, int32_t N,
                                          int32_t H, int32_t W, double* part, double* sum, const float* ug, const double* p,
                                          hrv_stream_t stream) {
  HRV_REQUIRE(g && u && part && sum && aug_shape_ok(N, H, W) && aug_policy_ok(policy), "diffaug_gsum_gated: bad args");
  HRV_REQUIRE(Ca >= 1 && Ca <= 8 && g_cstride == 12, "diffaug_gsum_gated: serves the PatchGAN shape only (gradient stride 12, C <= 8 + 3)");
  HRV_REQUIRE(((uintptr_t)g & 15) == 0 && ((uintptr_t)u & 3) == 0 && (((uintptr_t)part | (uintptr_t)sum) & 7) == 0 && aug_gate_ok(ug, p),
              "diffaug_gsum_gated: misaligned or missing pointer");
  hipLaunchKernelGGL((diffaug_gsum_kernel<true, const float*, const double*>), dim3(AUG_SLOTS, N), dim3(AUG_BLOCK), 0, (hipStream_t)stream, g, (int)Ca, u, (int)policy,
                     (int)H, (int)W, part, ug, p);
  int rc = check_launch("diffaug_gsum_kernel<gated>");
  if (rc != HRV_OK) return rc;
  hipLaunchKernelGGL(diffaug_finalize_kernel, dim3(N), dim3(AUG_BLOCK), 0, (hipStream_t)stream, (const double*)part, 1.0, (float*)nullptr,
                     sum);
  return check_launch("diffaug_finalize_kernel");
}

extern "C" int hrv_diffaug_bwd_gated_f32(const float* g, int32_t g_cstride, int32_t Ca, const float* u, const double* gsum, int32_t policy,
                                         int32_t N, int32_t H, int32_t W, float* d_img, const float* ug, const double* p,
                                         hrv_stream_t stream) {
  HRV_REQUIRE(g && u && d_img && aug_shape_ok(N, H, W) && aug_policy_ok(policy), "diffaug_bwd_gated: bad args");
  HRV_REQUIRE(Ca >= 1 && Ca <= 8 && g_cstride == 12, "diffaug_bwd_gated: serves the PatchGAN shape only (gradient stride 12, C <= 8 + 3)");
  HRV_REQUIRE(((uintptr_t)g & 15) == 0 && (((uintptr_t)u | (uintptr_t)d_img) & 3) == 0 && ((uintptr_t)gsum & 7) == 0 && aug_gate_ok(ug, p),
              "diffaug_bwd_gated: misaligned or missing pointer");
  HRV_REQUIRE(gsum || !(policy & HRV_DIFFAUG_COLOR), "diffaug_bwd_gated: color needs the per-sample gradient sums");
  hipLaunchKernelGGL((diffaug_bwd_kernel<true, const float*, const double*>), aug_grid_for(H * W, N), dim3(AUG_BLOCK), 0, (hipStream_t)stream, g, (int)Ca, u, gsum,
                     (int)policy, (int)H, (int)W, d_img, ug, p);
  return check_launch("diffaug_bwd_kernel<gated>");
}

extern "C" int hrv_ada_update_f64(const double* dhead_record, int32_t num_d, double target, double step, int32_t interval, double p_max,
                                  double* state, hrv_stream_t stream) {
  HRV_REQUIRE(dhead_record && state && (((uintptr_t)dhead_record | (uintptr_t)state) & 7) == 0, "ada_update: missing or misaligned pointer");
  HRV_REQUIRE(num_d >= 1 && num_d <= HRV_DHEAD_MAX_SCALES && interval >= 1, "ada_update: 1..HRV_DHEAD_MAX_SCALES scales, interval >= 1");
  HRV_REQUIRE(target >= -1.0 && target <= 1.0 && step >= 0.0 && step <= 1.0 && p_max >= 0.0 && p_max <= 1.0,
              "ada_update: target in [-1, 1], step and p_max in [0, 1]");
  hipLaunchKernelGGL(ada_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, dhead_record, (int)num_d, target, step, (int)interval,
                     p_max, state);
  return check_launch("ada_update_kernel");
}
