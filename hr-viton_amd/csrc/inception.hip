// Inception-v3 pieces of evaluate.py's Inception Score and FID / KID on gfx950 (fp32) that are not convolutions:
//   - the 3x3 pools of the network over NHWC channel slices: max, stride 2, no padding (the stem and the grid reductions
//     Mixed_6a / Mixed_7a, whose pooled branch is written straight into its slice of the block's concatenation), and
//     average, stride 1, padding 1, count_include_pad (the pooled branch of every other Mixed block); the FID variant of the
//     network pools those branches differently: the same average divided by the taps inside the image, and in Mixed_7c a
//     max, stride 1, padding 1;
//   - the FID input: a decoded uint8 image of any size -> fp32 NHWC4 299 x 299 (x / 255, bilinear, 2v - 1) in one pass;
//   - the classifier head: mean over the last feature map (also on its own: the FID feature), fc with bias, softmax.
// The 94 convolutions run on the fp32 conv engine (conv_f32.hip) with BatchNorm folded into scale / shift.
// Every reduction here has a fixed order that does not depend on the batch: the same image gives the same bits on every run
// and in every batch.
#include "hrv_common.h"

namespace hrv {
namespace {

// ---------------------------------------------------------------- 3x3 pools over channel slices
// A work item is one strip of POOL_STRIP output pixels of one output row and one group of 4 channels.  It walks the input
// columns of its strip once: per column three 16-byte loads (the three input rows) reduced vertically, then a sliding window
// of three column values.  Inside a strip every input element is loaded once per output row; the one or two columns two
// neighbouring strips share come from L2.  Channel groups are the fastest index, so a wave reads 1 KB runs.
constexpr int POOL_STRIP = 8;

struct MaxCol {
  float4 v;
  __device__ __forceinline__ void load(const float4* __restrict__ p0, const float4* __restrict__ p1, const float4* __restrict__ p2) {
    const float4 a = *p0, b = *p1, c = *p2;
    v.x = fmaxf(fmaxf(a.x, b.x), c.x); v.y = fmaxf(fmaxf(a.y, b.y), c.y);
    v.z = fmaxf(fmaxf(a.z, b.z), c.z); v.w = fmaxf(fmaxf(a.w, b.w), c.w);
  }
  // the padded pool: a column starts below every value and takes the rows that exist
  __device__ __forceinline__ void lowest() { v = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY); }
  __device__ __forceinline__ void take(const float4* __restrict__ p) {
    const float4 a = *p;
    v.x = fmaxf(v.x, a.x); v.y = fmaxf(v.y, a.y); v.z = fmaxf(v.z, a.z); v.w = fmaxf(v.w, a.w);
  }
  static __device__ __forceinline__ float4 combine(const MaxCol& a, const MaxCol& b, const MaxCol& c) {
    return make_float4(fmaxf(fmaxf(a.v.x, b.v.x), c.v.x), fmaxf(fmaxf(a.v.y, b.v.y), c.v.y),
                       fmaxf(fmaxf(a.v.z, b.v.z), c.v.z), fmaxf(fmaxf(a.v.w, b.v.w), c.v.w));
  }
};

// The average adds in double: nine fp32 values add exactly enough there (one rounding to fp32 at the end), so the result is
// the correctly rounded mean whatever the signs.  The kernel is bound by its loads, not by these 11 double operations.
struct SumCol {
  double x, y, z, w;
  __device__ __forceinline__ void zero() { x = y = z = w = 0.0; }
  __device__ __forceinline__ void add(const float4* __restrict__ p) {
    const float4 a = *p;
    x += (double)a.x; y += (double)a.y; z += (double)a.z; w += (double)a.w;
  }
  static __device__ __forceinline__ float4 combine(const SumCol& a, const SumCol& b, const SumCol& c) {
    return make_float4((float)(((a.x + b.x) + c.x) / 9.0), (float)(((a.y + b.y) + c.y) / 9.0),
                       (float)(((a.z + b.z) + c.z) / 9.0), (float)(((a.w + b.w) + c.w) / 9.0));
  }
  // count_include_pad=False: `taps` of the nine lie inside the image (4, 6 or 9; 1, 2 or 3 per axis in images narrower than 3)
  static __device__ __forceinline__ float4 combine(const SumCol& a, const SumCol& b, const SumCol& c, double taps) {
    return make_float4((float)(((a.x + b.x) + c.x) / taps), (float)(((a.y + b.y) + c.y) / taps),
                       (float)(((a.z + b.z) + c.z) / taps), (float)(((a.w + b.w) + c.w) / taps));
  }
};

struct PoolArgs {
  const float* x; float* y;
  int N, H, W, Ho, Wo, C4, strips;
  int x_cs, x_co, y_cs, y_co;     // in floats
};

// MODE 0: max, stride 2, no padding (every tap is inside the image: 2 * (Ho - 1) + 2 <= H - 1).  MODE 1: average, stride 1, padding 1,
// divided by 9.  MODE 2: that average divided by the taps inside the image.  MODE 3: max, stride 1, padding 1, over the taps inside
// the image (the centre tap always is).
template <int MODE>
__global__ __launch_bounds__(256) void pool3x3_kernel(PoolArgs a) {
  constexpr int ST = MODE == 0 ? 2 : 1, PAD = MODE == 0 ? 0 : 1;
  const int64_t total = (int64_t)a.N * a.Ho * a.strips * a.C4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int64_t t = i;
    const int c = (int)(t % a.C4); t /= a.C4;
    const int sp = (int)(t % a.strips); t /= a.strips;
    const int ho = (int)(t % a.Ho);
    const int n = (int)(t / a.Ho);
    const int wo0 = sp * POOL_STRIP, wo1 = min(wo0 + POOL_STRIP, a.Wo);
    const int hi0 = ho * ST - PAD;
    const int wi0 = wo0 * ST - PAD, wi1 = (wo1 - 1) * ST - PAD + 3;      // input columns [wi0, wi1)
    const float* xin = a.x + (int64_t)n * a.H * a.W * a.x_cs + a.x_co + 4 * c;
    float* yout = a.y + (((int64_t)n * a.Ho + ho) * a.Wo) * a.y_cs + a.y_co + 4 * c;
    if constexpr (MODE == 0) {
      MaxCol p2, p1, cur;
      p2.v = p1.v = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int wi = wi0; wi < wi1; ++wi) {
        const float* q = xin + ((int64_t)hi0 * a.W + wi) * a.x_cs;
        cur.load((const float4*)q, (const float4*)(q + (int64_t)a.W * a.x_cs), (const float4*)(q + 2 * (int64_t)a.W * a.x_cs));
        const int k = wi - wi0 - 2;
        if (k >= 0 && (k & 1) == 0) *(float4*)(yout + (int64_t)(wo0 + (k >> 1)) * a.y_cs) = MaxCol::combine(p2, p1, cur);
        p2 = p1; p1 = cur;
      }
    } else if constexpr (MODE == 3) {
      MaxCol p2, p1, cur;
      p2.lowest(); p1.lowest();
      for (int wi = wi0; wi < wi1; ++wi) {
        cur.lowest();
        if (wi >= 0 && wi < a.W) {
#pragma unroll
          for (int dy = 0; dy < 3; ++dy) {
            const int hi = hi0 + dy;
            if (hi >= 0 && hi < a.H) cur.take((const float4*)(xin + ((int64_t)hi * a.W + wi) * a.x_cs));
          }
        }
        const int k = wi - wi0 - 2;
        if (k >= 0) *(float4*)(yout + (int64_t)(wo0 + k) * a.y_cs) = MaxCol::combine(p2, p1, cur);
        p2 = p1; p1 = cur;
      }
    } else {
      SumCol p2, p1, cur;
      p2.zero(); p1.zero();
      for (int wi = wi0; wi < wi1; ++wi) {
        cur.zero();
        if (wi >= 0 && wi < a.W) {
#pragma unroll
          for (int dy = 0; dy < 3; ++dy) {
            const int hi = hi0 + dy;
            if (hi >= 0 && hi < a.H) cur.add((const float4*)(xin + ((int64_t)hi * a.W + wi) * a.x_cs));
          }
        }
        const int k = wi - wi0 - 2;
        if constexpr (MODE == 1) {
          if (k >= 0) *(float4*)(yout + (int64_t)(wo0 + k) * a.y_cs) = SumCol::combine(p2, p1, cur);
        } else {
          if (k >= 0) {
            const int wo = wo0 + k;      // window columns wo - 1 .. wo + 1, rows hi0 .. hi0 + 2
            const int nw = min(wo + 1, a.W - 1) - max(wo - 1, 0) + 1, nh = min(hi0 + 2, a.H - 1) - max(hi0, 0) + 1;
            *(float4*)(yout + (int64_t)wo * a.y_cs) = SumCol::combine(p2, p1, cur, (double)(nw * nh));
          }
        }
        p2 = p1; p1 = cur;
      }
    }
  }
}

// ---------------------------------------------------------------- classifier head
// pooled[n][c] = (sum over the HW pixels, in pixel order) / HW: a thread per (image, 4 channels)
__global__ __launch_bounds__(256) void incep_mean_kernel(const float* __restrict__ f, int N, int HW, int C4, int cs,
                                                        float4* __restrict__ pooled) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * C4) return;
  const int n = i / C4, c = i - n * C4;
  const float* p = f + (int64_t)n * HW * cs + 4 * c;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k = 0; k < HW; ++k) {
    const float4 v = *(const float4*)(p + (int64_t)k * cs);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const float d = (float)HW;
  pooled[i] = make_float4(s.x / d, s.y / d, s.z / d, s.w / d);
}

// ---------------------------------------------------------------- FID input
// One thread per output pixel: pytorch-fid's F.interpolate(x / 255, (Ho, Wo), mode='bilinear', align_corners=False) followed by
// 2v - 1, from the uint8 image as decoded.  Source coordinate max(0, (o + 0.5) * in / out - 0.5), upper neighbour clamped to the last
// row / column.  The arithmetic is double on the integer pixel values, in the form p + t * (q - p): a constant image comes out
// exactly, and every output is rounded to fp32 once.  (2v - 1 on v = u / 255 is (2u - 255) / 255.)
__global__ __launch_bounds__(256) void fid_prep_u8_kernel(const uint8_t* __restrict__ rgb, int N, int H, int W, int Ho, int Wo,
                                                         float4* __restrict__ out) {
  const int64_t total = (int64_t)N * Ho * Wo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int wo = (int)(i % Wo);
    const int ho = (int)((i / Wo) % Ho);
    const int n = (int)(i / ((int64_t)Wo * Ho));
    const double sy = fmax(0.0, ((double)ho + 0.5) * (double)H / (double)Ho - 0.5);
    const double sx = fmax(0.0, ((double)wo + 0.5) * (double)W / (double)Wo - 0.5);
    const int y0 = min((int)sy, H - 1), x0 = min((int)sx, W - 1);
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const double ty = sy - (double)y0, tx = sx - (double)x0;
    const uint8_t* img = rgb + (int64_t)n * H * W * 3;
    const uint8_t* p00 = img + ((int64_t)y0 * W + x0) * 3;
    const uint8_t* p01 = img + ((int64_t)y0 * W + x1) * 3;
    const uint8_t* p10 = img + ((int64_t)y1 * W + x0) * 3;
    const uint8_t* p11 = img + ((int64_t)y1 * W + x1) * 3;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double a = (double)p00[c], b = (double)p01[c], d = (double)p10[c], e = (double)p11[c];
      const double top = a + tx * (b - a), bot = d + tx * (e - d);
      const double u = top + ty * (bot - top);
      v[c] = (float)((2.0 * u - 255.0) / 255.0);
    }
    out[i] = make_float4(v[0], v[1], v[2], 0.f);
  }
}

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

constexpr int FC_WAVES = 4;      // classes per block (a wave per class)
constexpr int FC_IMGS = 8;       // images whose dot products share one pass over a weight row

// logits[n][k] = sum_c pooled[n][c] * w[k][c] + b[k].  A wave per class: lane l adds channels 4l + 256j (j ascending) with FMAs,
// then the 64 lanes are combined in a butterfly: the order depends on neither the batch size nor the image's place in it.
__global__ __launch_bounds__(64 * FC_WAVES) void incep_fc_kernel(const float* __restrict__ pooled, int N, int C,
                                                                const float* __restrict__ w, const float* __restrict__ b, int K,
                                                                float* __restrict__ logits) {
  const int lane = threadIdx.x & 63, k = blockIdx.x * FC_WAVES + (threadIdx.x >> 6);
  if (k >= K) return;
  const float* wr = w + (int64_t)k * C;
  const float bias = b ? b[k] : 0.f;
  for (int n0 = 0; n0 < N; n0 += FC_IMGS) {
    float acc[FC_IMGS];
#pragma unroll
    for (int j = 0; j < FC_IMGS; ++j) acc[j] = 0.f;
    for (int c = 4 * lane; c < C; c += 256) {
      const float4 wv = *(const float4*)(wr + c);
#pragma unroll
      for (int j = 0; j < FC_IMGS; ++j) {
        if (n0 + j < N) {
          const float4 x = *(const float4*)(pooled + (int64_t)(n0 + j) * C + c);
          acc[j] = fmaf(x.w, wv.w, fmaf(x.z, wv.z, fmaf(x.y, wv.y, fmaf(x.x, wv.x, acc[j]))));
        }
      }
    }
#pragma unroll
    for (int j = 0; j < FC_IMGS; ++j) {
      const float s = wave_sum64(acc[j]);
      if (lane == 0 && n0 + j < N) logits[(int64_t)(n0 + j) * K + k] = s + bias;
    }
  }
}

// probs[n][:] = softmax(logits[n][:]) as torch computes it: exp(x - max) / sum exp(x - max).  One block per image; the maximum and
// the sum are fixed-order trees over the 256 threads' strided partials.
__global__ __launch_bounds__(256) void incep_softmax_kernel(const float* __restrict__ logits, int K, float* __restrict__ probs) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const float* x = logits + (int64_t)blockIdx.x * K;
  float* y = probs + (int64_t)blockIdx.x * K;
  float m = -INFINITY;
  for (int k = tid; k < K; k += 256) m = fmaxf(m, x[k]);
  red[tid] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  m = red[0];
  __syncthreads();
  float sum = 0.f;
  for (int k = tid; k < K; k += 256) sum += expf(x[k] - m);
  red[tid] = sum;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  sum = red[0];
  for (int k = tid; k < K; k += 256) y[k] = expf(x[k] - m) / sum;
}

inline int grid_for(int64_t work) {
  const int64_t g = (work + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

}  // namespace
}  // namespace hrv

using namespace hrv;

extern "C" int hrv_pool3x3_nhwc_f32(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t x_cstride, int32_t x_coff,
                                    int32_t mode, float* y, int32_t y_cstride, int32_t y_coff, hrv_stream_t stream) {
  HRV_REQUIRE(x && y && N > 0 && H > 0 && W > 0 && C > 0, "pool3x3: bad args");
  HRV_REQUIRE(mode >= 0 && mode <= 3,
              "pool3x3: mode %d (0: max stride 2, 1: average stride 1 pad 1, 2: that average over the taps inside, 3: max stride 1 pad 1)",
              mode);
  HRV_REQUIRE(mode != 0 || (H >= 3 && W >= 3), "pool3x3: max-pool input %dx%d is smaller than the window", H, W);
  HRV_REQUIRE(C % 4 == 0 && x_cstride % 4 == 0 && x_coff % 4 == 0 && y_cstride % 4 == 0 && y_coff % 4 == 0 && x_coff >= 0 &&
                  y_coff >= 0 && x_coff + C <= x_cstride && y_coff + C <= y_cstride,
              "pool3x3: channels C=%d, slices (%d of %d, %d of %d) must be multiples of 4 and in range", C, x_coff, x_cstride, y_coff,
              y_cstride);
  HRV_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "pool3x3: 16-byte alignment");
  PoolArgs a;
  a.x = x; a.y = y; a.N = N; a.H = H; a.W = W; a.C4 = C / 4;
  a.Ho = mode == 0 ? (H - 3) / 2 + 1 : H;
  a.Wo = mode == 0 ? (W - 3) / 2 + 1 : W;
  a.strips = (a.Wo + POOL_STRIP - 1) / POOL_STRIP;
  a.x_cs = x_cstride; a.x_co = x_coff; a.y_cs = y_cstride; a.y_co = y_coff;
  const int grid = grid_for((int64_t)N * a.Ho * a.strips * a.C4);
  if (mode == 0) hipLaunchKernelGGL(pool3x3_kernel<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  else if (mode == 1) hipLaunchKernelGGL(pool3x3_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  else if (mode == 2) hipLaunchKernelGGL(pool3x3_kernel<2>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(pool3x3_kernel<3>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("pool3x3_kernel");
}

extern "C" int hrv_fid_prep_u8(const uint8_t* rgb, int32_t N, int32_t H, int32_t W, int32_t Ho, int32_t Wo, float* out,
                               hrv_stream_t stream) {
  HRV_REQUIRE(rgb && out && N > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "fid_prep_u8: bad args");
  HRV_REQUIRE(((uintptr_t)out & 15) == 0, "fid_prep_u8: 16-byte alignment");
  hipLaunchKernelGGL(fid_prep_u8_kernel, dim3(grid_for((int64_t)N * Ho * Wo)), dim3(256), 0, (hipStream_t)stream, rgb, N, H, W, Ho, Wo,
                     (float4*)out);
  return check_launch("fid_prep_u8_kernel");
}

extern "C" int hrv_inception_pool_f32(const float* feat, int32_t N, int32_t HW, int32_t C, int32_t cstride, float* pooled,
                                      hrv_stream_t stream) {
  HRV_REQUIRE(feat && pooled && N > 0 && HW > 0, "inception_pool: bad args");
  HRV_REQUIRE(C > 0 && C % 4 == 0 && cstride % 4 == 0 && cstride >= C, "inception_pool: C=%d cstride=%d must be multiples of 4", C,
              cstride);
  HRV_REQUIRE((((uintptr_t)feat | (uintptr_t)pooled) & 15) == 0, "inception_pool: 16-byte alignment");
  HRV_REQUIRE((int64_t)N * C < ((int64_t)1 << 31), "inception_pool: batch too large");
  hipLaunchKernelGGL(incep_mean_kernel, dim3((N * (C / 4) + 255) / 256), dim3(256), 0, (hipStream_t)stream, feat, N, HW, C / 4,
                     cstride, (float4*)pooled);
  return check_launch("incep_mean_kernel");
}

extern "C" int hrv_inception_head_f32(const float* feat, int32_t N, int32_t HW, int32_t C, int32_t cstride, const float* fc_w,
                                      const float* fc_b, int32_t K, float* pooled, float* logits, float* probs,
                                      hrv_stream_t stream) {
  HRV_REQUIRE(feat && fc_w && pooled && logits && N > 0 && HW > 0 && K > 0, "inception_head: bad args");
  HRV_REQUIRE(C > 0 && C % 4 == 0 && cstride % 4 == 0 && cstride >= C, "inception_head: C=%d cstride=%d must be multiples of 4", C,
              cstride);
  HRV_REQUIRE((((uintptr_t)feat | (uintptr_t)fc_w | (uintptr_t)pooled) & 15) == 0, "inception_head: 16-byte alignment");
  HRV_REQUIRE((int64_t)N * C < ((int64_t)1 << 31) && N <= 65535, "inception_head: batch too large");
  hipLaunchKernelGGL(incep_mean_kernel, dim3((N * (C / 4) + 255) / 256), dim3(256), 0, (hipStream_t)stream, feat, N, HW, C / 4,
                     cstride, (float4*)pooled);
  int rc = check_launch("incep_mean_kernel");
  if (rc != HRV_OK) return rc;
  hipLaunchKernelGGL(incep_fc_kernel, dim3((K + FC_WAVES - 1) / FC_WAVES), dim3(64 * FC_WAVES), 0, (hipStream_t)stream, pooled, N, C,
                     fc_w, fc_b, K, logits);
  rc = check_launch("incep_fc_kernel");
  if (rc != HRV_OK || probs == nullptr) return rc;
  hipLaunchKernelGGL(incep_softmax_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, logits, K, probs);
  return check_launch("incep_softmax_kernel");
}
