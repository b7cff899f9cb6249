// Validation passes of the training scripts on gfx950 (fp32):
//   - the counts behind train_condition.py's iou_metric (:18-36) of a 13-class segmentation map, cloth-mask composition and
//     softmax included, in one launch (integer atomics: the result does not depend on scheduling);
//   - LPIPS's input stage with train_generator.py's Resize((128, 128)) folded in (:482,578): both images of a pair batch are
//     resampled, passed through the ScalingLayer and written as the NHWC4 batch PNetLin.distance_prepped takes, in one launch.
#include "hrv_common.h"

namespace hrv {
namespace {

// ---------------------------------------------------------------- segmentation IoU counts
constexpr int IOU_C = 13;
constexpr int IOU_THREADS = 256;
constexpr int IOU_WAVES = IOU_THREADS / 64;
constexpr int IOU_MAX_BLOCKS_X = 4096;      // a thread then walks HW / (4096 * 256) pixels (1 up to 1024x1024)

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid (pixel blocks, N).  One thread per pixel: the 13 logits, the mask and the 13 labels are plane reads, coalesced across the
// wave.  pred = softmax_c(seg * mask) > 0.5 in the plain fp32 form (subtract the channel maximum, expf, sum in channel order,
// divide), strictly: a probability of exactly 0.5 is not counted.  Counts: wave (shuffle) -> block (LDS) -> one integer atomic add
// per block and counter onto out[n][0..2] = (intersection, sum_pred, sum_true), which the host entry zeroed in-stream.
__global__ __launch_bounds__(IOU_THREADS) void seg_iou_kernel(const float* __restrict__ seg, const float* __restrict__ cm,
                                                              const float* __restrict__ label, int HW, int comp,
                                                              unsigned long long* __restrict__ out) {
  __shared__ int red[IOU_WAVES][3];
  const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* s = seg + (size_t)n * IOU_C * HW;
  const float* l = label + (size_t)n * IOU_C * HW;
  int inter = 0, npred = 0, ntrue = 0;      // <= 13 per pixel, <= HW / gridDim.x / 256 + 1 pixels per thread: fits 32 bits
  for (int64_t p = (int64_t)blockIdx.x * IOU_THREADS + threadIdx.x; p < HW; p += (int64_t)gridDim.x * IOU_THREADS) {
    float v[IOU_C];
#pragma unroll
    for (int c = 0; c < IOU_C; ++c) v[c] = s[(size_t)c * HW + p];
    if (comp != 0) {                        // train_condition.py:344-353: fake_segmap * cloth_mask, ones but for channel 3
      const float m = cm[(size_t)n * HW + p];
      v[3] *= comp == 1 ? (m > 0.5f ? 1.f : 0.f) : m;
    }
    float mx = v[0];
#pragma unroll
    for (int c = 1; c < IOU_C; ++c) mx = fmaxf(mx, v[c]);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < IOU_C; ++c) {
      v[c] = expf(v[c] - mx);
      sum += v[c];
    }
#pragma unroll
    for (int c = 0; c < IOU_C; ++c) {
      const bool pred = v[c] / sum > 0.5f;
      const bool truth = l[(size_t)c * HW + p] == 1.f;
      npred += pred;
      ntrue += truth;
      inter += pred && truth;
    }
  }
  inter = wave_sum_i32(inter);
  npred = wave_sum_i32(npred);
  ntrue = wave_sum_i32(ntrue);
  if (lane == 0) {
    red[wave][0] = inter;
    red[wave][1] = npred;
    red[wave][2] = ntrue;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < IOU_WAVES; ++w) t += (unsigned long long)red[w][threadIdx.x];
    if (t != 0) atomicAdd(out + (size_t)n * 3 + threadIdx.x, t);
  }
}

// ---------------------------------------------------------------- LPIPS input with the resize folded in
struct Scaling {
  float shift[3], scale[3];
};

// One thread per output pixel of the [2N,Ho,Wo,4] batch; images [0, N) come from ``a``, [N, 2N) from ``b`` (fp32 NCHW [N,3,H,W]).
// The values must equal, bit for bit, resize_planes_kernel (glue.hip, bilinear) followed by lpips_prep_f32_kernel (metrics.hip),
// so the roundings are pinned to the ones that pair makes as compiled: the source coordinate is ONE fused multiply-add
// (r * (d + 0.5) - 0.5), each row is fma(1 - lx, left, round(lx * right)), and the two rows are combined with two rounded
// products and one add.  The ScalingLayer is a subtraction and a correctly rounded division.
__global__ __launch_bounds__(256) void lpips_prep_resize_kernel(const float* __restrict__ a, const float* __restrict__ b, int N,
                                                               int H, int W, int Ho, int Wo, float rh, float rw, int normalize,
                                                               Scaling sc, float4* __restrict__ out) {
#pragma clang fp contract(off)
  const size_t total = (size_t)2 * N * Ho * Wo;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int wo = (int)(i % Wo);
    const size_t t = i / Wo;
    const int ho = (int)(t % Ho);
    const int j = (int)(t / Ho);
    const float* src = (j < N ? a + (size_t)j * 3 * H * W : b + (size_t)(j - N) * 3 * H * W);
    float sy = fmaf(rh, (float)ho + 0.5f, -0.5f), sx = fmaf(rw, (float)wo + 0.5f, -0.5f);
    sy = sy < 0.f ? 0.f : sy;
    sx = sx < 0.f ? 0.f : sx;
    int y0 = (int)sy, x0 = (int)sx;
    y0 = y0 < H - 1 ? y0 : H - 1;
    x0 = x0 < W - 1 ? x0 : W - 1;
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    float ly = sy - (float)y0, lx = sx - (float)x0;
    ly = ly < 0.f ? 0.f : (ly > 1.f ? 1.f : ly);
    lx = lx < 0.f ? 0.f : (lx > 1.f ? 1.f : lx);
    const float my = 1.f - ly, mxw = 1.f - lx;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* pl = src + (size_t)c * H * W;
      const float v00 = pl[(size_t)y0 * W + x0], v01 = pl[(size_t)y0 * W + x1];
      const float v10 = pl[(size_t)y1 * W + x0], v11 = pl[(size_t)y1 * W + x1];
      const float r0 = fmaf(mxw, v00, lx * v01), r1 = fmaf(mxw, v10, lx * v11);
      const float q0 = my * r0, q1 = ly * r1;
      float x = q0 + q1;
      if (normalize) x = 2.f * x - 1.f;     // 2x is exact: fused or not, the same bits
      v[c] = (x - sc.shift[c]) / sc.scale[c];
    }
    out[i] = make_float4(v[0], v[1], v[2], 0.f);
  }
}

inline int grid_for(int64_t work) {
  const int64_t g = (work + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

}  // namespace
}  // namespace hrv

using namespace hrv;

extern "C" int hrv_seg_iou_nchw_f32(const float* seg, const float* cm, const float* label, int32_t N, int32_t h, int32_t w,
                                    int32_t comp, int64_t* out, hrv_stream_t stream) {
  HRV_REQUIRE(seg && label && out && N > 0 && h > 0 && w > 0, "seg_iou: bad args");
  HRV_REQUIRE(comp >= 0 && comp <= 2 && (comp == 0 || cm), "seg_iou: comp %d (0 no_composition, 1 detach, 2 warp_grad) needs cm", comp);
  HRV_REQUIRE(N <= 65535 && (int64_t)h * w <= ((int64_t)1 << 30), "seg_iou: batch or map too large");
  const int HW = h * w;
  hipError_t e = hipMemsetAsync(out, 0, (size_t)N * 3 * sizeof(int64_t), (hipStream_t)stream);
  if (e != hipSuccess) {
    set_error("seg_iou: hipMemsetAsync: %s", hipGetErrorString(e));
    return HRV_ERR_LAUNCH;
  }
  int bx = (HW + IOU_THREADS - 1) / IOU_THREADS;
  bx = bx > IOU_MAX_BLOCKS_X ? IOU_MAX_BLOCKS_X : bx;
  hipLaunchKernelGGL(seg_iou_kernel, dim3(bx, N), dim3(IOU_THREADS), 0, (hipStream_t)stream, seg, cm, label, HW, comp,
                     (unsigned long long*)out);
  return check_launch("seg_iou_kernel");
}

extern "C" int hrv_lpips_prep_resize_nchw_f32(const float* in0, const float* in1, int32_t N, int32_t H, int32_t W, int32_t Ho,
                                              int32_t Wo, int32_t normalize, const float* shift3, const float* scale3, float* out,
                                              hrv_stream_t stream) {
  HRV_REQUIRE(in0 && in1 && out && shift3 && scale3 && N > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "lpips_prep_resize: bad args");
  HRV_REQUIRE(((uintptr_t)out & 15) == 0, "lpips_prep_resize: out must be 16-byte aligned");
  Scaling sc;
  for (int c = 0; c < 3; ++c) { sc.shift[c] = shift3[c]; sc.scale[c] = scale3[c]; }
  hipLaunchKernelGGL(lpips_prep_resize_kernel, dim3(grid_for((int64_t)2 * N * Ho * Wo)), dim3(256), 0, (hipStream_t)stream, in0,
                     in1, N, H, W, Ho, Wo, (float)H / (float)Ho, (float)W / (float)Wo, normalize, sc, (float4*)out);
  return check_launch("lpips_prep_resize_kernel");
}
