// The scripts' image grids on gfx950: torchvision make_grid over up to 16 panels (fp32 views of any stride), the reference's
// t/2 + 0.5, visualize_segmap (argmax + palette) and the float -> uint8 conversion, N grids in ONE launch that reads every source
// element once and writes uint8 [N,Hg,Wg,3].  Memory bound: 12 fp32 [3,H,W] panels in, a quarter of the bytes out.
#include "hrv_common.h"

namespace hrv {
namespace {

constexpr int VIZ_THREADS = 256;
constexpr int VIZ_PIX = 4;                                  // pixels per thread
constexpr int VIZ_BLOCK_PIX = VIZ_THREADS * VIZ_PIX;        // 1024 pixels = 3072 bytes = 768 dwords of the flat output per block

struct VizPanels {
  hrv_viz_panel_t p[HRV_VIZ_MAX_PANELS];
};

// utils.visualize_segmap's palette, one r | g << 8 | b << 16 word per class
__constant__ uint32_t kVizPalette[HRV_VIZ_MAX_CLASSES] = {
    0x000000u, 0x000080u, 0x0000feu, 0x005500u, 0x3300a9u, 0x0055feu, 0x550000u, 0xdc7700u, 0x005555u, 0x555500u,
    0x003355u, 0x805634u, 0x008000u, 0xfe0000u, 0xdca933u, 0xfefe00u, 0xa9fe55u, 0x55fea9u, 0x00fefeu, 0x00a9feu};

// (uint8) clamp(v * 255 [+ 0.5], 0, 255), truncating.  The product and the sum are rounded separately (no fused multiply-add):
// torch's mul(255).add_(0.5) is two fp32 operations, and v * 255 lands exactly on k + 0.5 for hundreds of fp32 values v.  hipcc
// contracts __fmul_rn / __fadd_rn like plain operators, so contraction is switched off for this body.
__device__ __forceinline__ uint32_t viz_byte(float v, int quant) {
#pragma clang fp contract(off)
  float t = v * 255.f;
  if (quant == HRV_VIZ_ROUND) t = t + 0.5f;
  t = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
  return (uint32_t)(int)t;
}

__device__ __forceinline__ bool viz_vec4(const hrv_viz_panel_t& p) {
  return p.sc == 1 && ((uintptr_t)p.ptr & 15) == 0 && ((p.sn | p.sy | p.sx) & 3) == 0;
}

// the r | g << 8 | b << 16 word of pixel (n, y, x) of one panel
__device__ __forceinline__ uint32_t viz_pixel(const hrv_viz_panel_t& p, int n, int y, int x, int quant) {
  const float* s = p.ptr + ((int64_t)n * p.sn + (int64_t)y * p.sy + (int64_t)x * p.sx);
  const bool vec = viz_vec4(p);
  if (p.kind == HRV_VIZ_SEGMAP) {
    // first maximum wins: strictly greater replaces (np.argmax; +0.0 == -0.0)
    int best = 0;
    float bv;
    if (vec) {                                   // NHWC: one pixel's channels as float4 groups; the tail group's extra lanes
      f32x4 v = ld4(s);                          // (padding channels) are loaded and never compared
      bv = v[0];
      for (int c = 1; c < p.C; ++c) {
        if ((c & 3) == 0) v = ld4(s + c);
        const float f = v[c & 3];
        if (f > bv) { bv = f; best = c; }
      }
    } else {                                     // NCHW: a plane per channel, consecutive lanes read consecutive x
      bv = s[0];
      for (int c = 1; c < p.C; ++c) {
        const float f = s[(int64_t)c * p.sc];
        if (f > bv) { bv = f; best = c; }
      }
    }
    return kVizPalette[best];
  }
  float r, g, b;
  if (p.C == 1) {
    r = g = b = s[0];
  } else if (vec) {
    const f32x4 v = ld4(s);
    r = v[0]; g = v[1]; b = v[2];
  } else {
    r = s[0]; g = s[p.sc]; b = s[2 * p.sc];
  }
  if (p.kind == HRV_VIZ_SIGNED) {                // x * 0.5 is exact, so fused or not the sum is rounded once: t/2 + 0.5 == (t+1)/2
    r = r * 0.5f + 0.5f; g = g * 0.5f + 0.5f; b = b * 0.5f + 0.5f;
  }
  return viz_byte(r, quant) | (viz_byte(g, quant) << 8) | (viz_byte(b, quant) << 16);
}

// The flat output is a run of 3-byte pixels; a block owns 1024 consecutive ones, which start on a dword whatever the row length
// (3 * 1024 bytes per block).  Pass 1: thread t computes pixels t, t + 256, ... of the block -- consecutive lanes read consecutive x
// of a source plane -- and leaves each as one word in LDS.  Pass 2: thread t assembles dwords t, t + 256, t + 512 of the block's
// 768 from two neighbouring pixel words and stores them: every store of the main path is a whole, lane-consecutive dword.  Only the
// last dword of the whole output can be partial; it is written by bytes.
__global__ __launch_bounds__(VIZ_THREADS) void viz_grid_kernel(const VizPanels pa, int npanels, int xmaps, int pad, int H, int W,
                                                               int Hg, int Wg, uint32_t P, int quant, uint32_t* __restrict__ out) {
  __shared__ hrv_viz_panel_t sp[HRV_VIZ_MAX_PANELS];
  __shared__ uint32_t px[VIZ_BLOCK_PIX];
  const int tid = threadIdx.x;
  if (tid < npanels) sp[tid] = pa.p[tid];
  __syncthreads();
  const uint32_t base = blockIdx.x * (uint32_t)VIZ_BLOCK_PIX;
  const uint32_t plane = (uint32_t)Hg * (uint32_t)Wg;
  const uint32_t ch = (uint32_t)(H + pad), cw = (uint32_t)(W + pad);
#pragma unroll
  for (int j = 0; j < VIZ_PIX; ++j) {
    const int q = j * VIZ_THREADS + tid;
    const uint32_t gidx = base + (uint32_t)q;
    uint32_t v = 0;
    if (gidx < P) {
      const uint32_t n = gidx / plane, r = gidx - n * plane;
      const uint32_t y = r / (uint32_t)Wg, x = r - y * (uint32_t)Wg;
      const uint32_t cy = y / ch, cx = x / cw;
      const int oy = (int)(y - cy * ch) - pad, ox = (int)(x - cx * cw) - pad;
      const uint32_t k = cy * (uint32_t)xmaps + cx;
      // (the bottom / right border lies in cell row ymaps / cell column xmaps: oy < H and ox < W hold there, cx and k do not)
      if (oy >= 0 && ox >= 0 && cx < (uint32_t)xmaps && k < (uint32_t)npanels) v = viz_pixel(sp[k], (int)n, oy, ox, quant);
    }
    px[q] = v;
  }
  __syncthreads();
  const uint64_t total = (uint64_t)P * 3, byte0 = (uint64_t)base * 3;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int d = j * VIZ_THREADS + tid;                     // dword of the block: bytes 4d .. 4d + 3 = pixel q from byte r on
    const int q = (4 * d) / 3, r = 4 * d - 3 * q;            // q + 1 <= 1023
    const uint32_t v = (px[q] >> (8 * r)) | (px[q + 1] << (24 - 8 * r));
    const uint64_t gb = byte0 + (uint64_t)(4 * d);
    if (gb + 4 <= total) {
      out[gb >> 2] = v;
    } else {
      for (int b = 0; gb + b < total; ++b) reinterpret_cast<uint8_t*>(out)[gb + b] = (uint8_t)(v >> (8 * b));
    }
  }
}

}  // namespace
}  // namespace hrv

using namespace hrv;

extern "C" int hrv_viz_grid_u8(const hrv_viz_panel_t* panels, int32_t npanels, int32_t nrow, int32_t padding, int32_t N, int32_t H,
                               int32_t W, int32_t quant, uint8_t* out, hrv_stream_t stream) {
  HRV_REQUIRE(panels && out && N > 0 && H > 0 && W > 0, "viz_grid: bad args");
  HRV_REQUIRE(npanels >= 1 && npanels <= HRV_VIZ_MAX_PANELS, "viz_grid: %d panels (1 .. %d)", npanels, HRV_VIZ_MAX_PANELS);
  HRV_REQUIRE(nrow >= 1 && padding >= 0 && padding <= 64, "viz_grid: nrow %d, padding %d", nrow, padding);
  HRV_REQUIRE(quant == HRV_VIZ_ROUND || quant == HRV_VIZ_TRUNC, "viz_grid: quant %d", quant);
  HRV_REQUIRE(((uintptr_t)out & 3) == 0, "viz_grid: out must be 4-byte aligned");
  VizPanels pa;
  for (int k = 0; k < HRV_VIZ_MAX_PANELS; ++k) pa.p[k] = panels[k < npanels ? k : 0];
  for (int k = 0; k < npanels; ++k) {
    const hrv_viz_panel_t& p = panels[k];
    HRV_REQUIRE(p.ptr && ((uintptr_t)p.ptr & 3) == 0, "viz_grid: panel %d: null or misaligned pointer", k);
    HRV_REQUIRE(p.sn >= 0 && p.sy >= 0 && p.sx >= 0 && p.sc >= 0, "viz_grid: panel %d: negative stride", k);
    if (p.kind == HRV_VIZ_SEGMAP)
      HRV_REQUIRE(p.C >= 1 && p.C <= HRV_VIZ_MAX_CLASSES, "viz_grid: panel %d: SEGMAP over %d channels (1 .. %d)", k, p.C, HRV_VIZ_MAX_CLASSES);
    else
      HRV_REQUIRE((p.kind == HRV_VIZ_SIGNED || p.kind == HRV_VIZ_UNIT) && (p.C == 1 || p.C == 3),
                  "viz_grid: panel %d: kind %d with %d channels (SIGNED / UNIT take 1 or 3)", k, p.kind, p.C);
  }
  // torchvision make_grid: a single image is returned as it is, without a border
  const int pad = npanels == 1 ? 0 : padding;
  const int xmaps = npanels < nrow ? npanels : nrow;
  const int ymaps = (npanels + xmaps - 1) / xmaps;
  const int64_t Hg = (int64_t)ymaps * (H + pad) + pad, Wg = (int64_t)xmaps * (W + pad) + pad;
  const int64_t P = (int64_t)N * Hg * Wg;
  HRV_REQUIRE(Hg < (1 << 24) && Wg < (1 << 24) && P < ((int64_t)1 << 31), "viz_grid: %d grids of %lld x %lld pixels are too large",
              N, (long long)Hg, (long long)Wg);
  const unsigned blocks = (unsigned)((P + VIZ_BLOCK_PIX - 1) / VIZ_BLOCK_PIX);
  hipLaunchKernelGGL(viz_grid_kernel, dim3(blocks), dim3(VIZ_THREADS), 0, (hipStream_t)stream, pa, npanels, xmaps, pad, H, W, (int)Hg,
                     (int)Wg, (uint32_t)P, quant, reinterpret_cast<uint32_t*>(out));
  return check_launch("viz_grid_kernel");
}
