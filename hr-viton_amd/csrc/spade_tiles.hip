// Tile classification for the fused SPADE forward (spade_fused.hip): the modulation gamma|beta = conv(ReLU(conv_shared(seg)))
// depends on the label map alone, and over a 16x16-pixel tile whose 20x20 label patch (tile + the 2-pixel halo of the two stacked
// 3x3s) lies inside the image and carries one one-hot vector it is a constant.  Such a tile needs the epilogue only.  Two launches
// per (label map, level): classify every tile, then ONE block turns the classes into the two lists in ascending tile order (a
// fixed-order scan: the lists do not depend on the arrival order of anything).  Layout of the plan: spade_tiles.h.
#include "patch_pass.h"
#include "spade_tiles.h"

namespace hrv {

struct StParams {
  const uint4* seg;        // bf16 [N][seg_H][seg_W][8]
  int seg_H, seg_W, seg_shift;
  int N, H, W, m_tiles;
  int* plan;
};

// one wave per tile: the label pixels the fused kernel would read for it, (y << seg_shift, x << seg_shift)
__global__ __launch_bounds__(256) void spade_tiles_classify_kernel(const StParams p) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= p.m_tiles) return;
  const PatchTile T = patch_tile_at(t, p.W, p.H);
  int cls = -1;
  // the 20 x 20 patch wholly inside the level image (a partial tile fails this as well)
  if (T.y0 >= 2 && T.x0 >= 2 && T.y0 + 18 <= p.H && T.x0 + 18 <= p.W) {
    const uint4* const img = p.seg + (size_t)T.n * p.seg_H * p.seg_W;
    auto pixel = [&](const int j, const int i) {
      return img[(size_t)((T.y0 - 2 + j) << p.seg_shift) * p.seg_W + ((T.x0 - 2 + i) << p.seg_shift)];
    };
    const uint4 ref = pixel(0, 0);
    bool same = true;
    for (int q = lane; q < 400; q += 64) {
      const int j = q / 20, i = q - 20 * j;
      const uint4 v = pixel(j, i);
      same = same && v.x == ref.x && v.y == ref.y && v.z == ref.z && v.w == ref.w;
    }
    if (__all(same)) {
      // exactly one channel = bf16 1.0 (0x3F80), every other bit 0
      const unsigned w[4] = {ref.x, ref.y, ref.z, ref.w};
      int ones = 0, k = -1;
      bool clean = true;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned h = (w[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
        if (h == 0x3F80u) { ++ones; k = e; }
        else if (h != 0u) clean = false;
      }
      if (clean && ones == 1) cls = k;
    }
  }
  if (lane == 0) p.plan[ST_HDR + 2 * p.m_tiles + t] = cls;
}

// one block: thread i owns the tiles [i * chunk, (i + 1) * chunk)
__global__ __launch_bounds__(1024) void spade_tiles_lists_kernel(int* const plan, const int m) {
  __shared__ int rep[8];
  __shared__ int scan[1024];
  const int tid = threadIdx.x;
  const int* const cls = plan + ST_HDR + 2 * m;
  int* const heavy = plan + ST_HDR;
  int* const light = plan + ST_HDR + m;
  const int chunk = (m + 1023) / 1024;
  const int t0 = tid * chunk < m ? tid * chunk : m, t1 = t0 + chunk < m ? t0 + chunk : m;
  if (tid < 8) rep[tid] = 0x7FFFFFFF;
  __syncthreads();
  for (int t = t0; t < t1; ++t)
    if (cls[t] >= 0) atomicMin(&rep[cls[t]], t);          // (a minimum: the same whatever the order)
  __syncthreads();
  int nh = 0;
  for (int t = t0; t < t1; ++t) nh += (cls[t] < 0 || rep[cls[t]] == t) ? 1 : 0;
  scan[tid] = nh;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = tid >= d ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  int ih = scan[tid] - nh;             // heavy tiles in front of t0
  int il = t0 - ih;                    // light tiles in front of t0
  for (int t = t0; t < t1; ++t) {
    const int k = cls[t];
    if (k < 0) heavy[ih++] = t;
    else if (rep[k] == t) heavy[ih++] = t | ((k + 1) << 24);
    else light[il++] = t | (k << 24);
  }
  if (tid == 1023) { plan[ST_NHEAVY] = scan[1023]; plan[ST_NLIGHT] = m - scan[1023]; }
  if (tid < 8) plan[ST_REP + tid] = rep[tid] == 0x7FFFFFFF ? -1 : rep[tid];
}

}  // namespace hrv

using namespace hrv;

extern "C" int64_t hrv_spade_tiles_plan_bytes(int32_t N, int32_t H, int32_t W) {
  if (N <= 0 || H <= 0 || W <= 0) return -1;
  const int64_t m = patch_tiles(N, H, W);
  if (m >= ST_MAX_TILES) return -1;
  return (ST_HDR + 3 * m) * 4;
}

extern "C" int hrv_spade_tiles_bf16(const void* seg, int32_t seg_H, int32_t seg_W, int32_t seg_shift, int32_t N, int32_t H, int32_t W,
                                    void* plan, hrv_stream_t stream) {
  HRV_REQUIRE(seg && plan && (((uintptr_t)seg & 15) == 0) && (((uintptr_t)plan & 3) == 0), "spade_tiles: null or misaligned pointer");
  HRV_REQUIRE(N > 0 && H > 0 && W > 0 && patch_tiles(N, H, W) < ST_MAX_TILES, "spade_tiles: bad extent");
  HRV_REQUIRE(seg_shift >= 0 && seg_shift < 16 && seg_H == (H << seg_shift) && seg_W == (W << seg_shift),
              "spade_tiles: the label map must be [N, H << shift, W << shift, 8] bf16 (got %d x %d for %d x %d, shift %d)", seg_H, seg_W, H, W,
              seg_shift);
  StParams p;
  p.seg = (const uint4*)seg; p.seg_H = seg_H; p.seg_W = seg_W; p.seg_shift = seg_shift;
  p.N = N; p.H = H; p.W = W; p.m_tiles = (int)patch_tiles(N, H, W);
  p.plan = (int*)plan;
  hipLaunchKernelGGL(spade_tiles_classify_kernel, dim3((unsigned)((p.m_tiles + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
  hipLaunchKernelGGL(spade_tiles_lists_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, p.plan, p.m_tiles);
  return check_launch("spade_tiles");
}
