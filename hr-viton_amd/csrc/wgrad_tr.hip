// Weight gradient of a stride-1 'same' convolution whose operands are STORED in bf16 (mixed-precision training:
// dY = [dgamma|dbeta] / d(conv out), X = actv / a SPADE-modulated activation -- tensors only matrix cores read):
//
//     dW[co][tap][ci] = sum_p dY[p][co] * X[p + tap][ci]            (reference: autograd of nn.Conv2d,
//                                                                     network_generator.py:98-99,117-121,141-143)
//
// The bf16 MFMA wants 8 consecutive k (= PIXELS here) per lane, but NHWC is pixel-major.  conv_wgrad_bf16_kernel
// (conv_bwd.hip) transposes quads in registers: 26 VALU instructions per MFMA, MFMA-busy 13 %
// (profiles/r01_pmc_wgrad_bf16.txt).  This kernel has NO VALU in the staging path:
//   * both operands travel global -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds) in their natural [pixel][channel]
//     order: a tile is one image-row segment of 64 pixels, so dY is ONE contiguous run and X (with its KW-1 halo
//     pixels) another; 3-4 stages in flight with counted vmcnt across a fence-less s_barrier;
//   * fragments are read with transposing LDS reads: 16 lanes fetch a [4 pixels][16 channels] block and receive it
//     transposed -- lane j holds channel j's 4 pixels, i.e. half an MFMA operand.  Every lane passes its own address,
//     so a tap is just a pixel offset into the X patch (no im2col, no per-tap restaging);
//   * a block owns a (cout tile) x (one kernel row: KW taps x 32*XC input channels) tile of dW and keeps it in
//     registers (TM x TN x 16 accumulators per lane) while it streams its slab of the image; the kernel rows /
//     cout tiles of one slab are neighbouring blocks of one XCD (they re-read the same dY rows out of L2).
// LDS rows are padded to (4 mod 8) 16-byte slots so the four pixel rows of a transposing read fall into the four
// 64-byte bank quarters (pad slots are DMA'd as zeros by out-of-range offsets).
// Partial sums go to the same [S][tap][Cout][CinTot] workspace as the other weight-gradient kernels (fixed-order
// reduce => deterministic).
// The streaming loop, the stage geometry, the epilogue and the host's slab rule are wgrad_lds_dma.h (shared with wgrad_s2.hip);
// this file owns the stride-1 patch addressing, the (tap, chunk) table, the shape classes and the launch table.
#include "wgrad_lds_dma.h"

namespace hrv {

struct WgradTrParams {
  const void* dy; int dy_cs, dy_co, Cout;
  const void* x; int x_cs, x_co, x_C;       // x_C: channels of this source, multiple of 8
  int N, H, W, KH, KW, pad;
  int CinTot, ci_base, ci_real;
  int co_tiles, col_tiles, S;               // col tile = (kernel row kh, group range)
  int gpt;                                  // 32-channel groups per tap = ceil(x_C / 32)
  int row_mode;                             // 1: a block's column groups are the KW * gpt groups of ONE kernel row (the rest of its
                                            //    WN * TN group slots idle) -- sources whose width is not 128
  int tiles_per_row, n_tiles;               // 64-pixel row segments
  float* ws;
  float* bias_ws;                           // [S][Cout] column sums of dY (bias gradient), or null
};

// TM x 32 couts and TN groups (of 32 (tap, ci) columns) per wave; WM x WN waves; XC = 32-channel chunks of X a block
// stages; PR = image rows of the X patch: 1 (all groups of a block lie in ONE kernel row: the 128-channel sources) or
// KH (a block covers every tap: the thin convolutions of the 1024x768 level, 32..96 channels on either side).
template <int TM, int TN, int WM, int WN, int XC, int PR>
__global__ __launch_bounds__(256) void conv_wgrad_tr_kernel(const WgradTrParams p) {
  static_assert(WM * WN == 4, "4 waves");
  constexpr int RDY = pad_slots(4 * TM * WM, 4);      // 16-byte slots per dY pixel row
  constexpr int RX = pad_slots(4 * XC, 4);        // 16-byte slots per X patch pixel (fragment rows one pixel apart)
  constexpr int TW = 64;                          // pixels per tile
  constexpr int PXMAX = TW + 2;                   // patch pixels (KW <= 3)
  constexpr int NX = (PR * PXMAX * RX + 63) / 64; // X DMA instructions per tile
  typedef WgradStage<RDY, NX> G;
  constexpr int NDYW = G::NDYW, NXW = G::NXW, DYB = G::DYB, STAGE = G::STAGE;
  __shared__ __attribute__((aligned(1024))) unsigned char smem[G::NS * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int g = lane >> 4, i16 = lane & 15, l31 = lane & 31, lh = lane >> 5;

  // logical block id: slab-major, the (cout tile, column tile) jobs of one slab are neighbours on one XCD
  int b = xcd_remap(blockIdx.x, p.co_tiles * p.col_tiles * p.S);
  const int ct = b % p.col_tiles; b /= p.col_tiles;
  const int cot = b % p.co_tiles;
  const int s = b / p.co_tiles;
  const int co0 = cot * (32 * TM * WM);
  constexpr int NGB = WN * TN;                   // column groups of this block
  const int gidx0 = p.row_mode ? ct * p.KW * p.gpt : ct * NGB;   // first global group (tap-major: tap * gpt + chunk)
  const int tap0 = gidx0 / p.gpt;
  const int kh = PR == 1 ? tap0 / p.KW : 0;       // first kernel row of the patch
  const int chunk_lo = (NGB >= p.gpt) ? 0 : gidx0 % p.gpt;   // first 32-channel chunk staged (whole taps: all of them)

  const int t_begin = (int)(((long long)p.n_tiles * s) / p.S);
  const int t_end = (int)(((long long)p.n_tiles * (s + 1)) / p.S);

  // ---- DMA lane constants.  The buffer resources are based at the first image row of this block's slab (64-bit
  // pointer arithmetic once per block), so the per-tile scalar offsets stay small whatever the tensor size (the
  // 384-channel actv tensor of up_4 is 2.4 GB).
  const int r_base = t_begin / p.tiles_per_row;                    // global row index n*H + y of the slab's first tile
  const rsrc_t dy_rsrc = wgrad_rsrc((const char*)p.dy + ((long long)r_base * p.W * p.dy_cs + p.dy_co + co0) * 2);
  // X base shifted back by `pad` rows and `pad` pixels: patch pixel 0 of a tile is image column x0 - pad, its row may
  // be row - pad (both masked when outside the image; the address is never dereferenced then)
  const rsrc_t x_rsrc = wgrad_rsrc((const char*)p.x + (((long long)(r_base - p.pad) * p.W - p.pad) * p.x_cs + p.x_co + chunk_lo * 32) * 2);
  unsigned dy_voff[NDYW];
  int dy_p[NDYW];
#pragma unroll
  for (int q = 0; q < NDYW; ++q) {
    const int slot = 64 * (wave + 4 * q) + lane;
    const int pp = slot / RDY, sl = slot - pp * RDY;
    const bool ok = sl < 4 * TM * WM && co0 + 8 * sl < p.Cout;
    dy_p[q] = ok ? pp : 1 << 20;                                   // pixel of the tile (>= any width: never valid)
    dy_voff[q] = (unsigned)((pp * p.dy_cs + 8 * sl) * 2);
  }
  unsigned x_voff[NXW];
  int x_p[NXW], x_row[NXW];
  const int px_used = TW + p.KW - 1;
#pragma unroll
  for (int q = 0; q < NXW; ++q) {
    int j = wave + 4 * q;
    j = j < NX ? j : NX - 1;
    const int slot = 64 * j + lane;
    const int pq = slot / RX, sl = slot - pq * RX;                  // patch pixel (row-major over PR rows), slot
    const int prow = pq / PXMAX, pp = pq - prow * PXMAX;
    const bool ok = prow < PR && pp < px_used && sl < 4 * XC && (chunk_lo * 32 + 8 * sl) < p.x_C;
    x_p[q] = ok ? pp : 1 << 20;
    x_row[q] = prow < PR ? prow : 0;
    x_voff[q] = (unsigned)(((prow * p.W + pp) * p.x_cs + 8 * sl) * 2);
  }

  // ---- fragment lane constants (bytes inside a stage)
  //  a (dY): pixel 8*(g>>1) + (i16>>2) (+4 for the second read, +16 per k-step), channels wm*TM*32 + 16*(g&1) + 4*(i16&3) (+32 per tm)
  const int a_base = (8 * (g >> 1) + (i16 >> 2)) * (RDY * 16) + (wm * TM * 32 + 16 * (g & 1) + 4 * (i16 & 3)) * 2;
  int b_base[TN], b_tap[TN], b_chunk[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int gi = gidx0 + wn * TN + j;
    int tap = gi / p.gpt, chunk = gi - tap * p.gpt;
    if (p.row_mode && wn * TN + j >= p.KW * p.gpt) tap = p.KH * p.KW;   // an idle slot of a row-aligned block
    // groups past the last tap (and idle slots) are computed on the first staged tap / chunk and dropped
    const bool live = tap < p.KH * p.KW;
    const int tc = live ? tap : kh * p.KW;
    if (!live) chunk = chunk_lo;
    const int khj = tc / p.KW, kw = tc - khj * p.KW;
    b_tap[j] = tap; b_chunk[j] = chunk;
    b_base[j] = DYB + ((khj - kh) * PXMAX + 8 * (g >> 1) + (i16 >> 2) + kw) * (RX * 16) +
                ((chunk - chunk_lo) * 32 + 16 * (g & 1) + 4 * (i16 & 3)) * 2;
  }

  // Bias gradient: the TM cout tiles of a slab are spread over the 4 waves of its kernel-row blocks (wave w of the kh block takes
  // tile kh*4 + w), so no wave carries more than one extra MFMA per 15.
  const int bias_i = (p.bias_ws != nullptr && ct < 3) ? ct * 4 + wave : -1;      // wave-uniform

  // tile t -> (image row r = n*H + y, segment xt)
  auto issue = [&](int t, int buf) {
    const int r = t / p.tiles_per_row, xt = t - r * p.tiles_per_row;
    const int x0 = xt * TW;
    const int n = r / p.H, y = r - n * p.H;
    unsigned char* sb = smem + buf * STAGE;
    {
      const unsigned soff = (unsigned)(((r - r_base) * p.W + x0) * p.dy_cs * 2);
      const int lim = p.W - x0;                                    // valid pixels of this segment
#pragma unroll
      for (int q = 0; q < NDYW; ++q)
        dma16(dy_rsrc, sb + (wave + 4 * q) * 1024, dy_p[q] < lim ? dy_voff[q] : 0xFFFFFFF0u, soff);
    }
    {
      // patch row `prow` is image row y + kh + prow - pad of this sample; the scalar offset points at patch row 0
      // (never negative: the resource base sits `pad` rows before the slab), invalid rows / columns are masked per lane
      unsigned rowmask = 0;
#pragma unroll
      for (int pr = 0; pr < PR; ++pr) rowmask |= ((unsigned)(y + kh + pr - p.pad) < (unsigned)p.H) ? (1u << pr) : 0u;
      const unsigned soff = (unsigned)(((r + kh - r_base) * p.W + x0) * p.x_cs * 2);
      const int lo = p.pad - x0, hi = p.W - x0 + p.pad;            // patch pixel pp is image column x0 - pad + pp
#pragma unroll
      for (int q = 0; q < NXW; ++q) {
        int j = wave + 4 * q;
        j = j < NX ? j : NX - 1;
        const bool ok = ((rowmask >> x_row[q]) & 1u) && x_p[q] >= lo && x_p[q] < hi;
        dma16(x_rsrc, sb + DYB + j * 1024, ok ? x_voff[q] : 0xFFFFFFF0u, soff);
      }
    }
  };

  // fragment rows one pixel apart: +16 pixels per k-step, +4 for the high half, on either operand
  f32x16 acc[TM][TN], acc_b;
  WGRAD_STREAM(TM, TN, G, 16 * RDY * 16, 4 * RDY * 16, 16 * RX * 16, 4 * RX * 16, smem, issue, a_base, b_base, l31, bias_i, t_begin, t_end, acc, acc_b)
  const int taps = p.KH * p.KW;
  WGRAD_STORE(TM, TN, p, s, co0, taps, l31, lh, bias_i, acc_b, acc, b_chunk, wm * TM + i, b_tap[j], b_tap[j] < taps)
}

// The shape class (0..8) that serves this weight gradient, or -1: EVERY condition on the shape behind the route's front conditions
// (wgrad_route, conv_bwd.hip: bf16 storage, no resampling, stride 1, Ho == H, Wo == W), the environment switches and the slab-extent
// limit included.  Fills `pl`.
int wgrad_tr_class(const hrv_conv2d_wgrad_t& d, WgradLdsPlan& pl) {
  const int Cout = d.Cout, x_C = d.x_C, N = d.N, H = d.H, W = d.W, KH = d.KH, KW = d.KW;
  const char* env = hrv::env("HRV_WGRAD_TR");
  if (env && env[0] == '0') return -1;
  if (KW < 1 || KW > 3 || KH != KW || d.pad != KH / 2) return -1;
  if (Cout < 1 || x_C < 1 || N < 1 || H < 1 || W < 1) return -1;
  if ((d.dy_cstride | d.dy_coff | d.x_cstride | d.x_coff | x_C) & 7) return -1;  // 16-byte DMA granules (Cout itself may be
                                                                                  // anything: rows >= Cout are never written)
  const long long P = (long long)N * H * W;
  // low-resolution levels: weight-bound, old kernel.  HRV_WGRAD_TR_MIN_PIX: the smallest N*H*W this kernel takes -- 8192 since round 5
  // (the 64 x 48 level at 4 images: three same-box pairs of the whole iteration, each 0.16-0.27 ms in favour,
  // profiles/r05_ab_wgrad_tr_min.txt); 32768 before
  const char* emin = hrv::env("HRV_WGRAD_TR_MIN_PIX");
  const long long pmin = emin ? atoll(emin) : 8192;
  if (P < (pmin > 0 ? pmin : 8192) || W < 32) return -1;
  const int gpt = (x_C + 31) / 32;
  const int taps = KH * KW;
  pl.gpt = gpt;
  pl.tiles_per_row = (W + 63) / 64;
  pl.n_tiles = N * H * pl.tiles_per_row;
  // shape classes:  0 = 128-channel source, a block = the KW taps of one kernel row x all 128 channels x <= 160 couts
  //                 1..3 = thin layers (<= 32 couts, <= 96 source channels): a block = every tap x every channel
  //                 4..7 = other source widths (round 4): 4: 144 / 160 channels (5 groups), 6: 272 / 288 (9), 7: 256 (8) -- a block =
  //                        the KW taps of one kernel row x all groups x 64 couts (row mode); 5: 64 channels x 64 couts, every tap
  int cls = -1, tm = 0;
  pl.row_mode = 0;
  if (gpt == 4 && KW == 3) {
    cls = 0;
    pl.co_tiles = (Cout + 159) / 160;
    tm = (((Cout + pl.co_tiles - 1) / pl.co_tiles) + 31) / 32;                   // 1..5
    pl.col_tiles = KH * KW * gpt / 12;                                             // WN 4 x TN 3 groups per block
  } else if (KW == 3 && Cout % 64 == 0 && (gpt == 5 || gpt == 9 || gpt == 8)) {
    cls = gpt == 5 ? 4 : (gpt == 9 ? 6 : 7);
    pl.row_mode = 1;
    pl.co_tiles = Cout / 64; tm = 2;
    pl.col_tiles = KH;
  } else if (KW == 3 && Cout % 64 == 0 && gpt == 2) {
    cls = 5;
    pl.co_tiles = Cout / 64; tm = 2;
    pl.col_tiles = 1;
  } else if (KW == 2 && Cout % 64 == 0 && gpt == 2) {
    cls = 8;      // 2x2 over <= 64 channels (round 6: PatchGAN's model0 over its space-to-depth image, conv_s2.hip mode 2)
    pl.co_tiles = Cout / 64; tm = 2;
    pl.col_tiles = 1;
  } else if (Cout <= 32 && taps * gpt <= 28 && gpt <= 3) {
    cls = gpt == 3 ? (taps == 1 ? 3 : 1) : (gpt == 1 && taps == 9 ? 2 : -1);
    pl.co_tiles = 1; pl.col_tiles = 1; tm = 1;
  }
  if (cls < 0 || tm < 1 || tm > 5) return -1;
  // both operands are addressed from the slab's first row: either's extent is the slab's rows + 4 + KH
  if (!wgrad_slabs(pl.co_tiles * pl.col_tiles, pl.n_tiles, pl.tiles_per_row, 4 + KH, (long long)W * d.dy_cstride * 2, 4 + KH,
                   (long long)W * d.x_cstride * 2, pl.S))
    return -1;
  pl.cls = cls; pl.tm = tm;
  return cls;
}

// Host side: launches the instance of class `pl` (from wgrad_tr_class over this `d`); the partials of pl.S slabs are left in
// d.workspace, the bias column sums ([S][Cout]) right behind them, for the caller's wgrad_reduce_kernel launch.  HRV_OK or < 0.
int wgrad_tr_try(const hrv_conv2d_wgrad_t& d, const WgradLdsPlan& pl, hipStream_t st) {
  WgradTrParams p;
  p.dy = d.dy; p.dy_cs = d.dy_cstride; p.dy_co = d.dy_coff; p.Cout = d.Cout;
  p.x = d.x; p.x_cs = d.x_cstride; p.x_co = d.x_coff; p.x_C = d.x_C;
  p.N = d.N; p.H = d.H; p.W = d.W; p.KH = d.KH; p.KW = d.KW; p.pad = d.pad;
  p.CinTot = d.CinTot; p.ci_base = d.ci_base; p.ci_real = d.x_C_real;
  p.co_tiles = pl.co_tiles; p.col_tiles = pl.col_tiles; p.S = pl.S;
  p.gpt = pl.gpt; p.row_mode = pl.row_mode;
  p.tiles_per_row = pl.tiles_per_row; p.n_tiles = pl.n_tiles;
  p.ws = d.workspace;
  if (int rc = wgrad_workspace("wgrad_tr", pl.S, d.KH * d.KW, d.Cout, d.CinTot, d.workspace, d.workspace_bytes, d.dbias != nullptr, p.bias_ws))
    return rc;
  const int nblk = p.co_tiles * p.col_tiles * pl.S;
  const int cls = pl.cls;
  if (cls == 0) {
    switch (pl.tm) {
      case 1: hipLaunchKernelGGL((conv_wgrad_tr_kernel<1, 3, 1, 4, 4, 1>), dim3(nblk), dim3(256), 0, st, p); break;
      case 2: hipLaunchKernelGGL((conv_wgrad_tr_kernel<2, 3, 1, 4, 4, 1>), dim3(nblk), dim3(256), 0, st, p); break;
      case 3: hipLaunchKernelGGL((conv_wgrad_tr_kernel<3, 3, 1, 4, 4, 1>), dim3(nblk), dim3(256), 0, st, p); break;
      case 4: hipLaunchKernelGGL((conv_wgrad_tr_kernel<4, 3, 1, 4, 4, 1>), dim3(nblk), dim3(256), 0, st, p); break;
      case 5: hipLaunchKernelGGL((conv_wgrad_tr_kernel<5, 3, 1, 4, 4, 1>), dim3(nblk), dim3(256), 0, st, p); break;
      default:
        set_error("wgrad_tr: no instance for %d cout tiles per wave", pl.tm);
        return HRV_ERR_ARG;
    }
  } else if (cls == 4) {      // 3x3 over 144 / 160 channels: 15 groups per kernel row -> 4 waves x 4
    hipLaunchKernelGGL((conv_wgrad_tr_kernel<2, 4, 1, 4, 5, 1>), dim3(nblk), dim3(256), 0, st, p);
  } else if (cls == 5) {      // 3x3 over 64 channels: 18 groups -> 4 waves x 5, every tap in one block
    hipLaunchKernelGGL((conv_wgrad_tr_kernel<2, 5, 1, 4, 2, 3>), dim3(nblk), dim3(256), 0, st, p);
  } else if (cls == 6) {      // 3x3 over 272 / 288 channels: 27 groups per kernel row -> 4 waves x 7
    hipLaunchKernelGGL((conv_wgrad_tr_kernel<2, 7, 1, 4, 9, 1>), dim3(nblk), dim3(256), 0, st, p);
  } else if (cls == 7) {      // 3x3 over 256 channels: 24 groups per kernel row -> 4 waves x 6
    hipLaunchKernelGGL((conv_wgrad_tr_kernel<2, 6, 1, 4, 8, 1>), dim3(nblk), dim3(256), 0, st, p);
  } else if (cls == 8) {      // 2x2 over <= 64 channels: 8 groups -> 4 waves x 2, every tap in one block
    hipLaunchKernelGGL((conv_wgrad_tr_kernel<2, 2, 1, 4, 2, 2>), dim3(nblk), dim3(256), 0, st, p);
  } else if (cls == 1) {      // 3x3 over <= 96 channels: 27 groups -> 4 waves x 7
    hipLaunchKernelGGL((conv_wgrad_tr_kernel<1, 7, 1, 4, 3, 3>), dim3(nblk), dim3(256), 0, st, p);
  } else if (cls == 2) {      // 3x3 over 32 channels: 9 groups -> 4 waves x 3
    hipLaunchKernelGGL((conv_wgrad_tr_kernel<1, 3, 1, 4, 1, 3>), dim3(nblk), dim3(256), 0, st, p);
  } else {                    // 1x1 over <= 96 channels: 3 groups -> 4 waves x 1
    hipLaunchKernelGGL((conv_wgrad_tr_kernel<1, 1, 1, 4, 3, 1>), dim3(nblk), dim3(256), 0, st, p);
  }
  return check_launch("conv_wgrad_tr_kernel");
}

}  // namespace hrv
