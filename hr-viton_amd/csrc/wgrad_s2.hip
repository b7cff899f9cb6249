// Weight gradient of PatchGAN's 4x4 stride-2 pad-2 convolution (NLayerDiscriminator, network_generator.py:263-272) over bf16-STORED
// operands, on the streaming skeleton of wgrad_lds_dma.h that it shares with wgrad_tr.hip (LDS-DMA staging in natural
// [pixel][channel] order, transposing fragment reads, a block keeps its tile of dW in registers while it streams a slab of the image):
//
//     dW[co][kh][kw][ci] = sum_{n,oy,ox} dY[n][oy][ox][co] * X[n][2 oy + kh - 2][2 ox + kw - 2][ci]
//
// A tile is one segment of 64 OUTPUT pixels of one dY row; a block owns ONE kernel row kh x (the 4 kw taps x all 32-channel chunks
// of X) x a cout tile.  Its X patch is the single input row 2 oy + kh - 2, pixels 2 x0 - 2 .. 2 x0 + 127 (130 pixels, one
// contiguous run by LDS-DMA); a transposing LDS read takes every lane's own address, so the four k (= output pixel) rows of a
// transposed 4x16 block are simply TWO patch pixels apart and a tap kw is a one-pixel offset: no im2col, no space-to-depth copy.
// X rows are padded to (2 mod 8) 16-byte slots: the four rows of a transposing read, two pixels apart, then start in the four
// 64-byte quarters of the 256-byte bank line (wgrad_tr.hip pads to 4 mod 8 for rows one pixel apart).
// The generic quad-transposing kernel ran these layers at 250-420 TFLOP/s behind a width-padding copy of dY.
// Partial sums go to the [S][tap][Cout][CinTot] workspace of the other weight-gradient kernels (fixed-order reduce).
#include "wgrad_lds_dma.h"

namespace hrv {

struct WgradS2Params {
  const void* dy; int dy_cs, dy_co, Cout;
  const void* x; int x_cs, x_co, x_C;       // x_C: channels of X, multiple of 8
  int N, H, W, Ho, Wo;
  int CinTot, ci_base, ci_real;
  int co_tiles, S;
  int gpt;                                  // 32-channel groups of X = ceil(x_C / 32) (== XC of the instance)
  int tiles_per_row, n_tiles;               // 64-pixel segments of dY rows
  float* ws;
  float* bias_ws;                           // [S][Cout] column sums of dY (bias gradient), or null
};

// TM x 32 couts per block, TN groups per wave over the 4 waves: 4 TN = 4 kw x XC chunks
template <int TM, int TN, int XC>
__global__ __launch_bounds__(256) void conv_wgrad_s2_kernel(const WgradS2Params p) {
  static_assert(4 * TN == 4 * XC, "a block covers the 4 kw taps x XC chunks of one kernel row");
  constexpr int RDY = pad_slots(4 * TM, 4);       // 16-byte slots per dY pixel row (fragment rows one pixel apart)
  constexpr int RX = pad_slots(4 * XC, 2);        // 16-byte slots per X patch pixel (fragment rows two pixels apart)
  constexpr int TW = 64;                          // output pixels per tile
  constexpr int PXMAX = 2 * TW + 2;               // patch pixels: 2 x0 - 2 .. 2 x0 + 127
  constexpr int NX = (PXMAX * RX + 63) / 64;      // X DMA instructions per tile
  typedef WgradStage<RDY, NX> G;
  constexpr int NDYW = G::NDYW, NXW = G::NXW, DYB = G::DYB, STAGE = G::STAGE;
  __shared__ __attribute__((aligned(1024))) unsigned char smem[G::NS * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, i16 = lane & 15, l31 = lane & 31, lh = lane >> 5;

  // logical block id: slab-major, the (cout tile, kernel row) jobs of one slab are neighbours on one XCD
  int b = xcd_remap(blockIdx.x, p.co_tiles * 4 * p.S);
  const int kh = b & 3; b >>= 2;
  const int cot = b % p.co_tiles;
  const int s = b / p.co_tiles;
  const int co0 = cot * (32 * TM);

  const int t_begin = (int)(((long long)p.n_tiles * s) / p.S);
  const int t_end = (int)(((long long)p.n_tiles * (s + 1)) / p.S);

  // ---- DMA lane constants.  The buffer resources are based at the first rows of this block's slab, so the per-tile scalar
  // offsets stay small whatever the tensor size.  X: based two rows and two pixels before input row 2 oy_b of image n_b (never
  // dereferenced outside the image: such lanes are masked)
  const int r_base = t_begin / p.tiles_per_row;                    // dY row index n*Ho + oy of the slab's first tile
  const int n_b = r_base / p.Ho, oy_b = r_base - n_b * p.Ho;
  const long long xrow_b = (long long)n_b * p.H + 2 * oy_b;         // X row index of (n_b, 2 oy_b)
  const rsrc_t dy_rsrc = wgrad_rsrc((const char*)p.dy + ((long long)r_base * p.Wo * p.dy_cs + p.dy_co + co0) * 2);
  const rsrc_t x_rsrc = wgrad_rsrc((const char*)p.x + (((xrow_b - 2) * p.W - 2) * p.x_cs + p.x_co) * 2);
  unsigned dy_voff[NDYW];
  int dy_p[NDYW];
#pragma unroll
  for (int q = 0; q < NDYW; ++q) {
    const int slot = 64 * (wave + 4 * q) + lane;
    const int pp = slot / RDY, sl = slot - pp * RDY;
    const bool ok = sl < 4 * TM && co0 + 8 * sl < p.Cout;
    dy_p[q] = ok ? pp : 1 << 20;                                   // pixel of the tile (>= any width: never valid)
    dy_voff[q] = (unsigned)((pp * p.dy_cs + 8 * sl) * 2);
  }
  unsigned x_voff[NXW];
  int x_p[NXW];
#pragma unroll
  for (int q = 0; q < NXW; ++q) {
    int j = wave + 4 * q;
    j = j < NX ? j : NX - 1;
    const int slot = 64 * j + lane;
    const int pp = slot / RX, sl = slot - pp * RX;                  // patch pixel, slot
    const bool ok = pp < PXMAX && sl < 4 * XC && 8 * sl < p.x_C;
    x_p[q] = ok ? pp : 1 << 20;
    x_voff[q] = (unsigned)((pp * p.x_cs + 8 * sl) * 2);
  }

  // ---- fragment lane constants (bytes inside a stage)
  //  a (dY): pixel 8*(g>>1) + (i16>>2) (+4 for the second read, +16 per k-step), channels 16*(g&1) + 4*(i16&3) (+32 per tm)
  const int a_base = (8 * (g >> 1) + (i16 >> 2)) * (RDY * 16) + (16 * (g & 1) + 4 * (i16 & 3)) * 2;
  //  b (X): group gi = wave*TN + j = kw * XC + chunk; output pixel q -> patch pixel 2 q + kw
  int b_base[TN], b_kw[TN], b_chunk[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int gi = wave * TN + j;
    const int kw = gi / XC, chunk = gi - kw * XC;
    b_kw[j] = kw; b_chunk[j] = chunk;
    b_base[j] = DYB + (2 * (8 * (g >> 1) + (i16 >> 2)) + kw) * (RX * 16) + (chunk * 32 + 16 * (g & 1) + 4 * (i16 & 3)) * 2;
  }

  // Bias gradient: wave w of the kh == 0 block takes cout tile w.
  const int bias_i = (p.bias_ws != nullptr && kh == 0 && wave < TM) ? wave : -1;      // wave-uniform

  // tile t -> (dY row r = n*Ho + oy, segment xt)
  auto issue = [&](int t, int buf) {
    const int r = t / p.tiles_per_row, xt = t - r * p.tiles_per_row;
    const int x0 = xt * TW;
    const int n = r / p.Ho, oy = r - n * p.Ho;
    unsigned char* sb = smem + buf * STAGE;
    {
      const unsigned soff = (unsigned)(((r - r_base) * p.Wo + x0) * p.dy_cs * 2);
      const int lim = p.Wo - x0;                                   // valid pixels of this segment
#pragma unroll
      for (int q = 0; q < NDYW; ++q)
        dma16(dy_rsrc, sb + (wave + 4 * q) * 1024, dy_p[q] < lim ? dy_voff[q] : 0xFFFFFFF0u, soff);
    }
    {
      // the patch is input row iy = 2 oy + kh - 2 of sample n, pixels 2 x0 - 2 + pp; relative to the resource base (row xrow_b - 2,
      // pixel -2) that is row (n H + 2 oy - xrow_b) + kh, pixel 2 x0 + pp -- never negative
      const int iy = 2 * oy + kh - 2;
      const bool row_ok = (unsigned)iy < (unsigned)p.H;
      const long long rel = ((long long)n * p.H + 2 * oy - xrow_b + kh) * p.W + 2 * x0;
      const unsigned soff = (unsigned)(rel * p.x_cs * 2);
      const int lo = 2 - 2 * x0, hi = p.W - 2 * x0 + 2;             // patch pixel pp is image column 2 x0 - 2 + pp
#pragma unroll
      for (int q = 0; q < NXW; ++q) {
        int j = wave + 4 * q;
        j = j < NX ? j : NX - 1;
        const bool ok = row_ok && x_p[q] >= lo && x_p[q] < hi;
        dma16(x_rsrc, sb + DYB + j * 1024, ok ? x_voff[q] : 0xFFFFFFF0u, soff);
      }
    }
  };

  // a: fragment rows one pixel apart, +16 pixels per k-step, +4 for the high half; b: rows two patch pixels apart, +32 / +8
  f32x16 acc[TM][TN], acc_b;
  WGRAD_STREAM(TM, TN, G, 16 * RDY * 16, 4 * RDY * 16, 32 * RX * 16, 8 * RX * 16, smem, issue, a_base, b_base, l31, bias_i, t_begin, t_end, acc, acc_b)
  WGRAD_STORE(TM, TN, p, s, co0, 16, l31, lh, bias_i, acc_b, acc, b_chunk, i, kh * 4 + b_kw[j], true)
}

// 1 / 2: the shape class the kernel serves -- EVERY condition on the shape behind the route's front conditions (wgrad_route,
// conv_bwd.hip: bf16 storage, no resampling, 4x4 stride 2 pad 2, Ho == H / 2 + 1, Wo == W / 2 + 1), HRV_WGRAD_S2 and the
// slab-extent limit included -- or 0: none.  Fills `pl`.
int wgrad_s2_class(const hrv_conv2d_wgrad_t& d, WgradLdsPlan& pl) {
  const int Cout = d.Cout, x_C = d.x_C, N = d.N, H = d.H, W = d.W, Ho = d.Ho, Wo = d.Wo;
  const char* env = hrv::env("HRV_WGRAD_S2");
  if (env && env[0] == '0') return 0;
  if (Cout < 1 || x_C < 1 || N < 1 || H < 1 || W < 1) return 0;
  if ((d.dy_cstride | d.dy_coff | d.x_cstride | d.x_coff | x_C) & 7) return 0;   // 16-byte DMA granules
  if ((long long)N * Ho * Wo < 8192 || Wo < 32) return 0;
  const int gpt = (x_C + 31) / 32;
  int c_ = 0;
  if (gpt == 2 && Cout % 128 == 0) c_ = 1;              // 64 -> 128 (model1): 128 couts x (4 kw x 2 chunks)
  else if (gpt == 4 && Cout % 64 == 0) c_ = 2;          // 128 -> 256 (model2): 64 couts x (4 kw x 4 chunks)
  if (c_ == 0) return 0;
  pl.cls = c_; pl.tm = c_ == 1 ? 4 : 2;
  pl.gpt = gpt;
  pl.co_tiles = Cout / (32 * pl.tm); pl.col_tiles = 4; pl.row_mode = 0;       // (a block: one kernel row kh)
  pl.tiles_per_row = (Wo + 63) / 64;
  pl.n_tiles = N * Ho * pl.tiles_per_row;
  // X is addressed from two rows before the input row of the slab's first dY row, two input rows per dY row
  if (!wgrad_slabs(pl.co_tiles * 4, pl.n_tiles, pl.tiles_per_row, 4, (long long)Wo * d.dy_cstride * 2, 8, 2LL * W * d.x_cstride * 2, pl.S))
    return 0;
  return c_;
}

// Host side: launches the instance of class `pl` (from wgrad_s2_class over this `d`); the partials of pl.S slabs are left in
// d.workspace, the bias column sums right behind them, for the caller's wgrad_reduce_kernel launch.  HRV_OK or < 0.
int wgrad_s2_try(const hrv_conv2d_wgrad_t& d, const WgradLdsPlan& pl, hipStream_t st) {
  WgradS2Params p;
  p.dy = d.dy; p.dy_cs = d.dy_cstride; p.dy_co = d.dy_coff; p.Cout = d.Cout;
  p.x = d.x; p.x_cs = d.x_cstride; p.x_co = d.x_coff; p.x_C = d.x_C;
  p.N = d.N; p.H = d.H; p.W = d.W; p.Ho = d.Ho; p.Wo = d.Wo;
  p.CinTot = d.CinTot; p.ci_base = d.ci_base; p.ci_real = d.x_C_real;
  p.gpt = pl.gpt;
  p.co_tiles = pl.co_tiles;
  p.tiles_per_row = pl.tiles_per_row;
  p.n_tiles = pl.n_tiles;
  p.S = pl.S; p.ws = d.workspace;
  if (int rc = wgrad_workspace("wgrad_s2", pl.S, 16, d.Cout, d.CinTot, d.workspace, d.workspace_bytes, d.dbias != nullptr, p.bias_ws)) return rc;
  const int nblk = p.co_tiles * 4 * pl.S;
  if (pl.cls == 1) hipLaunchKernelGGL((conv_wgrad_s2_kernel<4, 2, 2>), dim3(nblk), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((conv_wgrad_s2_kernel<2, 4, 4>), dim3(nblk), dim3(256), 0, st, p);
  return check_launch("conv_wgrad_s2_kernel");
}

}  // namespace hrv
