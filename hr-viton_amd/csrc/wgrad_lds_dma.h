// The streaming skeleton shared by the LDS-DMA weight-gradient kernels (wgrad_tr.hip: stride 1, wgrad_s2.hip: PatchGAN's 4x4
// stride 2).  A block keeps a TM x TN grid of 32x32 tiles of dW in registers and streams 64-pixel tiles of dY and of an X patch
// through NS LDS stages: both operands arrive by LDS-DMA in their natural [pixel][channel] order, fragments are fetched with
// transposing reads.  What differs between the kernels -- how a tile's X patch is addressed, how far apart a fragment's pixel rows
// lie, which (tap, chunk) a column group is, the shape classes -- stays in their files; the stage geometry, the pipelined tile
// loop with its hand-counted waits, the epilogue and the host's slab rule are here, once.
#pragma once
#include "conv_params.h"

namespace hrv {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// A resource over "everything after `base`": every out-of-image lane is masked explicitly (voffset = 0xFFFFFFF0 >= num_records =>
// the DMA writes zeros); in-range voffsets are small, the tile position travels in the (unchecked) scalar offset
__device__ __forceinline__ rsrc_t wgrad_rsrc(const void* base) { return make_rsrc(base, 0x7FFFFFF0u); }

// LDS rows [pixel][channel] are padded to `res` (mod 8) 16-byte slots: a transposing read of a 32-lane group touches 4 pixel rows
// x 64 bytes, and banks are (address / 4) mod 64, so the four rows must start in four different 64-byte quarters of the 256-byte
// bank line -- 4 (mod 8) for rows one pixel apart, 2 (mod 8) for rows two pixels apart.  Pad slots are DMA'd as zeros by
// out-of-range offsets.  Measured on dense 256-byte X rows (profiles/r02_pmc_wgrad_tr.txt, first build): SQ_LDS_BANK_CONFLICT =
// 53 % of SQ_LDS_IDX_ACTIVE = exactly the 4-way conflict of the 6 X reads per k-step next to 10 conflict-free dY reads on
// 320-byte rows.
constexpr int pad_slots(int s, int res) { return s + ((res - (s & 7)) & 7); }

// Stage geometry of a kernel instance: RDY 16-byte slots per dY pixel row, NX X DMA instructions (of 64 lanes x 16 bytes) per tile
template <int RDY, int NX>
struct WgradStage {
  static constexpr int TW = 64;                   // pixels per tile
  static constexpr int NDY = RDY;                 // dY DMA instructions per tile (64 pixels x RDY slots / 64 lanes)
  static_assert(NDY % 4 == 0, "dY instructions split evenly over the waves");
  static constexpr int NDYW = NDY / 4;
  static constexpr int NXW = (NX + 3) / 4;        // per wave (the last ones may repeat instruction NX-1: benign)
  static constexpr int DYB = NDY * 1024, XB = NX * 1024, STAGE = DYB + XB;
  static constexpr int NS = (163840 / STAGE) >= 4 ? 4 : (163840 / STAGE);
  static_assert(NS >= 2, "at least two stages must fit the 160 KB LDS");
  static constexpr int NPW = NDYW + NXW;          // DMA instructions per wave per stage
  static_assert(NPW * (NS - 2) < 64, "vmcnt is a 6-bit counter");
  // lgkmcnt(0) and: all but the NS-2 youngest stages of this wave's DMA / every DMA
  static constexpr int WAIT_RUN = ((NPW * (NS - 2)) & 15) | (7 << 4) | (0 << 8) | (((NPW * (NS - 2)) >> 4) << 14);
  static constexpr int WAIT_ALL = 0 | (7 << 4) | (0 << 8);
};

// WGRAD_STREAM streams tiles [t_begin, t_end) of a block's slab: acc[i][j] (f32x16 [TM][TN], zeroed here) += dY tile i^T x X group j
// over every pixel, acc_b (wave-uniform bias_i >= 0) += column sums of dY tile bias_i -- the bias gradient, one extra MFMA per
// k-step against a constant B fragment whose column 0 is all ones (D[co][0] = sum_k dY[k][co]).  G is the kernel's WgradStage;
// `issue(t, buf)` requests tile t into stage `buf` of smem (G::NPW DMA instructions per wave); a_base / b_base[j] are this lane's
// fragment addresses inside a stage, A_KS / B_KS the bytes from one k-step (16 pixels) to the next, A_HI / B_HI those from a
// fragment's low half (pixel rows 0..3) to its high half.
//
// Fragment reads are inline asm (the ds_read_tr16 builtin makes hipcc wait vmcnt(0) for every pending LDS-DMA before the first
// read of a k-step, which serialises the pipeline; plain asm reads are invisible to that pass), so the LDS counter is managed by
// hand: reads of k-step k+1 are issued in two halves around the MFMAs of k-step k, "lgkmcnt(half)" at the top of a step says the
// CURRENT step's fragments have all landed (LDS returns in order).
//
// The prologue leaves NS-1 tiles in flight, the first one landed.  Tile t+NS-1 is requested at the top of tile t: its buffer was
// read in tile t-1, and every wave passed the barrier after its reads.  At the last k-step of a tile every LDS read of the tile
// has been issued; once they are back (lgkmcnt(0)) the stage is free, and tile t+1 (this wave's DMA of it: WAIT_RUN, or WAIT_ALL
// when nothing younger is in flight) must have landed on every wave (the barrier) before its first fragments are fetched.
//
// A macro and not a function template: a template receives `issue` as a callable that the compiler inlines into the template
// first and optimises there, behind the closure's references, before the whole arrives in the kernel -- the kernels then come out
// with other prologues and register assignments than with the loop written in place.  Expanded in place they compile to what
// they were (profiles/wgrad_skeleton_isa.txt).
#define WGRAD_READ(DST, ADDR, OFF) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(DST) : "v"(ADDR), "n"(OFF) : "memory")
// reads [R0, R1) of k-step KS into fragment set SET: reads 2i, 2i+1 = a[i] (lo, hi) from ABASE, 2TM + 2j, +1 = b[j] from BBASE[j]
#define WGRAD_READS(TM, A_KS, A_HI, B_KS, B_HI, SET, KS, R0, R1, ABASE, BBASE)                             \
  {                                                                                                        \
    _Pragma("unroll") for (int r = (R0); r < (R1); ++r) {                                                  \
      if (r < 2 * TM) {                                                                                    \
        const int i = r >> 1, hi = r & 1;                                                                  \
        WGRAD_READ(fr[SET][r], ABASE, (KS) * (A_KS) + i * 64 + hi * (A_HI));                               \
      } else {                                                                                             \
        const int j = (r - 2 * TM) >> 1, hi = r & 1;                                                       \
        WGRAD_READ(fr[SET][r], BBASE[j], (KS) * (B_KS) + hi * (B_HI));                                     \
      }                                                                                                    \
    }                                                                                                      \
  }
#define WGRAD_FRAG(SET, R) __builtin_bit_cast(bf16x8, __builtin_shufflevector(fr[SET][2 * (R)], fr[SET][2 * (R) + 1], 0, 1, 2, 3, 4, 5, 6, 7))
// MFMAs [M0, M1) of the TM x TN grid (row-major) on set SET; the bias MFMA rides behind the last one
#define WGRAD_MMAS(TM, TN, SET, M0, M1, acc, acc_b, bias_i)                                                \
  {                                                                                                        \
    _Pragma("unroll") for (int m = (M0); m < (M1); ++m) {                                                  \
      const int i = m / TN, j = m - i * TN;                                                                \
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(WGRAD_FRAG(SET, i), WGRAD_FRAG(SET, TM + j), acc[i][j], 0, 0, 0); \
    }                                                                                                      \
    if ((M1) == TM * TN) {                                                                                 \
      _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                       \
        if (bias_i == i) acc_b = __builtin_amdgcn_mfma_f32_32x32x16_bf16(WGRAD_FRAG(SET, i), ones, acc_b, 0, 0, 0); \
    }                                                                                                      \
  }
#define WGRAD_STREAM(TM, TN, G, A_KS, A_HI, B_KS, B_HI, smem, issue, a_base, b_base, l31, bias_i, t_begin, t_end, acc, acc_b)          \
  {                                                                                                                                    \
    _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                                                     \
      _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                                                   \
        _Pragma("unroll") for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;                                                             \
    _Pragma("unroll") for (int e = 0; e < 16; ++e) acc_b[e] = 0.f;                                                                     \
    bf16x8 ones;                                                                                                                       \
    {                                                                                                                                  \
      const short one = l31 == 0 ? (short)0x3F80 : (short)0;                                                                           \
      const s16x8 o8 = {one, one, one, one, one, one, one, one};                                                                       \
      ones = __builtin_bit_cast(bf16x8, o8);                                                                                           \
    }                                                                                                                                  \
    constexpr int NS_ = G::NS, STAGE_ = G::STAGE;                                                                                      \
    constexpr int NR = 2 * (TM + TN); /* tr reads per k-step */                                                                        \
    constexpr int NH1 = NR / 2;                                                                                                        \
    static_assert(NH1 <= 15, "lgkmcnt is a 4-bit counter");                                                                            \
    constexpr int KSTEPS = G::TW / 16;                                                                                                 \
    static_assert(KSTEPS % 2 == 0, "fragment sets alternate by k-step parity");                                                        \
    s16x4 fr[2][NR]; /* [set][read] */                                                                                                 \
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;                                    \
    constexpr int WAIT_H1 = 0x3F | (7 << 4) | (NH1 << 8) | (3 << 14); /* lgkmcnt(NH1), vmcnt untouched */                              \
    constexpr int WAIT_L0 = 0x3F | (7 << 4) | (0 << 8) | (3 << 14);   /* lgkmcnt(0) */                                                 \
    if (t_begin < t_end) {                                                                                                             \
      _Pragma("unroll") for (int q = 0; q < NS_ - 1; ++q)                                                                              \
        if (t_begin + q < t_end) issue(t_begin + q, q);                                                                                \
      if (t_begin + NS_ - 1 <= t_end) __builtin_amdgcn_s_waitcnt(G::WAIT_RUN);                                                         \
      else __builtin_amdgcn_s_waitcnt(G::WAIT_ALL);                                                                                    \
      __builtin_amdgcn_s_barrier();                                                                                                    \
      asm volatile("" ::: "memory");                                                                                                   \
      int rb = 0, wb = NS_ - 1;                                                                                                        \
      unsigned a_addr = lds0 + (unsigned)a_base;                                                                                       \
      unsigned b_addr[TN];                                                                                                             \
      _Pragma("unroll") for (int j = 0; j < TN; ++j) b_addr[j] = lds0 + (unsigned)b_base[j];                                           \
      WGRAD_READS(TM, A_KS, A_HI, B_KS, B_HI, 0, 0, 0, NR, a_addr, b_addr) /* first k-step of the first tile */                        \
      for (int t = t_begin; t < t_end; ++t) {                                                                                          \
        const bool more = t + NS_ - 1 < t_end;                                                                                         \
        if (more) issue(t + NS_ - 1, wb);                                                                                              \
        const int nb = rb == NS_ - 1 ? 0 : rb + 1;                                                                                     \
        const unsigned a_next = lds0 + (unsigned)(a_base + nb * STAGE_);                                                               \
        unsigned b_next[TN];                                                                                                           \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) b_next[j] = lds0 + (unsigned)(b_base[j] + nb * STAGE_);                         \
        _Pragma("unroll") for (int ks = 0; ks < KSTEPS; ++ks) {                                                                        \
          const int cur = ks & 1, nxt = cur ^ 1;                                                                                       \
          if (ks + 1 < KSTEPS) {                                                                                                       \
            WGRAD_READS(TM, A_KS, A_HI, B_KS, B_HI, nxt, ks + 1, 0, NH1, a_addr, b_addr)                                               \
            __builtin_amdgcn_s_waitcnt(WAIT_H1); /* set `cur` has landed */                                                            \
          } else {                                                                                                                     \
            if (t + 1 < t_end) {                                                                                                       \
              if (more) __builtin_amdgcn_s_waitcnt(G::WAIT_RUN);                                                                       \
              else __builtin_amdgcn_s_waitcnt(G::WAIT_ALL);                                                                            \
              __builtin_amdgcn_s_barrier();                                                                                            \
              asm volatile("" ::: "memory");                                                                                           \
              WGRAD_READS(TM, A_KS, A_HI, B_KS, B_HI, nxt, 0, 0, NH1, a_next, b_next)                                                  \
              __builtin_amdgcn_s_waitcnt(WAIT_H1);                                                                                     \
            } else {                                                                                                                   \
              __builtin_amdgcn_s_waitcnt(WAIT_L0);                                                                                     \
            }                                                                                                                          \
          }                                                                                                                            \
          __builtin_amdgcn_sched_barrier(0);                                                                                           \
          WGRAD_MMAS(TM, TN, cur, 0, (TM * TN) / 2, acc, acc_b, bias_i)                                                                \
          __builtin_amdgcn_sched_barrier(0);                                                                                           \
          if (ks + 1 < KSTEPS) {                                                                                                       \
            WGRAD_READS(TM, A_KS, A_HI, B_KS, B_HI, nxt, ks + 1, NH1, NR, a_addr, b_addr)                                              \
          } else if (t + 1 < t_end) {                                                                                                  \
            WGRAD_READS(TM, A_KS, A_HI, B_KS, B_HI, nxt, 0, NH1, NR, a_next, b_next)                                                   \
          }                                                                                                                            \
          __builtin_amdgcn_sched_barrier(0);                                                                                           \
          WGRAD_MMAS(TM, TN, cur, (TM * TN) / 2, TM * TN, acc, acc_b, bias_i)                                                          \
          __builtin_amdgcn_sched_barrier(0);                                                                                           \
        }                                                                                                                              \
        a_addr = a_next;                                                                                                               \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) b_addr[j] = b_next[j];                                                          \
        rb = nb;                                                                                                                       \
        wb = wb == NS_ - 1 ? 0 : wb + 1;                                                                                               \
      }                                                                                                                                \
    }                                                                                                                                  \
  }

// WGRAD_STORE is the epilogue of slab s: the bias column sums to bias_ws[s][Cout], tile acc[i][j] to couts co0 + 32 COT .. of tap TAP,
// input channels 32 b_chunk[j] .. of the [S][taps][Cout][CinTot] workspace of p.  COT is an expression in the tile row i: the block's
// cout tile that row is; TAP and LIVE are expressions in the group index j: the group's tap, and whether it is a real (tap, chunk)
// and not an idle slot.  A macro for the reason given above.
// D[i = cout][j = ci]: col = l31 = lane&31 (ci), row = (reg&3) + 8*(reg>>2) + 4*lh, lh = lane>>5 (cout)
#define WGRAD_STORE(TM, TN, p, s, co0, taps, l31, lh, bias_i, acc_b, acc, b_chunk, COT, TAP, LIVE)                                     \
  {                                                                                                                                    \
    if (bias_i >= 0 && bias_i < TM && l31 == 0) {                                                                                      \
      _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                                                 \
        const int co = co0 + bias_i * 32 + 4 * lh + (e & 3) + 8 * (e >> 2);                                                            \
        if (co < p.Cout) p.bias_ws[(size_t)s * p.Cout + co] = acc_b[e];                                                                \
      }                                                                                                                                \
    }                                                                                                                                  \
    _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                                                   \
      const int ci = b_chunk[j] * 32 + l31;                                                                                            \
      if (!(LIVE) || ci >= p.ci_real) continue;                                                                                        \
      float* wsp = p.ws + ((size_t)s * (taps) + TAP) * p.Cout * p.CinTot; /* TAP as written: the sum associates left */                \
      _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                                                   \
        _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                                               \
          const int co = co0 + (COT) * 32 + 4 * lh + (e & 3) + 8 * (e >> 2);                                                           \
          if (co < p.Cout) wsp[(size_t)co * p.CinTot + p.ci_base + ci] = acc[i][j][e];                                                 \
        }                                                                                                                              \
    }                                                                                                                                  \
  }
// (bias gradient, second stage: the per-slab column sums are summed by the caller's wgrad_reduce_kernel launch)

// Host: the slab count of `jobs` (cout tile, column tile) blocks per slab over n_tiles tiles.  One block per CU (a block owns
// 120-152 KB of LDS): the grid must NOT exceed the CU count, or the surplus blocks run as a second round on an otherwise idle chip
// (first build: 258 blocks, kernel time 2x the wave lifetime).  Per-tile scalar offsets are relative to the slab's first row, so
// either operand's extent over a slab -- its dY rows plus *_pad rows, of *_row_bytes each -- must fit 31 bits: false when not.
inline bool wgrad_slabs(int jobs, int n_tiles, int tiles_per_row, long long dy_pad, long long dy_row_bytes, long long x_pad,
                        long long x_row_bytes, int& S) {
  S = persistent_cus() / jobs;
  if (S > n_tiles / 8) S = n_tiles / 8;
  if (S > 256) S = 256;
  if (S < 1) S = 1;
  const long long rows = n_tiles / S / tiles_per_row;
  return (rows + dy_pad) * dy_row_bytes < 0x7FF00000LL && (rows + x_pad) * x_row_bytes < 0x7FF00000LL;
}

// Host: checks that `workspace` holds S slabs of [taps][Cout][CinTot] partials plus the bias sums and places the latter right
// behind the slabs ([S][Cout]; null when no bias gradient is wanted).  HRV_OK or HRV_ERR_ARG.
inline int wgrad_workspace(const char* who, int S, int taps, int Cout, int CinTot, float* workspace, long long workspace_bytes, bool bias,
                           float*& bias_ws) {
  const long long need = ((long long)S * taps * Cout * CinTot + 256LL * Cout) * 4;
  if (workspace_bytes < need) {
    set_error("%s: workspace too small (%lld < %lld)", who, workspace_bytes, need);
    return HRV_ERR_ARG;
  }
  bias_ws = bias ? workspace + (size_t)S * taps * Cout * CinTot : nullptr;
  return HRV_OK;
}

// Host: the shape class of a weight gradient on one of the two kernels and the block geometry that follows from it.  The route
// (conv_bwd.hip, wgrad_route) has a class function fill it, hrv_conv2d_wgrad hands it to the same kernel's launch.
struct WgradLdsPlan {
  int cls;                                  // wgrad_tr: 0..8; wgrad_s2: 1 / 2
  int tm;                                   // 32-cout tiles per wave (tr) / per block (s2)
  int co_tiles, col_tiles, row_mode;        // (col_tiles, row_mode: tr only)
  int gpt, tiles_per_row, n_tiles, S;
};
// wgrad_tr.hip, stride-1 'same' layers: the class (0..8) or -1 / launches what the class says (partials of pl.S slabs in d.workspace)
int wgrad_tr_class(const hrv_conv2d_wgrad_t& d, WgradLdsPlan& pl);
int wgrad_tr_try(const hrv_conv2d_wgrad_t& d, const WgradLdsPlan& pl, hipStream_t st);
// wgrad_s2.hip, PatchGAN's 4x4 stride-2 pad-2 layers (d.Ho == d.H / 2 + 1, d.Wo == d.W / 2 + 1): the class (1 / 2) or 0 / the launch
int wgrad_s2_class(const hrv_conv2d_wgrad_t& d, WgradLdsPlan& pl);
int wgrad_s2_try(const hrv_conv2d_wgrad_t& d, const WgradLdsPlan& pl, hipStream_t st);

}  // namespace hrv
