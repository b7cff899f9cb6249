// The frame around the main loops of the persistent bf16 "patch-pass" kernels (conv_p2.hip, conv_s2.hip, spade_fused.hip,
// spade_gb.hip): a block works through 16x16-pixel tiles, and per tile through COLUMN PASSES of NTP column tiles of 32.  Shared
// here: the column plan, the tile decode, the unit-of-work scheduler, the timeline stamps, and -- host side -- the one place that
// decides how tiles and passes become launches and grids.  The main loops, heads and epilogues stay in the kernels' files.
#pragma once
#include "conv_params.h"

namespace hrv {

// ---- the column plan of a layer: `npass` passes, pass i = column tiles tile0[i] .. tile0[i] + ntp[i] of the layer, its packed
// weights at byte woff[i] of `bytes`.  (nchunk: K chunks per pass, for the planners that count them.  The layout is what the pack
// kernels read by value: spade_gb.hip's GbPlan keeps its own member order for that reason, see profiles/patch_pass_isa.txt.)
constexpr int PATCH_MAXP = 16;
struct PatchPlan {
  int npass, ntp[PATCH_MAXP], tile0[PATCH_MAXP];
  unsigned woff[PATCH_MAXP];
  int nchunk;
  long long bytes;
};
// the kernel parameters carry the same four members
template <typename Params, typename Plan>
inline void patch_plan_copy(Params& p, const Plan& pl) {
  p.npass = pl.npass;
  for (int i = 0; i < pl.npass; ++i) { p.ntp[i] = pl.ntp[i]; p.tile0[i] = pl.tile0[i]; p.woff[i] = pl.woff[i]; }
}

// ---- device side
// tile `bid` (0 .. m_tiles - 1, dealt over the XCDs by xcd_remap) of N images of H x W pixels (or cells): image, top-left corner.
// (The tile first, width before height: the order in which a kernel evaluates these is part of its device code.)
struct PatchTile { int n, y0, x0; };
__device__ __forceinline__ PatchTile patch_tile(const int bid, const int W, const int H, const int m_tiles) {
  const int tx = (W + 15) >> 4, ty = (H + 15) >> 4;
  const int mt = xcd_remap(bid, m_tiles);
  PatchTile t;
  t.n = mt / (tx * ty);
  const int rr = mt - t.n * (tx * ty);
  t.y0 = (rr / tx) << 4;
  t.x0 = (rr % tx) << 4;
  return t;
}

// tile number `mt` (no remap: the caller read it from a list) -> image, top-left corner
__device__ __forceinline__ PatchTile patch_tile_at(const int mt, const int W, const int H) {
  const int tx = (W + 15) >> 4, ty = (H + 15) >> 4;
  PatchTile t;
  t.n = mt / (tx * ty);
  const int rr = mt - t.n * (tx * ty);
  t.y0 = (rr / tx) << 4;
  t.x0 = (rr % tx) << 4;
  return t;
}

// registers 4g .. 4g+3 of an accumulator tile (swapped operands: 4 consecutive columns of the lane's pixel)
__device__ __forceinline__ f32x4 acc4(const f32x16& a, int g) {
  f32x4 r;
  r[0] = a[4 * g]; r[1] = a[4 * g + 1]; r[2] = a[4 * g + 2]; r[3] = a[4 * g + 3];
  return r;
}

// The diagnostic timeline (hrv_diag_set_tlog): 8 u64 per tile.  Slots 0 / 1 / 2 / 6 / 7 are the passes' own; slot 4 = where the
// tile ran (XCC_ID << 32 | HW_ID), slot 5 = which block, slot 3 = every store of the tile has drained.
// (start: slot 0 as well, for the kernel whose passes do not stamp it themselves)
__device__ __forceinline__ void tlog_where(unsigned long long* const tlog, const int bid, const bool start = false) {
  unsigned hw, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  if (start) tlog[(size_t)bid * 8 + 0] = wall_clock64();
  tlog[(size_t)bid * 8 + 4] = ((unsigned long long)xcc << 32) | hw;
  tlog[(size_t)bid * 8 + 5] = blockIdx.x;
}
// (a macro: as a function the same stamp picks other scalar registers in five conv_p2 instances)
#define TLOG_DRAINED(TLOG, BID)                                                                                         \
  if (TLOG) {                                                                                                           \
    __builtin_amdgcn_s_waitcnt(wait_vm(0));                                                                             \
    if (threadIdx.x == 0) (TLOG)[(size_t)(BID) * 8 + 3] = wall_clock64();                                               \
  }

// The scheduler of a launch that covers the passes [PASS0, PASS1) of the plan, all of one width.  A unit of work = one tile with
// those passes one after the other (what a tile's passes share -- source patch, label patch -- is loaded once or comes out of
// L2) -- or, P.pp (fewer tiles than resident blocks: the coarse levels), ONE (tile, pass): the passes of a tile run on different
// CUs at the same time.  Block b takes units b, b + gridDim.x, ...; every pass requests the head of the one that follows it.
//
// Expanded in the kernel, and its per-kernel parts are function-like MACROS expanded with it, not callables: a function template
// -- and already a lambda around the pass call -- is optimised on its own and changes register allocation and instruction order
// of every instance (profiles/patch_pass_isa.txt).  Each part sees the kernel's locals:
//   TILE(bid) -> PatchTile                                  HEAD(pass, T): the head of the block's first (tile, pass)
//   PASS(pass, T, bid, stale, block_first, first, last, nxt_pass, NT): one (tile, pass).  stale: the constants in LDS belong to
//     another pass (an EXPRESSION, to be used once: a kernel that keys its constants on more puts its own test in front);
//     block_first: nothing of an earlier pass is in flight; first / last: of this unit; nxt_pass / NT: whose head
//     to request (nxt_pass < 0: none)
// TLOG: the timeline buffer (a null constant where a kernel has none).
#define PATCH_PASS_UNITS(P, PASS0, PASS1, TILE, HEAD, PASS, TLOG)                                                       \
  {                                                                                                                     \
    const int npg = (PASS1) - (PASS0);                                                                                  \
    const int units = (P).pp ? (P).m_tiles * npg : (P).m_tiles;                                                         \
    auto unit_tile = [&](const int u) { return (P).pp ? u / npg : u; };                                                 \
    auto unit_pass = [&](const int u) { return (P).pp ? (PASS0) + u % npg : (PASS0); };                                 \
    if ((int)blockIdx.x < units) HEAD(unit_pass(blockIdx.x), TILE(unit_tile(blockIdx.x)));                              \
    int c_pass = -1;                                                                                                    \
    _Pragma("unroll 1") for (int u = blockIdx.x; u < units; u += gridDim.x) {                                           \
      const int bid = unit_tile(u);                                                                                     \
      if ((TLOG) && threadIdx.x == 0) tlog_where(TLOG, bid);                                                            \
      const PatchTile T = TILE(bid);                                                                                    \
      const int nu = u + gridDim.x;                                                                                     \
      const PatchTile TN = TILE(unit_tile(nu < units ? nu : u));                                                        \
      const int pa = unit_pass(u), pb = (P).pp ? pa + 1 : (PASS1);                                                      \
      _Pragma("unroll 1") for (int pass = pa; pass < pb; ++pass) {                                                      \
        const bool lastp = pass == pb - 1;                                                                              \
        const int nxt_pass = !lastp ? pass + 1 : (nu < units ? unit_pass(nu) : -1);                                     \
        PASS(pass, T, bid, (c_pass != pass), u == (int)blockIdx.x && pass == pa, pass == pa, lastp, nxt_pass,           \
             lastp ? TN : T);                                                                                           \
        c_pass = pass;                                                                                                  \
      }                                                                                                                 \
      TLOG_DRAINED(TLOG, bid)                                                                                           \
    }                                                                                                                   \
  }

// ---- host side: tiles -> units -> launches
inline int64_t patch_tiles(int N, int H, int W) { return (int64_t)N * ((H + 15) / 16) * ((W + 15) / 16); }
// fewer tiles than the resident blocks of a two-blocks-per-CU kernel: one (tile, pass) per unit of work (P.pp)
inline bool patch_pp(int64_t tiles) { return tiles < 2 * (int64_t)persistent_cus(); }
// Does a layer fill the chip?  The threshold is in quarter-units per CU (environment `env_name`, default `q4_default`), counted in
// UNITS of work: a level with fewer tiles than resident blocks spreads the passes of a tile over the CUs, so what has to fill
// the chip is tiles x passes (the 64 x 48 level's 48 tiles x 4 passes of a 512-column layer).
inline int patch_units_fill(int64_t tiles, int npass, const char* env_name, int q4_default) {
  const char* e = hrv::env(env_name);      // (cached by hrv::env: no getenv here after the first call)
  int q4 = e ? atoi(e) : q4_default;
  if (q4 < 1) q4 = q4_default;
  const int64_t units = patch_pp(tiles) ? tiles * npass : tiles;
  return 4 * units >= q4 * (int64_t)persistent_cus() ? 1 : 0;
}
// Passes of equal width share a launch: launch(a, b, grid) for every run [a, b) of equal ntp, grid = the launch's units of work,
// at most the resident blocks of that width (blocks_per_cu(ntp) per CU).
template <typename Plan, typename BlocksPerCu, typename Launch>
inline void patch_pass_groups(const Plan& pl, int m_tiles, bool pp, BlocksPerCu blocks_per_cu, Launch launch) {
  for (int a = 0; a < pl.npass;) {
    int b = a;
    while (b < pl.npass && pl.ntp[b] == pl.ntp[a]) ++b;
    const long long units = pp ? (long long)m_tiles * (b - a) : m_tiles;
    const int cap = blocks_per_cu(pl.ntp[a]) * persistent_cus();
    launch(a, b, units < cap ? (int)units : cap);
    a = b;
  }
}

}  // namespace hrv
