// SPADE / InstanceNorm backward (NHWC, fp32 or bf16 storage per operand): stage 1 (element-wise + per-(n, slab, c) partial sums),
// the fixed-order finalize of the slab partials, stage 2 (dx + the noise-scale partials) -- for one norm, or in one pass for the two
// norms of a learned-shortcut block that normalise the same x.  There is ONE body per stage: the per-norm statements are written
// once (norm_s1_* / norm_s2_* below) and the single kernel is the one-norm case of the pair's, so an instance is bit-identical
// to the generic kernel, and the pair to two sequential single calls, by construction.  All reductions are two-stage with a fixed
// summation order (deterministic).
#include <string>

#include "hrv_common.h"

namespace hrv {

// x = cat(nearest_up2(lo), hi) along channels, never materialised (up_g > 0): channel groups [0, up_g) come from `x` = lo
// [N][H/2][W/2][x_cs] at (h >> 1, w >> 1), the others from `x2` = hi [N][H][W][x2_cs]
struct XSrc {
  const float* x; int x_cs, x_co;
  const float* x2; int x2_cs, x2_co, up_g;
  int H, W;
};
// a thread's channel group g is fixed: its source (tensor, stride, low-resolution or not) is resolved once, per pixel only the
// pixel index differs
struct XThread {
  const float* base;      // channel group g of pixel 0 of sample n
  int cs, lo, W, Wl;
};
// UP: whether x is the up-sampled pair, known when the kernel is compiled (0 / 1) or read from the source (-1)
template <int UP = -1>
__device__ __forceinline__ XThread xsrc_thread(const XSrc& s, int n, int g) {
  XThread t;
  const bool up = UP < 0 ? s.up_g > 0 : UP != 0;
  t.W = s.W; t.Wl = s.W >> 1;
  t.lo = (up && g < s.up_g) ? 1 : 0;
  if (up && !t.lo) {
    t.cs = s.x2_cs;
    t.base = s.x2 + (size_t)n * s.H * s.W * s.x2_cs + s.x2_co + (g - s.up_g) * 4;
  } else {
    t.cs = s.x_cs;
    t.base = s.x + (size_t)n * (t.lo ? (s.H >> 1) * (s.W >> 1) : s.H * s.W) * s.x_cs + s.x_co + g * 4;
  }
  return t;
}
__device__ __forceinline__ const float* xsrc_ptr(const XThread& t, int px) {
  int q = px;
  if (t.lo) {
    const int h = px / t.W, w = px - h * t.W;
    q = (h >> 1) * t.Wl + (w >> 1);
  }
  return t.base + (size_t)q * t.cs;
}

// ---------------------------------------------------------------------------
// stage 1 (elementwise + per-(n,c) partial sums).
//   forward:  v = x + z*ns;  nh = (v - mean)*rstd;  out = act(nh*g1p + beta)   (g1p = 1+gamma)
//   given dout:  dpre = dout * act'(out);  dnh = dpre*g1p;  dgamma = dpre*nh;  dbeta = dpre
// plain InstanceNorm (+act) is the same with g1p == NULL (=1) and no dgamma/dbeta outputs.
// Writes dnh (needed again by stage 2), optionally dgb = [dgamma | dbeta] (2C channels) and
// the partial sums S1 = sum dnh, S2 = sum dnh*nh per (n, slab, c).
// ---------------------------------------------------------------------------
struct NormBwdParams {
  XSrc xs;
  const float* z; const float* ns;           // noise (nullable)
  const float* mean; const float* rstd;      // [N][C]
  const float* out; int out_cs, out_co;      // activation output (mask), nullable when act == NONE
  const float* g1p; int g_cs, g_co;          // 1+gamma, nullable
  const float* dout; int do_cs, do_co;
  float* dnh; int dn_cs, dn_co;
  float* dgb; int dgb_cs, dgb_co;            // nullable; [.., 2C]: dgamma at [0,C), dbeta at [C,2C)
  int N, H, W, C4, act; float slope;
  int NB; float* part;                       // [N][NB][C][2]
  int dgb_bf16, out_bf16;                    // storage of dgb / out: bf16 when only matrix cores (and this mask) read them
  int g1p_bf16;                              // (1 + gamma) stored as bf16 (the dedicated gamma|beta kernel writes it so)
  int dnh_bf16;                              // dnh (stage 1 -> stage 2) stored as bf16
  int dout_bf16;                             // dout stored as bf16 (the data gradient of a bf16-stored SPADE output)
  int dbeta_in_place;                        // dout IS the dbeta half of dgb (its producer wrote it there, activation derivative applied): not stored again
};

// stage 2: dx = rstd * (dnh - m1 - nh*m2)  (+ optional accumulate into dx), and partial sums of
// dx*z per (n, slab, c) for the noise_scale gradient.
struct NormBwd2Params {
  XSrc xs;
  const float* z; const float* ns;
  const float* mean; const float* rstd; const float* m1; const float* m2;
  const float* dnh; int dn_cs, dn_co; int dnh_bf16;
  float* dx; int dx_cs, dx_co; int accumulate;
  int dx_bf16;
  int N, H, W, C4;
  int NB; float* part;  // [N][NB][C] (only when z != NULL)
};

// ---- the storage form of a normalisation backward as one word.  The generic kernels (F < 0) read every choice from the parameter
// block at run time, as they always did; an instance (F >= 0) is compiled for one form, so its two-pixel body has no branch and
// keeps one storage form of each operand in registers.  Same statements, same order: an instance is bit-identical to the generic
// kernel on a descriptor of its form (norm_form_of() below is the only place that derives the word).
enum : int {
  NF_DOUT_BF16 = 1 << 0, NF_ACT_SHIFT = 1, NF_ACT_MASK = 3 << NF_ACT_SHIFT /* HRV_ACT_NONE / RELU / LRELU */, NF_OUT_BF16 = 1 << 3,
  NF_G1P = 1 << 4, NF_G1P_BF16 = 1 << 5, NF_DNH_BF16 = 1 << 6, NF_DGB = 1 << 7, NF_DGB_BF16 = 1 << 8, NF_DBETA_IN_PLACE = 1 << 9,
  NF_NOISE = 1 << 10, NF_UP = 1 << 11, NF_DX_BF16 = 1 << 12, NF_DX_ACC = 1 << 13,
  NF_STAGE2 = NF_DNH_BF16 | NF_NOISE | NF_UP | NF_DX_BF16 | NF_DX_ACC,       // what stage 2 depends on
  NF_STAGE1 = (NF_DX_BF16 - 1)                                               // ... and stage 1: everything but the dx bits
};
template <int F> struct NormForm {
  static __device__ __forceinline__ bool is(int bit, int run_time) { return F < 0 ? run_time != 0 : (F & bit) != 0; }
  static __device__ __forceinline__ int act(int run_time) { return F < 0 ? run_time : (F & NF_ACT_MASK) >> NF_ACT_SHIFT; }
  static constexpr int up = F < 0 ? -1 : ((F & NF_UP) ? 1 : 0);
};

// ---- what every stage kernel starts and ends with.  A block's share of the (pixel slab, sample, channel chunk) grid of
// hrv_common.h and a thread's place in it: pixels [p0, p1) of sample n, R pixel rows in flight, this thread on row r with channel
// group g (gl inside the chunk; blockIdx.z picks the chunk).
struct NormTile {
  int n, b, t, H, W, HW, C, p0, p1, GB, R, r, gl, g;
  bool live;        // g is a channel group of the tensor (the last chunk may be partly empty)
  bool active;      // ... and r a row that walks pixels (256 - R * GB threads idle)
};
__device__ __forceinline__ NormTile norm_tile(int H, int W, int C4, int NB) {
  NormTile T;
  T.n = blockIdx.y; T.b = blockIdx.x; T.t = threadIdx.x;
  T.H = H; T.W = W; T.HW = H * W; T.C = C4 * 4;
  const int PB = (T.HW + NB - 1) / NB;
  T.p0 = T.b * PB; T.p1 = min(T.p0 + PB, T.HW);
  T.GB = C4 < NORM_GCAP ? C4 : NORM_GCAP;
  T.R = 256 / T.GB;
  T.r = T.t / T.GB; T.gl = T.t - T.r * T.GB;
  T.g = blockIdx.z * T.GB + T.gl;
  T.live = T.g < C4;
  T.active = T.r < T.R && T.live;
  return T;
}
// Row 0 of the block collects the K per-thread sums of its R rows through LDS, rows in order (a fixed order).  True on the threads
// that then hold a total.  Every thread of the block must call it.  (The single's stage 1 carries these statements written out,
// see norm_bwd_stage1_body: whoever changes the order of the sums here changes it there, or the single and the pair part ways.)
template <int K>
__device__ __forceinline__ bool norm_reduce_rows(const NormTile& T, f32x4 (&s)[K]) {
  __shared__ f32x4 red[K][256];
#pragma unroll
  for (int k = 0; k < K; ++k) red[k][T.t] = s[k];
  __syncthreads();
  if (T.r != 0 || !T.live) return false;
  for (int rr = 1; rr < T.R; ++rr) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += red[k][rr * T.GB + T.gl];
  }
  return true;
}

// the noise map is [N][W][H]; (h, w) of a pixel are worked out once, whatever the number of norms that have noise
struct PixelHW { int h, w; };
__device__ __forceinline__ PixelHW norm_pixel_hw(const NormTile& T, int px, bool any_noise) {
  PixelHW q = {0, 0};
  if (any_noise) { q.h = px / T.W; q.w = px - q.h * T.W; }
  return q;
}
__device__ __forceinline__ float norm_noise_at(const float* z, const NormTile& T, PixelHW q) { return z[((size_t)T.n * T.W + q.w) * T.H + q.h]; }

// Stage 1 pins its roundings (fp contract(off) + the two fused multiply-adds written out): left to the compiler, which products
// fuse into a following add depends on the surrounding code, and an instance must round exactly as the generic kernel does --
// v = fma(z, noise_scale, x) and s2 = fma(dnh, nh, s2) are the two it has always fused; dnh and dgamma are rounded products.
__device__ __forceinline__ f32x4 fma4(f32x4 a, f32x4 b, f32x4 c) { return __builtin_elementwise_fma(a, b, c); }

// ---- stage 1, the part of ONE norm.  (A norm's parameter block is taken by reference to the kernel argument itself: no pointer
// tables over the two norms of a pair, which would force the arguments into scratch memory.)
struct Norm1 { f32x4 mu, rs, ns4; };                 // per thread: statistics and noise scale of its channel group
struct In1 { f32x4 d, o, g1; float zz; };            // per pixel: what is loaded besides x
template <int F>
__device__ __forceinline__ Norm1 norm_s1_begin(const NormBwdParams& q, const NormTile& T) {
  Norm1 m;
  m.mu = ld4(q.mean + (size_t)T.n * T.C + T.g * 4);
  m.rs = ld4(q.rstd + (size_t)T.n * T.C + T.g * 4);
  m.ns4 = NormForm<F>::is(NF_NOISE, q.z != nullptr) ? ld4(q.ns + T.g * 4) : (f32x4)(0.f);
  return m;
}
template <int F>
__device__ __forceinline__ In1 norm_s1_load(const NormBwdParams& q, const NormTile& T, int px, PixelHW hw) {
  typedef NormForm<F> Fm;
  In1 L;
  const size_t pix = (size_t)T.n * T.HW + px;
  const int g = T.g;
  L.zz = Fm::is(NF_NOISE, q.z != nullptr) ? norm_noise_at(q.z, T, hw) : 0.f;
  L.d = Fm::is(NF_DOUT_BF16, q.dout_bf16) ? ld4_bf16(q.dout, pix * q.do_cs + q.do_co + g * 4) : ld4(q.dout + pix * q.do_cs + q.do_co + g * 4);
  L.o = (f32x4)(0.f);
  if (Fm::act(q.act) != HRV_ACT_NONE) {
    const size_t oe = pix * q.out_cs + q.out_co + g * 4;
    L.o = Fm::is(NF_OUT_BF16, q.out_bf16) ? ld4_bf16(q.out, oe) : ld4(q.out + oe);
  }
  L.g1 = (f32x4)(1.f);
  if (Fm::is(NF_G1P, q.g1p != nullptr)) {
    const size_t ge1 = pix * q.g_cs + q.g_co + g * 4;
    L.g1 = Fm::is(NF_G1P_BF16, q.g1p_bf16) ? ld4_bf16(q.g1p, ge1) : ld4(q.g1p + ge1);
  }
  return L;
}
template <int F>
__device__ __forceinline__ void norm_s1_finish(const NormBwdParams& q, const NormTile& T, int px, f32x4 v, const In1& L, const Norm1& m,
                                               f32x4& s1, f32x4& s2) {
#pragma clang fp contract(off)      // (see fma4)
  typedef NormForm<F> Fm;
  const size_t pix = (size_t)T.n * T.HW + px;
  const int g = T.g, act = Fm::act(q.act);
  if (Fm::is(NF_NOISE, q.z != nullptr)) v = fma4((f32x4)(L.zz), m.ns4, v);
  const f32x4 nh = (v - m.mu) * m.rs;
  f32x4 dpre = L.d;
  if (act != HRV_ACT_NONE) {
#pragma unroll
    for (int e = 0; e < 4; ++e) dpre[e] *= dact(L.o[e], act, q.slope);
  }
  f32x4 dnh = dpre;
  if (Fm::is(NF_G1P, q.g1p != nullptr)) dnh *= L.g1;
  if (Fm::is(NF_DNH_BF16, q.dnh_bf16)) st4_bf16(q.dnh, pix * q.dn_cs + q.dn_co + g * 4, dnh);
  else *reinterpret_cast<f32x4*>(q.dnh + pix * q.dn_cs + q.dn_co + g * 4) = dnh;
  if (Fm::is(NF_DGB, q.dgb != nullptr)) {
    const bool keep_dbeta = Fm::is(NF_DBETA_IN_PLACE, q.dbeta_in_place);
    const size_t ge = pix * q.dgb_cs + q.dgb_co + g * 4;
    if (Fm::is(NF_DGB_BF16, q.dgb_bf16)) {
      st4_bf16(q.dgb, ge, dpre * nh);
      if (!keep_dbeta) st4_bf16(q.dgb, ge + T.C, dpre);
    } else {
      *reinterpret_cast<f32x4*>(q.dgb + ge) = dpre * nh;
      if (!keep_dbeta) *reinterpret_cast<f32x4*>(q.dgb + ge + T.C) = dpre;
    }
  }
  s1 += dnh;
  s2 = fma4(dnh, nh, s2);
}
__device__ __forceinline__ void norm_s1_store_part(const NormBwdParams& q, const NormTile& T, f32x4 s1, f32x4 s2) {
  float* dst = q.part + (((size_t)T.n * q.NB + T.b) * T.C + T.g * 4) * 2;
#pragma unroll
  for (int e = 0; e < 4; ++e) { dst[2 * e] = s1[e]; dst[2 * e + 1] = s2[e]; }
}

// NN norms over the same x (geometry and x are pa's; pb is read only when NN == 2), PX pixels per iteration: all loads of the PX
// pixels are requested before the first result is stored (the stores may alias the loads as far as the compiler knows, so a
// plain loop keeps one pixel's loads in flight per thread); every value and the order of the sums are those of the plain loop.
// The single runs two pixels.  The pair runs one: its seven 16-byte loads (x + three per norm) are as many as the single keeps
// in flight with two pixels, at half the registers of a two-pixel body (two pixels: the generic pair 229 -> two waves per SIMD,
// the instances 131 / 165, three waves; one pixel: 166, three waves, and 98 / 96, four and five).
template <int F, int NN, int PX>
__device__ __forceinline__ void norm_bwd_stage1_body(const NormBwdParams& pa, const NormBwdParams& pb) {
  const NormTile T = norm_tile(pa.H, pa.W, pa.C4, pa.NB);
  f32x4 s[2 * NN];                                   // s1, s2 of each norm
#pragma unroll
  for (int k = 0; k < 2 * NN; ++k) s[k] = (f32x4)(0.f);
  if (T.active) {
    Norm1 m[NN];
    m[0] = norm_s1_begin<F>(pa, T);
    if constexpr (NN == 2) m[1] = norm_s1_begin<F>(pb, T);
    const XThread xt = xsrc_thread<NormForm<F>::up>(pa.xs, T.n, T.g);
    const bool noise = NormForm<F>::is(NF_NOISE, pa.z != nullptr) || (NN == 2 && NormForm<F>::is(NF_NOISE, pb.z != nullptr));
    struct In { f32x4 v; In1 k[NN]; };
    auto load = [&](int px) {
      In L;
      L.v = ld4(xsrc_ptr(xt, px));                   // x: once per pixel, whatever NN
      const PixelHW hw = norm_pixel_hw(T, px, noise);
      L.k[0] = norm_s1_load<F>(pa, T, px, hw);
      if constexpr (NN == 2) L.k[1] = norm_s1_load<F>(pb, T, px, hw);
      return L;
    };
    auto finish = [&](int px, const In& L) {
      norm_s1_finish<F>(pa, T, px, L.v, L.k[0], m[0], s[0], s[1]);
      if constexpr (NN == 2) norm_s1_finish<F>(pb, T, px, L.v, L.k[1], m[1], s[2], s[3]);
    };
    int px = T.p0 + T.r;
    if constexpr (PX == 2) {
      for (; px + T.R < T.p1; px += 2 * T.R) {
        const In A = load(px), B = load(px + T.R);
        finish(px, A);
        finish(px + T.R, B);
      }
      if (px < T.p1) finish(px, load(px));
    } else {
      for (; px < T.p1; px += T.R) finish(px, load(px));
    }
  }
  if constexpr (NN == 1) {
    // norm_reduce_rows<2> written out, statement for statement (keep the two alike): through the helper the up-sampled SPADE
    // instance holds 81 registers instead of 79 and loses its sixth wave per SIMD (the other single instances move by up to four
    // registers either way)
    __shared__ f32x4 red[2][256];
    red[0][T.t] = s[0]; red[1][T.t] = s[1];
    __syncthreads();
    if (T.r == 0 && T.live) {
      for (int rr = 1; rr < T.R; ++rr) { s[0] += red[0][rr * T.GB + T.gl]; s[1] += red[1][rr * T.GB + T.gl]; }
      norm_s1_store_part(pa, T, s[0], s[1]);
    }
  } else if (norm_reduce_rows(T, s)) {
    norm_s1_store_part(pa, T, s[0], s[1]);
    norm_s1_store_part(pb, T, s[2], s[3]);
  }
}
__global__ __launch_bounds__(256) void norm_bwd_stage1_kernel(const NormBwdParams p) { norm_bwd_stage1_body<-1, 1, 2>(p, p); }
template <int F>
__global__ __launch_bounds__(256) void norm_bwd_stage1_inst(const NormBwdParams p) { norm_bwd_stage1_body<F, 1, 2>(p, p); }
// two normalisations over the SAME x (norm_0 and norm_s of a learned-shortcut SPADEResBlock both normalise the block input,
// network_generator.py:158-166); an instance serves two norms of the SAME form F
__global__ __launch_bounds__(256) void norm_bwd2_stage1_kernel(const NormBwdParams pa, const NormBwdParams pb) { norm_bwd_stage1_body<-1, 2, 1>(pa, pb); }
template <int F>
__global__ __launch_bounds__(256) void norm_bwd2_stage1_inst(const NormBwdParams pa, const NormBwdParams pb) { norm_bwd_stage1_body<F, 2, 1>(pa, pb); }

// fixed-order reduction of the slab partials: m1[n][c] = S1/HW, m2[n][c] = S2/HW
// 16 lanes per (sample, channel): lane l sums slabs l, l + 16, ... in double, then a fixed butterfly inside the 16-lane group
// (deterministic).  (One thread per (n, c) walking up to 256 slabs took 35 us; 31 of these per training step.)
__global__ void norm_bwd_finalize_kernel(const float* __restrict__ part, int N, int NB, int C, int HW,
                                         float* __restrict__ m1, float* __restrict__ m2) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = t >> 4, l = t & 15;
  const bool live = i < N * C;
  const int ii = live ? i : 0;
  const int n = ii / C, c = ii - n * C;
  double s1 = 0.0, s2 = 0.0;
  for (int b = l; b < NB; b += 16) {
    const float* src = part + (((size_t)n * NB + b) * C + c) * 2;
    s1 += (double)src[0];
    s2 += (double)src[1];
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o, 16);
    s2 += __shfl_xor(s2, o, 16);
  }
  if (live && l == 0) {
    m1[i] = (float)(s1 / HW);
    m2[i] = (float)(s2 / HW);
  }
}

// ---- stage 2, the part of ONE norm: its dx term d = rstd * (dnh - m1 - nh * m2), a rounded product, and the d * z sum
struct Norm2 { f32x4 mu, rs, a1, a2, ns4; };
struct In2 { f32x4 dn; float zz; };
template <int F>
__device__ __forceinline__ Norm2 norm_s2_begin(const NormBwd2Params& q, const NormTile& T) {
  const size_t sc = (size_t)T.n * T.C + T.g * 4;
  Norm2 m;
  m.mu = ld4(q.mean + sc); m.rs = ld4(q.rstd + sc); m.a1 = ld4(q.m1 + sc); m.a2 = ld4(q.m2 + sc);
  m.ns4 = NormForm<F>::is(NF_NOISE, q.z != nullptr) ? ld4(q.ns + T.g * 4) : (f32x4)(0.f);
  return m;
}
template <int F>
__device__ __forceinline__ In2 norm_s2_load(const NormBwd2Params& q, const NormTile& T, int px, PixelHW hw) {
  typedef NormForm<F> Fm;
  In2 L;
  L.zz = Fm::is(NF_NOISE, q.z != nullptr) ? norm_noise_at(q.z, T, hw) : 0.f;
  const size_t de = ((size_t)T.n * T.HW + px) * q.dn_cs + q.dn_co + T.g * 4;
  L.dn = Fm::is(NF_DNH_BF16, q.dnh_bf16) ? ld4_bf16(q.dnh, de) : ld4(q.dnh + de);
  return L;
}
template <int F>
__device__ __forceinline__ f32x4 norm_s2_term(const NormBwd2Params& q, f32x4 v, const In2& L, const Norm2& m, f32x4& sz) {
#pragma clang fp contract(off)      // (every product is rounded, in a single call and in a pair alike)
  if (NormForm<F>::is(NF_NOISE, q.z != nullptr)) v += L.zz * m.ns4;
  const f32x4 nh = (v - m.mu) * m.rs;
  const f32x4 d = m.rs * (L.dn - m.a1 - nh * m.a2);
  sz += d * L.zz;
  return d;
}

// NN norms over the same x, PX pixels per iteration with the loads of all of them first (see stage 1).  One norm: dx is bf16, or
// fp32 written or accumulated into.  Two: dx = d_b + d_a is written once, in fp32, with no read-modify-write of the first norm's
// result -- one commutative fp32 add of the two rounded terms, so bit-identical to two sequential calls with dx_accumulate on the
// second.
template <int F, int NN, int PX>
__device__ __forceinline__ void norm_bwd_stage2_body(const NormBwd2Params& pa, const NormBwd2Params& pb) {
  typedef NormForm<F> Fm;
  const NormTile T = norm_tile(pa.H, pa.W, pa.C4, pa.NB);
  const bool noise_a = Fm::is(NF_NOISE, pa.z != nullptr), noise_b = NN == 2 && Fm::is(NF_NOISE, pb.z != nullptr);
  f32x4 sz[NN];
#pragma unroll
  for (int k = 0; k < NN; ++k) sz[k] = (f32x4)(0.f);
  if (T.active) {
    Norm2 m[NN];
    m[0] = norm_s2_begin<F>(pa, T);
    if constexpr (NN == 2) m[1] = norm_s2_begin<F>(pb, T);
    const bool dx_bf16 = NN == 1 && Fm::is(NF_DX_BF16, pa.dx_bf16), acc = NN == 1 && Fm::is(NF_DX_ACC, pa.accumulate);
    const XThread xt = xsrc_thread<Fm::up>(pa.xs, T.n, T.g);
    struct In { f32x4 v, acc; In2 k[NN]; };
    auto load = [&](int px) {
      In L;
      L.v = ld4(xsrc_ptr(xt, px));
      const PixelHW hw = norm_pixel_hw(T, px, noise_a || noise_b);
      L.k[0] = norm_s2_load<F>(pa, T, px, hw);
      if constexpr (NN == 2) L.k[1] = norm_s2_load<F>(pb, T, px, hw);
      L.acc = (f32x4)(0.f);
      if (!dx_bf16 && acc) L.acc = ld4(pa.dx + ((size_t)T.n * T.HW + px) * pa.dx_cs + pa.dx_co + T.g * 4);
      return L;
    };
    auto finish = [&](int px, const In& L) {
#pragma clang fp contract(off)      // (the terms are rounded products, their sum with each other or with the old dx one add)
      const size_t oe = ((size_t)T.n * T.HW + px) * pa.dx_cs + pa.dx_co + T.g * 4;
      f32x4 d = norm_s2_term<F>(pa, L.v, L.k[0], m[0], sz[0]);
      if constexpr (NN == 2) d = norm_s2_term<F>(pb, L.v, L.k[1], m[1], sz[1]) + d;
      if (dx_bf16) {
        st4_bf16(pa.dx, oe, d);
      } else {
        if (acc) d += L.acc;
        *reinterpret_cast<f32x4*>(pa.dx + oe) = d;
      }
    };
    int px = T.p0 + T.r;
    if constexpr (PX == 2) {
      for (; px + T.R < T.p1; px += 2 * T.R) {
        const In A = load(px), B = load(px + T.R);
        finish(px, A);
        finish(px + T.R, B);
      }
      if (px < T.p1) finish(px, load(px));
    } else {
      for (; px < T.p1; px += T.R) finish(px, load(px));
    }
  }
  if (noise_a || noise_b) {
    if (norm_reduce_rows(T, sz)) {
      const size_t o = ((size_t)T.n * pa.NB + T.b) * T.C + T.g * 4;
      if (noise_a) *reinterpret_cast<f32x4*>(pa.part + o) = sz[0];
      if constexpr (NN == 2)
        if (noise_b) *reinterpret_cast<f32x4*>(pb.part + o) = sz[1];
    }
  }
}
__global__ __launch_bounds__(256) void norm_bwd_stage2_kernel(const NormBwd2Params p) { norm_bwd_stage2_body<-1, 1, 2>(p, p); }
template <int F>
__global__ __launch_bounds__(256) void norm_bwd_stage2_inst(const NormBwd2Params p) { norm_bwd_stage2_body<F, 1, 2>(p, p); }
__global__ __launch_bounds__(256) void norm_bwd2_stage2_kernel(const NormBwd2Params pa, const NormBwd2Params pb) { norm_bwd_stage2_body<-1, 2, 2>(pa, pb); }
template <int F>
__global__ __launch_bounds__(256) void norm_bwd2_stage2_inst(const NormBwd2Params pa, const NormBwd2Params pb) { norm_bwd_stage2_body<F, 2, 2>(pa, pb); }

}  // namespace hrv

using namespace hrv;

extern "C" int64_t hrv_norm_bwd_workspace_elems(int32_t N, int32_t H, int32_t W, int32_t C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return -1;
  const int nb = norm_slabs(H * W);
  return (int64_t)N * nb * ((C + 3) / 4 * 4) * 2 + (int64_t)N * ((C + 3) / 4 * 4) * 2;
}

static int norm_bwd_check(const hrv_norm_bwd_t* d) {
  HRV_REQUIRE(d && d->x && d->mean && d->rstd && d->dout && d->dnh && d->dx && d->workspace, "norm_bwd: null pointer");
  HRV_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->C % 4 == 0, "norm_bwd: extent (C %% 4 == 0)");
  HRV_REQUIRE((d->noise_z == nullptr) == (d->noise_scale == nullptr), "norm_bwd: noise_z/noise_scale go together");
  HRV_REQUIRE(d->act == HRV_ACT_NONE || d->out, "norm_bwd: activation output needed for its derivative");
  HRV_REQUIRE(((d->x_cstride | d->x_coff | d->out_cstride | d->out_coff | d->g1p_cstride | d->g1p_coff | d->dout_cstride |
                d->dout_coff | d->dnh_cstride | d->dnh_coff | d->dgb_cstride | d->dgb_coff | d->dx_cstride | d->dx_coff) & 3) == 0,
              "norm_bwd: strides/offsets must be multiples of 4");
  const int C = d->C;
  if (d->x_up_channels > 0) {
    HRV_REQUIRE(d->x2 && d->x_up_channels % 4 == 0 && d->x_up_channels < C && d->H % 2 == 0 && d->W % 2 == 0 &&
                    d->x_coff + d->x_up_channels <= d->x_cstride && d->x2_cstride % 4 == 0 && d->x2_coff % 4 == 0 &&
                    d->x2_coff + (C - d->x_up_channels) <= d->x2_cstride && ((uintptr_t)d->x2 & 15) == 0,
                "norm_bwd: upsampled source (%d of %d channels, %d x %d)", d->x_up_channels, C, d->H, d->W);
  }
  HRV_REQUIRE(!(d->dx_bf16 && d->dx_accumulate), "norm_bwd: a bf16 dx cannot be accumulated into");
  return HRV_OK;
}
// one descriptor (b == NULL) or the two norms of a pair
static int norm_bwd_check(const hrv_norm_bwd_t* a, const hrv_norm_bwd_t* b) {
  int rc = norm_bwd_check(a);
  if (rc || !b) return rc;
  rc = norm_bwd_check(b);
  if (rc) return rc;
  HRV_REQUIRE(a->x == b->x && a->x2 == b->x2 && a->x_cstride == b->x_cstride && a->x_coff == b->x_coff && a->x_up_channels == b->x_up_channels &&
                  a->N == b->N && a->H == b->H && a->W == b->W && a->C == b->C,
              "norm_bwd2: both norms must normalise the same x");
  HRV_REQUIRE(!a->dx_bf16 && !a->dx_accumulate && a->workspace != b->workspace && a->dnh != b->dnh, "norm_bwd2: dx fp32 (written, = dx_a + dx_b); separate scratch");
  return HRV_OK;
}

static int norm_bwd_pair_check(const hrv_norm_bwd_t* a, const hrv_norm_bwd_t* b) {
  HRV_REQUIRE(b, "norm_bwd: null pointer");
  return norm_bwd_check(a, b);
}

// dout handed over as the dbeta half of dgb (same buffer, same pixel stride, C channels up, same storage, no activation left
// to differentiate): dbeta = dout is already where it belongs
static bool norm_dbeta_in_place(const hrv_norm_bwd_t* d) {
  return d->dgb != nullptr && (const void*)d->dout == (const void*)d->dgb && d->dout_cstride == d->dgb_cstride &&
         d->dout_coff == d->dgb_coff + d->C && d->dout_bf16 == d->dgb_bf16 && d->act == HRV_ACT_NONE;
}

// workspace layout: [N][nb][C][2] slab partials (stage 1; reused as [N][nb][C] by stage 2) | m1 [N][C] | m2 [N][C]
static void norm_bwd_fill(const hrv_norm_bwd_t* d, NormBwdParams& p, NormBwd2Params& q) {
  const int C = d->C, nb = norm_slabs(d->H * d->W);
  float* part = d->workspace;
  float* m1 = part + (size_t)d->N * nb * C * 2;
  float* m2 = m1 + (size_t)d->N * C;
  XSrc xs;
  xs.x = d->x; xs.x_cs = d->x_cstride; xs.x_co = d->x_coff; xs.H = d->H; xs.W = d->W;
  xs.x2 = d->x2; xs.x2_cs = d->x2_cstride; xs.x2_co = d->x2_coff; xs.up_g = d->x_up_channels / 4;
  p.xs = xs; p.z = d->noise_z; p.ns = d->noise_scale;
  p.mean = d->mean; p.rstd = d->rstd; p.out = d->out; p.out_cs = d->out_cstride; p.out_co = d->out_coff;
  p.g1p = d->g1p; p.g_cs = d->g1p_cstride; p.g_co = d->g1p_coff; p.g1p_bf16 = d->g1p_bf16;
  p.dout = d->dout; p.do_cs = d->dout_cstride; p.do_co = d->dout_coff; p.dout_bf16 = d->dout_bf16;
  p.dnh = d->dnh; p.dn_cs = d->dnh_cstride; p.dn_co = d->dnh_coff; p.dnh_bf16 = d->dnh_bf16;
  p.dgb = d->dgb; p.dgb_cs = d->dgb_cstride; p.dgb_co = d->dgb_coff;
  p.N = d->N; p.H = d->H; p.W = d->W; p.C4 = C / 4; p.act = d->act; p.slope = d->act_slope; p.NB = nb; p.part = part;
  p.dgb_bf16 = d->dgb_bf16; p.out_bf16 = d->out_bf16;
  p.dbeta_in_place = norm_dbeta_in_place(d) ? 1 : 0;
  q.xs = xs; q.z = d->noise_z; q.ns = d->noise_scale;
  q.mean = d->mean; q.rstd = d->rstd; q.m1 = m1; q.m2 = m2;
  q.dnh = d->dnh; q.dn_cs = d->dnh_cstride; q.dn_co = d->dnh_coff; q.dnh_bf16 = d->dnh_bf16;
  q.dx = d->dx; q.dx_cs = d->dx_cstride; q.dx_co = d->dx_coff; q.accumulate = d->dx_accumulate;
  q.dx_bf16 = d->dx_bf16;
  q.N = d->N; q.H = d->H; q.W = d->W; q.C4 = C / 4; q.NB = nb; q.part = part;  // partials are free again in stage 2
}

// ---- compile-time instances.  The form word of a descriptor, and per kernel the table of forms that have an
// instance; a form outside its table, or HRV_NORM_BWD_GENERIC=1, runs on the generic kernel exactly as before the instances existed.
static int norm_form_of(const hrv_norm_bwd_t* d) {
  int f = 0;
  if (d->dout_bf16) f |= NF_DOUT_BF16;
  f |= (d->act << NF_ACT_SHIFT) & NF_ACT_MASK;          // (no table entry holds HRV_ACT_TANH: such a descriptor stays generic)
  if (d->act != HRV_ACT_NONE && d->out_bf16) f |= NF_OUT_BF16;
  if (d->g1p) f |= NF_G1P | (d->g1p_bf16 ? NF_G1P_BF16 : 0);
  if (d->dnh_bf16) f |= NF_DNH_BF16;
  if (d->dgb) f |= NF_DGB | (d->dgb_bf16 ? NF_DGB_BF16 : 0) | (norm_dbeta_in_place(d) ? NF_DBETA_IN_PLACE : 0);
  if (d->noise_z) f |= NF_NOISE;
  if (d->x_up_channels > 0) f |= NF_UP;
  if (d->dx_bf16) f |= NF_DX_BF16;
  else if (d->dx_accumulate) f |= NF_DX_ACC;
  return f;
}

// mixed-precision SPADE norm whose dout arrived in the dbeta half of [dgamma | dbeta] (1 + gamma in fp32 where the fused forward
// kernel saved it, in bf16 where the dedicated gamma|beta kernel did) / PatchGAN's InstanceNorm + LeakyReLU
constexpr int NF_SPADE = NF_DOUT_BF16 | NF_G1P | NF_DNH_BF16 | NF_DGB | NF_DGB_BF16 | NF_DBETA_IN_PLACE | NF_NOISE;
constexpr int NF_IN_LRELU = (HRV_ACT_LRELU << NF_ACT_SHIFT) | NF_DNH_BF16;
constexpr int NF_S2 = NF_DNH_BF16 | NF_NOISE;

// a kernel by its address: a single's takes one parameter block, a pair's two, and hipLaunchKernel hands over either
struct NormInst { int form; const void* fn; };
#define INST(KERNEL, F) {F, (const void*)KERNEL<F>}
static const NormInst norm_s1_insts[] = {INST(norm_bwd_stage1_inst, NF_SPADE | NF_G1P_BF16), INST(norm_bwd_stage1_inst, NF_SPADE | NF_G1P_BF16 | NF_UP),
                                         INST(norm_bwd_stage1_inst, NF_SPADE), INST(norm_bwd_stage1_inst, NF_IN_LRELU),
                                         INST(norm_bwd_stage1_inst, NF_IN_LRELU | NF_DOUT_BF16 | NF_OUT_BF16)};
static const NormInst norm_s2_insts[] = {INST(norm_bwd_stage2_inst, NF_S2 | NF_DX_BF16), INST(norm_bwd_stage2_inst, NF_S2),
                                         INST(norm_bwd_stage2_inst, NF_S2 | NF_DX_ACC), INST(norm_bwd_stage2_inst, NF_S2 | NF_UP),
                                         INST(norm_bwd_stage2_inst, NF_S2 | NF_UP | NF_DX_ACC), INST(norm_bwd_stage2_inst, NF_DNH_BF16 | NF_DX_BF16)};
static const NormInst norm_p1_insts[] = {INST(norm_bwd2_stage1_inst, NF_SPADE | NF_G1P_BF16 | NF_UP), INST(norm_bwd2_stage1_inst, NF_SPADE)};
static const NormInst norm_p2_insts[] = {INST(norm_bwd2_stage2_inst, NF_S2 | NF_UP), INST(norm_bwd2_stage2_inst, NF_S2)};
#undef INST

static bool norm_generic_forced() {
  const char* e = hrv::env("HRV_NORM_BWD_GENERIC");
  return e && atoi(e) != 0;
}
template <size_t K>
static const void* norm_inst_for(const NormInst (&tab)[K], int form) {
  if (!norm_generic_forced())
    for (size_t i = 0; i < K; ++i)
      if (tab[i].form == form) return tab[i].fn;
  return nullptr;
}

static std::string norm_form_name(int f) {
  static const struct { int bit; const char* name; } bits[] = {
      {NF_DOUT_BF16, "dout_bf16"}, {NF_OUT_BF16, "out_bf16"}, {NF_G1P, "g1p"}, {NF_G1P_BF16, "g1p_bf16"}, {NF_DNH_BF16, "dnh_bf16"}, {NF_DGB, "dgb"},
      {NF_DGB_BF16, "dgb_bf16"}, {NF_DBETA_IN_PLACE, "dbeta_in_place"}, {NF_NOISE, "noise"}, {NF_UP, "up"}, {NF_DX_BF16, "dx_bf16"}, {NF_DX_ACC, "dx_acc"}};
  static const char* acts[] = {"", "relu", "lrelu", "tanh"};
  std::string s = acts[(f & NF_ACT_MASK) >> NF_ACT_SHIFT];
  for (const auto& b : bits)
    if (f & b.bit) s += (s.empty() ? "" : "+") + std::string(b.name);
  return s.empty() ? "plain" : s;
}

// the instance table as text, one line per kernel: "<single|pair>.<stage1|stage2> <form>" (DESIGN.md 7h lists the same lines)
extern "C" const char* hrv_diag_norm_bwd_instances(void) {
  static const std::string text = [] {
    std::string t;
    for (const auto& i : norm_s1_insts) t += "single.stage1 " + norm_form_name(i.form) + "\n";
    for (const auto& i : norm_s2_insts) t += "single.stage2 " + norm_form_name(i.form) + "\n";
    for (const auto& i : norm_p1_insts) t += "pair.stage1 " + norm_form_name(i.form) + "\n";
    for (const auto& i : norm_p2_insts) t += "pair.stage2 " + norm_form_name(i.form) + "\n";
    return t;
  }();
  return text.c_str();
}

// The two stage kernels that serve a descriptor (b == NULL) or a pair, with the names their launches are checked under.  route:
// bit 0 = stage 1 runs on an instance, bit 1 = stage 2.  A pair runs on an instance where both norms have the same form and that
// form is in the table.
struct NormKernels { const void *k1, *k2; const char *name1, *name2; int route; };
static NormKernels norm_kernels_for(const hrv_norm_bwd_t* a, const hrv_norm_bwd_t* b) {
  const int fa = norm_form_of(a);
  const void *i1, *i2;
  if (!b) {
    i1 = norm_inst_for(norm_s1_insts, fa & NF_STAGE1);
    i2 = norm_inst_for(norm_s2_insts, fa & NF_STAGE2);
    return {i1 ? i1 : (const void*)norm_bwd_stage1_kernel, i2 ? i2 : (const void*)norm_bwd_stage2_kernel, "norm_bwd_stage1_kernel",
            "norm_bwd_stage2_kernel", (i1 ? 1 : 0) | (i2 ? 2 : 0)};
  }
  const int fb = norm_form_of(b) & ~NF_DX_ACC & ~NF_DX_BF16;      // (b->dx is ignored)
  i1 = (fa & NF_STAGE1) == (fb & NF_STAGE1) ? norm_inst_for(norm_p1_insts, fa & NF_STAGE1) : nullptr;
  i2 = (fa & NF_STAGE2) == (fb & NF_STAGE2) ? norm_inst_for(norm_p2_insts, fa & NF_STAGE2) : nullptr;
  return {i1 ? i1 : (const void*)norm_bwd2_stage1_kernel, i2 ? i2 : (const void*)norm_bwd2_stage2_kernel, "norm_bwd2_stage1_kernel",
          "norm_bwd2_stage2_kernel", (i1 ? 1 : 0) | (i2 ? 2 : 0)};
}

// which kernels serve a descriptor (b == NULL) or a pair: bit 0 = stage 1 runs on an instance, bit 1 = stage 2; < 0: invalid
extern "C" int hrv_diag_norm_bwd_route(const hrv_norm_bwd_t* a, const hrv_norm_bwd_t* b) {
  const int rc = norm_bwd_check(a, b);
  return rc ? rc : norm_kernels_for(a, b).route;
}

// Whether the pair pass is the faster way through norm_0 and norm_s of a block (gen_train.BlockT.backward asks; HRV_NORM_BWD2 there
// overrides the answer).  The gate is on the form alone: both stages on an instance.  On the generic pair kernels (166 / 117
// registers, three and four waves per SIMD) the pair lost 10-17 % to two sequential calls; on the instances (98 / 96 and
// 106 / 118, four or five waves) it measured faster at every level of the 4 x 1024x768 step, 1024x768x80 (-27 %) down to
// 16x12x1040 (-41 %), and level with them at 128x96x528 -- so there is no extent gate.
extern "C" int hrv_spade_norm_bwd2_supported(const hrv_norm_bwd_t* a, const hrv_norm_bwd_t* b) {
  return norm_bwd_pair_check(a, b) == HRV_OK && norm_kernels_for(a, b).route == 3 ? 1 : 0;
}

// The launch chain of one norm (b == NULL) or a pair: stage 1, finalize (once per norm), stage 2, sum_rows (once per norm with noise).
static int norm_bwd_launch(const hrv_norm_bwd_t* a, const hrv_norm_bwd_t* b, hipStream_t st) {
  int rc = norm_bwd_check(a, b);
  if (rc) return rc;
  const hrv_norm_bwd_t* ds[2] = {a, b};
  const int nn = b ? 2 : 1, N = a->N, C = a->C, HW = a->H * a->W, nb = norm_slabs(HW);
  NormBwdParams p[2];
  NormBwd2Params q[2];
  for (int k = 0; k < nn; ++k) norm_bwd_fill(ds[k], p[k], q[k]);
  const NormKernels ks = norm_kernels_for(a, b);
  const dim3 grid(nb, N, norm_chunks(C / 4));
  void* args1[2] = {&p[0], &p[1]};      // (a single's kernel takes one argument: the address of the unfilled second block is never read)
  void* args2[2] = {&q[0], &q[1]};
  (void)hipLaunchKernel(ks.k1, grid, dim3(256), args1, 0, st);
  rc = check_launch(ks.name1);
  if (rc) return rc;
  for (int k = 0; k < nn; ++k)
    hipLaunchKernelGGL(norm_bwd_finalize_kernel, dim3((N * C * 16 + 255) / 256), dim3(256), 0, st, p[k].part, N, nb, C, HW, const_cast<float*>(q[k].m1),
                       const_cast<float*>(q[k].m2));
  rc = check_launch("norm_bwd_finalize_kernel");
  if (rc) return rc;
  (void)hipLaunchKernel(ks.k2, grid, dim3(256), args2, 0, st);
  rc = check_launch(ks.name2);
  if (rc) return rc;
  for (int k = 0; k < nn; ++k)
    if (ds[k]->noise_z && ds[k]->dnoise_scale) {
      hipLaunchKernelGGL(sum_rows_kernel<>, dim3((C + 15) / 16), dim3(256), 0, st, p[k].part, N * nb, C, ds[k]->dnoise_scale, ds[k]->dns_accumulate);
      rc = check_launch("sum_rows_kernel");
    }
  return rc;
}

extern "C" int hrv_spade_norm_bwd_nhwc_f32(const hrv_norm_bwd_t* d, hrv_stream_t stream) {
  return norm_bwd_launch(d, nullptr, (hipStream_t)stream);
}

extern "C" int hrv_spade_norm_bwd2_nhwc_f32(const hrv_norm_bwd_t* a, const hrv_norm_bwd_t* b, hrv_stream_t stream) {
  const int rc = norm_bwd_pair_check(a, b);
  return rc ? rc : norm_bwd_launch(a, b, (hipStream_t)stream);
}
