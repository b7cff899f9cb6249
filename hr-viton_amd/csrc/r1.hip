// R1 gradient penalty of the PatchGAN by a tangent pass (ABI and the closed form: include/hrviton_hip.h).
//   instnorm_jvp_partial_kernel   five fp64 sums per (sample, channel, pixel slab) over c, f, t, df
//   instnorm_jvp_reduce_kernel    slab partials -> record [N][C][5], one wave per (n, c), fixed order
//   instnorm_jvp_bwd_kernel       the element-wise pass: tbar and cbar from the record
//   r1_seed_kernel / r1_seed_finalize_kernel   tangent v and ||g_n||^2 of the image channels, penalty and loss on the device
// HBM-bound.  The InstanceNorm kernels: one float4 per lane and tensor, wavefront-contiguous channel groups, the geometry of norm.hip
// (grid = pixel slabs x samples x channel chunks).  The seed kernel: one PIXEL per lane, its Cp / 4 float4 groups in turn -- adjacent
// lanes are Cp * 4 bytes apart (48 here), every byte of a line is still used by the wave; it runs once per phase over a 12-channel
// tensor.  Every sum is fp64 and has one order that depends on (H * W, C) alone; no atomics.
#include "hrv_common.h"

namespace hrv {

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct JvpGeom {
  int HW, PB, p0, p1, GB, R, r, gl, g;
  bool active;
};

// block (slab b, sample n, chunk z) -> pixel range and this thread's (pixel row, channel group)
__device__ __forceinline__ JvpGeom jvp_geom(const hrv_instnorm_jvp_t& d, int NB) {
  JvpGeom q;
  const int C4 = d.C >> 2;
  q.HW = d.H * d.W;
  q.PB = (q.HW + NB - 1) / NB;
  q.p0 = blockIdx.x * q.PB;
  q.p1 = min(q.p0 + q.PB, q.HW);
  q.GB = C4 < NORM_GCAP ? C4 : NORM_GCAP;
  q.R = 256 / q.GB;
  q.r = threadIdx.x / q.GB;
  q.gl = threadIdx.x - q.r * q.GB;
  q.g = blockIdx.z * q.GB + q.gl;
  q.active = q.r < q.R && q.g < C4;
  return q;
}

__device__ __forceinline__ f64x4 widen(f32x4 v) { return __builtin_convertvector(v, f64x4); }

// y and q = lrelu'(f) * df of one channel group at one pixel, in fp64
__device__ __forceinline__ void jvp_yq(const hrv_instnorm_jvp_t& d, size_t pix, int g, f64x4 mu, f64x4 rs, f64x4& y, f64x4& q) {
  const f32x4 xv = ld4(d.x + pix * d.x_cstride + d.x_coff + g * 4);
  const f32x4 fv = ld4(d.f + pix * d.f_cstride + d.f_coff + g * 4);
  const f32x4 dv = ld4(d.df + pix * d.df_cstride + d.df_coff + g * 4);
  y = (widen(xv) - mu) * rs;
  const double sl = (double)d.slope;
#pragma unroll
  for (int e = 0; e < 4; ++e) q[e] = fv[e] > 0.f ? (double)dv[e] : sl * (double)dv[e];
}

__global__ __launch_bounds__(256) void instnorm_jvp_partial_kernel(const hrv_instnorm_jvp_t d, int NB) {
  __shared__ f64x4 red[256];
  const JvpGeom G = jvp_geom(d, NB);
  const int n = blockIdx.y;
  f64x4 s[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) s[k] = (f64x4)(0.0);
  if (G.active) {
    const f64x4 mu = widen(ld4(d.mean + (size_t)n * d.C + G.g * 4));
    const f64x4 rs = widen(ld4(d.rstd + (size_t)n * d.C + G.g * 4));
    for (int px = G.p0 + G.r; px < G.p1; px += G.R) {      // ONE chain per thread, in pixel order
      const size_t pix = (size_t)n * G.HW + px;
      f64x4 y, q;
      jvp_yq(d, pix, G.g, mu, rs, y, q);
      const f64x4 t = widen(ld4(d.t + pix * d.t_cstride + d.t_coff + G.g * 4));
      s[0] += q;
      s[1] += t;
      s[2] += y * q;
      s[3] += y * t;
      s[4] += q * t;
    }
  }
  // rows 1 .. R-1 into row 0 in row order, one statistic at a time (8 KiB of LDS instead of 40)
  double* dst = d.workspace + (((size_t)n * NB + blockIdx.x) * d.C + (size_t)G.g * 4) * 5;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    __syncthreads();
    red[threadIdx.x] = s[k];
    __syncthreads();
    if (G.active && G.r == 0) {
      f64x4 a = s[k];
      for (int rr = 1; rr < G.R; ++rr) a += red[rr * G.GB + G.gl];
#pragma unroll
      for (int e = 0; e < 4; ++e) dst[e * 5 + k] = a[e];
    }
  }
}

// one WAVE per (n, c): lane l sums slabs l, l + 64, ... of each statistic, then a fixed butterfly
__global__ __launch_bounds__(256) void instnorm_jvp_reduce_kernel(const double* __restrict__ part, int N, int NB, int C,
                                                                  double* __restrict__ record) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= N * C) return;
  const int n = i / C, c = i - n * C;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = lane; b < NB; b += 64) {
    const double* src = part + (((size_t)n * NB + b) * C + c) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k] += src[k];
  }
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
  if (lane != 0) return;
#pragma unroll
  for (int k = 0; k < 5; ++k) record[(size_t)i * 5 + k] = s[k];
}

__global__ __launch_bounds__(256) void instnorm_jvp_bwd_kernel(const hrv_instnorm_jvp_t d, int NB) {
  const JvpGeom G = jvp_geom(d, NB);
  const int n = blockIdx.y;
  if (!G.active) return;
  const f64x4 mu = widen(ld4(d.mean + (size_t)n * d.C + G.g * 4));
  const f64x4 rs = widen(ld4(d.rstd + (size_t)n * d.C + G.g * 4));
  const double P = (double)G.HW;
  f64x4 mq, mt, myq, myt, k1, mw, myw;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double* rec = d.record + ((size_t)n * d.C + G.g * 4 + e) * 5;
    mq[e] = rec[0] / P;
    mt[e] = rec[1] / P;
    myq[e] = rec[2] / P;
    myt[e] = rec[3] / P;
    const double A = rec[4] - P * mq[e] * mt[e];
    const double B = P * myq[e] * myt[e];
    k1[e] = (A - B) / P;
    mw[e] = mq[e] * myt[e] + mt[e] * myq[e];
    myw[e] = 2.0 * myq[e] * myt[e];
  }
  const f64x4 rs2 = rs * rs;
  for (int px = G.p0 + G.r; px < G.p1; px += G.R) {
    const size_t pix = (size_t)n * G.HW + px;
    f64x4 y, q;
    jvp_yq(d, pix, G.g, mu, rs, y, q);
    const f64x4 t = widen(ld4(d.t + pix * d.t_cstride + d.t_coff + G.g * 4));
    const f64x4 tb = rs * (q - mq - y * myq);
    const f64x4 w = q * myt + t * myq;
    f64x4 cb = -(rs2 * k1) * y - rs2 * (w - mw - y * myw);
    if (d.cin) cb += widen(ld4(d.cin + pix * d.cin_cstride + d.cin_coff + G.g * 4));
    *reinterpret_cast<f32x4*>(d.tbar + pix * d.tbar_cstride + d.tbar_coff + G.g * 4) = __builtin_convertvector(tb, f32x4);
    *reinterpret_cast<f32x4*>(d.cbar + pix * d.cbar_cstride + d.cbar_coff + G.g * 4) = __builtin_convertvector(cb, f32x4);
  }
}

// ---- the seed -------------------------------------------------------------------------------------------------------------------
constexpr int R1_SLOTS = 64;      // per sample; a compile-time constant (never the CU count)

// block (slot s, sample n): pixels s * 256 + tid, + R1_SLOTS * 256, ...; every channel group of its pixel in turn
__global__ __launch_bounds__(256) void r1_seed_kernel(const float* __restrict__ din, int HW, int Cp, int Ca, int Cb, float inv_n,
                                                     float* __restrict__ v, double* __restrict__ part) {
  __shared__ double red[4];
  const int n = blockIdx.y;
  const int C4 = Cp >> 2;
  double s = 0.0;
  for (int px = blockIdx.x * 256 + threadIdx.x; px < HW; px += R1_SLOTS * 256) {
    const size_t base = ((size_t)n * HW + px) * Cp;
    for (int g = 0; g < C4; ++g) {
      const f32x4 x = ld4(din + base + g * 4);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = g * 4 + e;
        const bool img = c >= Ca && c < Ca + Cb;
        o[e] = img ? x[e] * inv_n : 0.f;      // a select: what a parse or pad channel holds never reaches v or the sum
        const double xd = img ? (double)x[e] : 0.0;
        s += xd * xd;
      }
      *reinterpret_cast<f32x4*>(v + base + g * 4) = o;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)n * R1_SLOTS + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(64) void r1_seed_finalize_kernel(const double* __restrict__ part, int N, float gamma,
                                                            double* __restrict__ sums, float* __restrict__ out) {
  double total = 0.0;
  for (int n = 0; n < N; ++n) {
    double s = part[(size_t)n * R1_SLOTS + threadIdx.x];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (threadIdx.x == 0) sums[n] = s;
    total += s;
  }
  if (threadIdx.x == 0) {
    const double pen = total / (double)N;
    out[0] = (float)pen;
    out[1] = (float)(0.5 * (double)gamma * pen);
  }
}

// stats entry point: needs the workspace; element-wise entry point (`outputs`): needs tbar / cbar, ignores the workspace
static int jvp_check(const hrv_instnorm_jvp_t* d, const char* what, bool outputs) {
  HRV_REQUIRE(d, "%s: null descriptor", what);
  HRV_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->C % 4 == 0 && (int64_t)d->H * d->W < (1ll << 31), "%s: bad extents",
              what);
  HRV_REQUIRE(d->x && d->mean && d->rstd && d->f && d->t && d->df && d->record && (outputs || d->workspace), "%s: null operand", what);
  auto view_ok = [&](const void* p, int cs, int co) {
    return ((uintptr_t)p & 15) == 0 && cs % 4 == 0 && co % 4 == 0 && co >= 0 && co + d->C <= cs;
  };
  HRV_REQUIRE(view_ok(d->x, d->x_cstride, d->x_coff) && view_ok(d->f, d->f_cstride, d->f_coff) && view_ok(d->t, d->t_cstride, d->t_coff) &&
                  view_ok(d->df, d->df_cstride, d->df_coff) && ((uintptr_t)d->mean & 15) == 0 && ((uintptr_t)d->rstd & 15) == 0 &&
                  ((uintptr_t)d->record & 7) == 0 && ((uintptr_t)d->workspace & 7) == 0,
              "%s: every tensor is a 16-byte aligned channel slice [coff, coff + C) with coff, cstride multiples of 4", what);
  if (outputs) {
    HRV_REQUIRE(d->tbar && d->cbar && view_ok(d->tbar, d->tbar_cstride, d->tbar_coff) && view_ok(d->cbar, d->cbar_cstride, d->cbar_coff) &&
                    (!d->cin || view_ok(d->cin, d->cin_cstride, d->cin_coff)),
                "%s: bad tbar / cbar / cin view", what);
    const void* ins[] = {d->x, d->f, d->t, d->df, d->cin};
    for (const void* p : ins) HRV_REQUIRE(p != d->tbar && p != d->cbar, "%s: tbar / cbar must not alias an input", what);
    HRV_REQUIRE((const void*)d->tbar != (const void*)d->cbar || d->tbar_coff + d->C <= d->cbar_coff || d->cbar_coff + d->C <= d->tbar_coff,
                "%s: tbar and cbar overlap", what);
  }
  return HRV_OK;
}

}  // namespace hrv

using namespace hrv;

extern "C" int64_t hrv_instnorm_jvp_workspace_elems(int32_t N, int32_t H, int32_t W, int32_t C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
  return (int64_t)N * norm_slabs(H * W) * ((C + 3) / 4 * 4) * 5;
}

extern "C" int hrv_instnorm_jvp_stats_nhwc_f32(const hrv_instnorm_jvp_t* d, hrv_stream_t stream) {
  if (int rc = jvp_check(d, "instnorm_jvp_stats", false)) return rc;
  const int NB = norm_slabs(d->H * d->W);
  const dim3 grid(NB, d->N, norm_chunks(d->C / 4));
  hipLaunchKernelGGL(instnorm_jvp_partial_kernel, grid, dim3(256), 0, (hipStream_t)stream, *d, NB);
  if (int rc = check_launch("instnorm_jvp_partial_kernel")) return rc;
  hipLaunchKernelGGL(instnorm_jvp_reduce_kernel, dim3((d->N * d->C + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                     (const double*)d->workspace, d->N, NB, d->C, d->record);
  return check_launch("instnorm_jvp_reduce_kernel");
}

extern "C" int hrv_instnorm_jvp_bwd_nhwc_f32(const hrv_instnorm_jvp_t* d, hrv_stream_t stream) {
  if (int rc = jvp_check(d, "instnorm_jvp_bwd", true)) return rc;
  const int NB = norm_slabs(d->H * d->W);
  const dim3 grid(NB, d->N, norm_chunks(d->C / 4));
  hipLaunchKernelGGL(instnorm_jvp_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, *d, NB);
  return check_launch("instnorm_jvp_bwd_kernel");
}

extern "C" int hrv_r1_seed_slots(void) { return R1_SLOTS; }

extern "C" int hrv_r1_seed_nhwc_f32(const float* d_in, int32_t N, int32_t H, int32_t W, int32_t Cp, int32_t Ca, int32_t Cb, float gamma,
                                    float* v, double* part, double* sums, float* out, hrv_stream_t stream) {
  HRV_REQUIRE(d_in && v && part && sums && out && d_in != v, "r1_seed: null or aliased operand");
  HRV_REQUIRE(N > 0 && H > 0 && W > 0 && Cp > 0 && Cp % 4 == 0 && Ca >= 0 && Cb > 0 && Ca + Cb <= Cp && (int64_t)H * W < (1ll << 31),
              "r1_seed: bad extents (N=%d H=%d W=%d Cp=%d Ca=%d Cb=%d)", N, H, W, Cp, Ca, Cb);
  HRV_REQUIRE(((uintptr_t)d_in & 15) == 0 && ((uintptr_t)v & 15) == 0 && ((uintptr_t)part & 7) == 0 && ((uintptr_t)sums & 7) == 0,
              "r1_seed: misaligned operand");
  hipLaunchKernelGGL(r1_seed_kernel, dim3(R1_SLOTS, N), dim3(256), 0, (hipStream_t)stream, d_in, H * W, Cp, Ca, Cb, 1.0f / (float)N, v, part);
  if (int rc = check_launch("r1_seed_kernel")) return rc;
  hipLaunchKernelGGL(r1_seed_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)part, N, gamma, sums, out);
  return check_launch("r1_seed_finalize_kernel");
}
