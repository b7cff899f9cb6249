// Fused loss head of the PatchGAN's discriminator step (ABI and record layout: include/hrviton_hip.h): the hinge terms of D_Fake /
// D_Real, the logit statistics (means, ADA's r_t = E[sign D(real)]), the LeCam anchors and regulariser (Tseng et al., CVPR 2021) and
// all four gradients, for every scale, in three launches.  Everything is decided on the device: no host read, capturable.
//   dhead_reduce_kernel    one launch, grid (DHEAD_SLOTS, 2 * num_d): block (b, q) is slot b of half q & 1 (0 fake, 1 real) of scale
//                          q >> 1 -> fp64 partials {sum x, sum x^2, sum hinge, non-finite count, sum sign}
//   dhead_finalize_kernel  one block: partials -> sums -> means, anchor update (BEFORE use), r_t, count, lambda_eff, the three losses
//   dhead_grad_kernel      one launch, grid (blocks, 2 * num_d): hinge + regulariser gradient of every logit, reading the record and
//                          the three upstream scalars from device memory
// The regulariser's VALUE needs the updated anchors, which need the means, which need the whole reduce pass.  Form `paper`: closed
// form from sum x and sum x^2, R_r = (sum x_r^2 - 2 a_F sum x_r + n a_F^2) / n, no second pass.  Form `relu` is not polynomial in
// the anchor: the finalize block makes a second pass over the logits itself (they are in L2), and only when lambda_eff != 0 -- a second
// accumulator in the reduce pass would have to use the anchors of the step before, which is not the published order.
// Determinism as in grad_guard.hip: the slot count is a compile-time constant (never the CU count), block b IS slot b, the
// element -> thread rule depends only on (pointer alignment, n), and every sum has a fixed order: per thread over its trips in turn
// (then its head and tail element, slot 0 only), a 64-lane shuffle tree, the waves through LDS in wave order, the slots in a 64-lane
// shuffle tree.  No atomics.  All sums are fp64.
#include "hrv_common.h"

namespace hrv {

constexpr int DHEAD_SLOTS = HRV_DHEAD_SLOTS;
constexpr int DHEAD_BLOCK = 256;
constexpr int DHEAD_FIN_BLOCK = 1024;
constexpr int DHEAD_VALS = 5;      // per (scale, half, slot): sum x, sum x^2, sum hinge, non-finite count, sum sign (real half)
static_assert(DHEAD_SLOTS == 64, "the slot tree of dhead_finalize_kernel is one 64-lane shuffle tree");

struct dhead_desc_t {
  const float* x[HRV_DHEAD_MAX_SCALES][2];      // [scale][0 fake | 1 real]
  float* dx[HRV_DHEAD_MAX_SCALES][2];           // (backward only)
  long long n[HRV_DHEAD_MAX_SCALES];
  int num_d;
};

struct dhead_acc_t {
  double v[DHEAD_VALS];
};

__device__ __forceinline__ bool dhead_nonfinite(float x) { return (__builtin_bit_cast(unsigned, x) & 0x7f800000u) == 0x7f800000u; }

template <bool REAL>
__device__ __forceinline__ void dhead_acc(float xf, dhead_acc_t& a) {
  const double x = (double)xf;
  a.v[0] += x;
  a.v[1] += x * x;
  const double h = REAL ? 1.0 - x : 1.0 + x;
  a.v[2] += h > 0.0 ? h : (h != h ? h : 0.0);      // max(h, 0) that keeps a NaN
  a.v[3] += dhead_nonfinite(xf) ? 1.0 : 0.0;
  if (REAL) a.v[4] += x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0);
}

// the values of the block's threads -> thread 0, fixed order: shuffle tree inside each wave, then the waves in turn
template <int NV, int THREADS>
__device__ __forceinline__ void dhead_block_reduce(double* v, double (*red)[THREADS / 64]) {
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_down(v[j], o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int j = 0; j < NV; ++j) red[j][wave] = v[j];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      v[j] = red[j][0];
#pragma unroll
      for (int k = 1; k < THREADS / 64; ++k) v[j] += red[j][k];
    }
  __syncthreads();
}

// x[0, head) scalar | n4 float4 groups from the first 16-byte boundary | the scalar tail up to n (the guard kernel's split)
__device__ __forceinline__ void dhead_split(const float* x, size_t n, size_t& head, size_t& n4) {
  head = ((16 - ((uintptr_t)x & 15)) & 15) / 4;
  if (head > n) head = n;
  n4 = (n - head) / 4;
}

// Group i belongs to thread i mod (DHEAD_SLOTS * 256) of its half's row of the grid; head and tail elements (at most 3 each) to
// threads 0..2 of slot 0.
__global__ __launch_bounds__(DHEAD_BLOCK) void dhead_reduce_kernel(dhead_desc_t d, double* __restrict__ part) {
  __shared__ double red[DHEAD_VALS][DHEAD_BLOCK / 64];
  const int q = blockIdx.y, k = q >> 1, half = q & 1;
  const float* __restrict__ x = d.x[k][half];
  const size_t n = (size_t)d.n[k];
  size_t head, n4;
  dhead_split(x, n, head, n4);
  const f32x4* __restrict__ body = reinterpret_cast<const f32x4*>(x + head);
  const size_t stride = (size_t)DHEAD_SLOTS * DHEAD_BLOCK;
  dhead_acc_t a;
#pragma unroll
  for (int j = 0; j < DHEAD_VALS; ++j) a.v[j] = 0.0;
  auto acc = [&](float v) {
    if (half) dhead_acc<true>(v, a);
    else dhead_acc<false>(v, a);
  };
  for (size_t i = (size_t)blockIdx.x * DHEAD_BLOCK + threadIdx.x; i < n4; i += stride) {
    const f32x4 v = body[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc(v[e]);
  }
  if (blockIdx.x == 0) {
    const size_t t = threadIdx.x, tail0 = head + 4 * n4;
    if (t < head) acc(x[t]);
    if (tail0 + t < n) acc(x[tail0 + t]);
  }
  dhead_block_reduce<DHEAD_VALS, DHEAD_BLOCK>(a.v, red);
  if (threadIdx.x == 0) {
    double* p = part + ((size_t)q * DHEAD_SLOTS + blockIdx.x) * DHEAD_VALS;
#pragma unroll
    for (int j = 0; j < DHEAD_VALS; ++j) p[j] = a.v[j];
  }
}

// stage bit 0: partials -> the sums of the record; bit 1: sums -> everything else.  (Data parallel: the caller all-reduces the sums
// between a launch with bit 0 and one with bit 1 and passes n_mult = world, so that means and anchors are the global batch's.)
__global__ __launch_bounds__(DHEAD_FIN_BLOCK) void dhead_finalize_kernel(dhead_desc_t d, const double* __restrict__ part, int form,
                                                                        double weight, double decay, int start, int n_mult,
                                                                        int stage, double* __restrict__ rec, float* __restrict__ losses) {
#pragma clang fp contract(off)      // the anchor update is d * a + (1 - d) * m with both products rounded, as a host restatement has it
  __shared__ double red[1][DHEAD_FIN_BLOCK / 64];
  __shared__ double sh_anchor[HRV_DHEAD_MAX_SCALES][2];
  __shared__ double sh_reg[HRV_DHEAD_MAX_SCALES];
  __shared__ int sh_second;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (stage & 1) {
    // quantity (q, j): the 64 slots in one shuffle tree; the 16 waves take the quantities in turn
    for (int item = wave; item < 2 * d.num_d * DHEAD_VALS; item += DHEAD_FIN_BLOCK / 64) {
      const int q = item / DHEAD_VALS, j = item % DHEAD_VALS;
      double s = part[((size_t)q * DHEAD_SLOTS + lane) * DHEAD_VALS + j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
      if (lane == 0) {
        const int k = q >> 1, half = q & 1;
        double* sums = rec + HRV_DHEAD_SUMS + HRV_DHEAD_SCALE_WORDS * k;
        if (j == 0) sums[half ? HRV_DHEAD_SUM_REAL : HRV_DHEAD_SUM_FAKE] = s;
        else if (j == 1) sums[half ? HRV_DHEAD_SUMSQ_REAL : HRV_DHEAD_SUMSQ_FAKE] = s;
        else if (j == 2) sums[half ? HRV_DHEAD_HINGE_REAL : HRV_DHEAD_HINGE_FAKE] = s;
        else if (j == 4) { if (half) sums[HRV_DHEAD_SIGN_REAL] = s; }
      }
    }
    __syncthreads();      // (the two non-finite counts of a scale land in one word: after the barrier, one thread per scale)
    if ((int)threadIdx.x < d.num_d) {
      const int k = threadIdx.x;
      double c = 0.0;
      for (int half = 0; half < 2; ++half)
        for (int b = 0; b < DHEAD_SLOTS; ++b) c += part[((size_t)(2 * k + half) * DHEAD_SLOTS + b) * DHEAD_VALS + 3];
      rec[HRV_DHEAD_SUMS + HRV_DHEAD_SCALE_WORDS * k + HRV_DHEAD_NONFINITE_K] = c;
    }
    __threadfence_block();
    __syncthreads();
  }
  if (!(stage & 2)) return;
  double lam = 0.0, hinge_f = 0.0, hinge_r = 0.0, reg = 0.0;
  bool poisoned = false;
  if (threadIdx.x == 0) {
    double bad = 0.0;
    for (int k = 0; k < d.num_d; ++k) bad += rec[HRV_DHEAD_SUMS + HRV_DHEAD_SCALE_WORDS * k + HRV_DHEAD_NONFINITE_K];
    poisoned = bad != 0.0;
    const double count = rec[HRV_DHEAD_COUNT];
    lam = count >= (double)start ? weight : 0.0;
    const double dd = count == 0.0 ? 0.0 : decay;
    for (int k = 0; k < d.num_d; ++k) {
      const double* sums = rec + HRV_DHEAD_SUMS + HRV_DHEAD_SCALE_WORDS * k;
      double* st = rec + HRV_DHEAD_STATE + HRV_DHEAD_SCALE_WORDS * k;
      const double nt = (double)d.n[k] * (double)n_mult;
      const double m_r = sums[HRV_DHEAD_SUM_REAL] / nt, m_f = sums[HRV_DHEAD_SUM_FAKE] / nt, r = sums[HRV_DHEAD_SIGN_REAL] / nt;
      double a_r = st[HRV_DHEAD_ANCHOR_REAL], a_f = st[HRV_DHEAD_ANCHOR_FAKE];
      if (!poisoned) {
        a_r = dd * a_r + (1.0 - dd) * m_r;
        a_f = dd * a_f + (1.0 - dd) * m_f;
        st[HRV_DHEAD_ANCHOR_REAL] = a_r;
        st[HRV_DHEAD_ANCHOR_FAKE] = a_f;
        st[HRV_DHEAD_RT_AVG] = dd * st[HRV_DHEAD_RT_AVG] + (1.0 - dd) * r;
      }
      st[HRV_DHEAD_RT] = r;
      st[HRV_DHEAD_MEAN_REAL] = m_r;
      st[HRV_DHEAD_MEAN_FAKE] = m_f;
      hinge_r += sums[HRV_DHEAD_HINGE_REAL] / nt;
      hinge_f += sums[HRV_DHEAD_HINGE_FAKE] / nt;
      double rk = 0.0;
      if (form == HRV_DHEAD_FORM_PAPER)
        rk = (sums[HRV_DHEAD_SUMSQ_REAL] - 2.0 * a_f * sums[HRV_DHEAD_SUM_REAL] + nt * (a_f * a_f)) / nt +
             (sums[HRV_DHEAD_SUMSQ_FAKE] - 2.0 * a_r * sums[HRV_DHEAD_SUM_FAKE] + nt * (a_r * a_r)) / nt;
      sh_reg[k] = rk;
      sh_anchor[k][0] = a_r;
      sh_anchor[k][1] = a_f;
    }
    sh_second = (form == HRV_DHEAD_FORM_RELU && lam != 0.0 && !poisoned) ? 1 : 0;
    rec[HRV_DHEAD_COUNT] = poisoned ? count : count + 1.0;
    rec[HRV_DHEAD_NONFINITE] = bad;
    rec[HRV_DHEAD_LAMBDA] = lam;
    rec[HRV_DHEAD_STEPS] += 1.0;
  }
  __syncthreads();
  if (sh_second) {      // relu: sum relu(x_r - a_F)^2 + sum relu(a_R - x_f)^2 over this process's logits, the whole block per scale
    for (int k = 0; k < d.num_d; ++k) {
      const size_t n = (size_t)d.n[k];
      const double a_r = sh_anchor[k][0], a_f = sh_anchor[k][1];
      double s = 0.0;
      for (int half = 0; half < 2; ++half) {
        const float* __restrict__ x = d.x[k][half];
        size_t head, n4;
        dhead_split(x, n, head, n4);
        const f32x4* __restrict__ body = reinterpret_cast<const f32x4*>(x + head);
        auto acc = [&](float v) {
          const double t = half ? (double)v - a_f : a_r - (double)v;
          s += t > 0.0 ? t * t : 0.0;
        };
        for (size_t i = threadIdx.x; i < n4; i += DHEAD_FIN_BLOCK) {
          const f32x4 v = body[i];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc(v[e]);
        }
        const size_t t = threadIdx.x, tail0 = head + 4 * n4;
        if (t < head) acc(x[t]);
        if (tail0 + t < n) acc(x[tail0 + t]);
      }
      dhead_block_reduce<1, DHEAD_FIN_BLOCK>(&s, red);
      if (threadIdx.x == 0) sh_reg[k] = s / (double)n;
    }
  }
  if (threadIdx.x != 0) return;
  for (int k = 0; k < d.num_d; ++k) {
    rec[HRV_DHEAD_STATE + HRV_DHEAD_SCALE_WORDS * k + HRV_DHEAD_REG_K] = sh_reg[k];
    reg += sh_reg[k];
  }
  const double nd = (double)d.num_d;
  reg = reg / nd;
  rec[HRV_DHEAD_REG] = reg;
  losses[0] = (float)(hinge_f / nd);
  losses[1] = (float)(hinge_r / nd);
  // a poisoned step reports a NaN regulariser whatever the weight: the statistics it would have used are not trustworthy
  losses[2] = poisoned ? __builtin_nanf("") : (lam != 0.0 ? (float)(lam * reg) : 0.f);
}

// d(sum_k (D_Fake + D_Real + D_LeCam)) / d(logit).  Hinge part in fp32, (+-1 * 1/n) * (g_out / num_d) in that order -- the bits of
// loss_kernel followed by scale_kernel under GANLoss's  / num_D ; regulariser part in fp64, added to it and rounded once.
__global__ __launch_bounds__(DHEAD_BLOCK) void dhead_grad_kernel(dhead_desc_t d, int form, const double* __restrict__ rec,
                                                                const float* __restrict__ g_fake, const float* __restrict__ g_real,
                                                                const float* __restrict__ g_lecam) {
  const int q = blockIdx.y, k = q >> 1, half = q & 1;
  const float* __restrict__ x = d.x[k][half];
  float* __restrict__ dx = d.dx[k][half];
  const size_t n = (size_t)d.n[k];
  const float inv_n = (float)(1.0 / (double)n);
  const float gh = (half ? g_real[0] : g_fake[0]) / (float)d.num_d;
  const double lam = rec[HRV_DHEAD_LAMBDA];
  // (the anchor of the OTHER half: real logits are pulled towards the fake anchor and the other way round)
  const double anchor = rec[HRV_DHEAD_STATE + HRV_DHEAD_SCALE_WORDS * k + (half ? HRV_DHEAD_ANCHOR_FAKE : HRV_DHEAD_ANCHOR_REAL)];
  const double c = ((double)(g_lecam[0] / (float)d.num_d) * lam) * 2.0 / (double)n;
  for (size_t i = (size_t)blockIdx.x * DHEAD_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * DHEAD_BLOCK) {
    const float v = x[i];
    const float sg = half ? (v < 1.f ? -1.f : 0.f) : (v > -1.f ? 1.f : 0.f);
    const float h = (sg * inv_n) * gh;
    if (lam == 0.0) {
      dx[i] = h;
    } else {
      double t = (double)v - anchor;
      if (form == HRV_DHEAD_FORM_RELU) t = half ? (t > 0.0 ? t : 0.0) : (t < 0.0 ? t : 0.0);
      dx[i] = (float)((double)h + c * t);
    }
  }
}

static int dhead_fill(dhead_desc_t& d, int num_d, const float* const* xf, const float* const* xr, const int64_t* n,
                      float* const* df, float* const* dr) {
  if (!(num_d >= 1 && num_d <= HRV_DHEAD_MAX_SCALES && xf && xr && n)) return 0;
  d.num_d = num_d;
  for (int k = 0; k < HRV_DHEAD_MAX_SCALES; ++k) {
    const bool on = k < num_d;
    d.x[k][0] = on ? xf[k] : nullptr;
    d.x[k][1] = on ? xr[k] : nullptr;
    d.dx[k][0] = (on && df) ? df[k] : nullptr;
    d.dx[k][1] = (on && dr) ? dr[k] : nullptr;
    d.n[k] = on ? (long long)n[k] : 0;
    if (on && !(d.x[k][0] && d.x[k][1] && n[k] >= 1 && ((uintptr_t)d.x[k][0] & 3) == 0 && ((uintptr_t)d.x[k][1] & 3) == 0)) return 0;
    if (on && df && !(d.dx[k][0] && d.dx[k][1] && ((uintptr_t)d.dx[k][0] & 3) == 0 && ((uintptr_t)d.dx[k][1] & 3) == 0)) return 0;
  }
  return 1;
}

}  // namespace hrv

using namespace hrv;

extern "C" int hrv_dhead_forward_f32(int32_t num_d, const float* const* x_fake, const float* const* x_real, const int64_t* n,
                                     int32_t form, double weight, double decay, int32_t start, int32_t n_mult, int32_t stage,
                                     double* part, double* record, float* losses, hrv_stream_t stream) {
  dhead_desc_t d;
  HRV_REQUIRE(dhead_fill(d, num_d, x_fake, x_real, n, nullptr, nullptr),
              "dhead_forward: 1..%d scales, non-null 4-byte-aligned logit pointers and n >= 1 per scale", HRV_DHEAD_MAX_SCALES);
  HRV_REQUIRE((form == HRV_DHEAD_FORM_PAPER || form == HRV_DHEAD_FORM_RELU) && weight >= 0.0 && decay >= 0.0 && decay < 1.0 &&
                  start >= 0 && n_mult >= 1 && stage >= 1 && stage <= 7,
              "dhead_forward: bad form / weight / decay / start / n_mult / stage");
  HRV_REQUIRE(part && record && ((uintptr_t)part & 7) == 0 && ((uintptr_t)record & 7) == 0 && (losses || !(stage & 4)),
              "dhead_forward: null or misaligned partials / record / losses");
  if (stage & 1) {
    hipLaunchKernelGGL(dhead_reduce_kernel, dim3(DHEAD_SLOTS, 2 * num_d), dim3(DHEAD_BLOCK), 0, (hipStream_t)stream, d, part);
    const int rc = check_launch("dhead_reduce_kernel");
    if (rc != HRV_OK) return rc;
  }
  if (!(stage & 6)) return HRV_OK;
  hipLaunchKernelGGL(dhead_finalize_kernel, dim3(1), dim3(DHEAD_FIN_BLOCK), 0, (hipStream_t)stream, d, (const double*)part, (int)form,
                     weight, decay, (int)start, (int)n_mult, (int)(stage >> 1), record, losses);
  return check_launch("dhead_finalize_kernel");
}

extern "C" int hrv_dhead_backward_f32(int32_t num_d, const float* const* x_fake, const float* const* x_real, const int64_t* n,
                                      int32_t form, const double* record, const float* g_fake, const float* g_real,
                                      const float* g_lecam, float* const* d_fake, float* const* d_real, hrv_stream_t stream) {
  dhead_desc_t d;
  HRV_REQUIRE(d_fake && d_real && dhead_fill(d, num_d, x_fake, x_real, n, d_fake, d_real),
              "dhead_backward: 1..%d scales, non-null 4-byte-aligned logit / gradient pointers and n >= 1 per scale",
              HRV_DHEAD_MAX_SCALES);
  HRV_REQUIRE((form == HRV_DHEAD_FORM_PAPER || form == HRV_DHEAD_FORM_RELU) && record && ((uintptr_t)record & 7) == 0 && g_fake &&
                  g_real && g_lecam,
              "dhead_backward: bad form, or null record / upstream scalars");
  int64_t nmax = 1;
  for (int k = 0; k < num_d; ++k) nmax = n[k] > nmax ? n[k] : nmax;
  const int64_t gx = (nmax + DHEAD_BLOCK - 1) / DHEAD_BLOCK;
  hipLaunchKernelGGL(dhead_grad_kernel, dim3((unsigned)(gx > 256 ? 256 : gx), 2 * num_d), dim3(DHEAD_BLOCK), 0, (hipStream_t)stream, d,
                     (int)form, record, g_fake, g_real, g_lecam);
  return check_launch("dhead_grad_kernel");
}
