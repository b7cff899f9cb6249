// Nearest-neighbour manifold statistics over banks of Inception features for evaluate.py's --prdc (improved precision / recall,
// density / coverage) on gfx950, in float64 on squared Euclidean distances:
//   - the squared norm of every row of an fp32 bank;
//   - a block of squared distances out[i][j] = max(0, |x_i|^2 + |y_j|^2 - 2 x_i . y_j), the dot products on
//     v_mfma_f64_16x16x4_f64 (the tile loop of feat_stats.hip's GEMM, restated), a row's own entry replaced by +inf on request;
//   - the k-th smallest of every row of such a block (the k-nearest-neighbour radius);
//   - per row the number of entries below a per-column radius, and the row minimum.
// No atomics, no split-K: every output element is the work of one wave (or one thread of one block) walking its row (or k) in a
// fixed order, so results do not depend on the grid and are bit-identical from run to run.
#include "hrv_common.h"

namespace hrv {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int ROWS_PER_BLOCK = 4;      // the row kernels: a wave per row, 4 waves per block
constexpr int KTH_MAX = 16;            // hrv_row_kth_max()

// the wave's 64 values meet in a fixed butterfly: 32, 16, 8, 4, 2, 1 lanes apart; every lane ends with the result
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------- squared row norms
// out[i] = sum_c (double)x[i][c]^2: lane l adds the squares of columns l, l + 64, ... in ascending order, then the butterfly
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void row_sqnorm_kernel(const float* __restrict__ x, int n, int D, int64_t ld,
                                                                         double* __restrict__ out) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= n) return;      // (uniform over the wave; no barrier in this kernel)
  const float* p = x + (int64_t)row * ld;
  double s = 0.0;
  for (int c = lane; c < D; c += 64) {
    const double v = (double)p[c];
    s += v * v;
  }
  s = wave_sum(s);
  if (lane == 0) out[row] = s;
}

// ---------------------------------------------------------------- squared distances, X [nx][D] against Y [ny][D]
// The dot products: feat_stats.hip's gemm_nt_f64_kernel for fp32 operands.  A block of 256 threads (4 waves, 2 x 2) owns a 64 x 64
// tile of the output; a wave owns 32 x 32 of it as 2 x 2 MFMA tiles of 16 x 16.  Per chunk of GK = 16 k the block stages 64 rows of
// X and 64 rows of Y in LDS as fp64 (row stride GK + 1 doubles: the staging writes are consecutive, the fragment reads of
// 16 rows x 4 k spread over the banks), zero-filled past nx, ny and D -- edges in all three extents cost nothing else.  Chunks go in
// ascending k, the four MFMA steps of a chunk too.
//
// Fragment maps of v_mfma_f64_16x16x4_f64 (D = A * B + C, 16 x 16 x 4): lane l feeds A[row l & 15][k l >> 4] and
// B[k l >> 4][col l & 15]; it receives, in register r of 4, D[row (l >> 4) + 4 r][col l & 15] -- NOT the (l >> 4) * 4 + r of the
// fp32-accumulating instructions.
constexpr int GT = 64;          // tile extent in rows and columns of the output
constexpr int GK = 16;          // k per LDS stage
constexpr int GS = GK + 1;      // LDS row stride in doubles

struct SqdistArgs {
  const float* X; const float* Y;
  const double* normX; const double* normY;
  double* out;
  int nx, ny, D;
  int64_t ldx, ldy, ldo;
  int64_t self_offset;      // >= 0: out[i][self_offset + i] = +inf; -1: nothing replaced
};

__device__ __forceinline__ void stage_tile(double (*dst)[GS], const float* __restrict__ src, int64_t ld, int row0, int rows, int k0,
                                           int K) {
  const int kk = threadIdx.x & (GK - 1), r0 = threadIdx.x >> 4;      // 16 k x 16 rows per pass
#pragma unroll
  for (int p = 0; p < GT / 16; ++p) {
    const int r = r0 + 16 * p;
    const int gr = row0 + r, gk = k0 + kk;
    dst[r][kk] = (gr < rows && gk < K) ? (double)src[(int64_t)gr * ld + gk] : 0.0;
  }
}

__global__ __launch_bounds__(256) void sqdist_nt_f64_kernel(SqdistArgs a) {
  __shared__ double Xs[GT][GS];
  __shared__ double Ys[GT][GS];
  const int ti = blockIdx.y, tj = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
  const int fr = lane & 15, fk = lane >> 4;
  f64x4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < a.D; k0 += GK) {
    stage_tile(Xs, a.X, a.ldx, ti * GT, a.nx, k0, a.D);
    stage_tile(Ys, a.Y, a.ldy, tj * GT, a.ny, k0, a.D);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < GK; ks += 4) {
      const double a0 = Xs[wi + fr][ks + fk], a1 = Xs[wi + 16 + fr][ks + fk];
      const double b0 = Ys[wj + fr][ks + fk], b1 = Ys[wj + 16 + fr][ks + fk];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      const int j = tj * GT + wj + 16 * y + fr;
      if (j >= a.ny) continue;
      const double nyj = a.normY[j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ti * GT + wi + 16 * x + fk + 4 * r;
        if (i >= a.nx) continue;
        // three roundings: the sum of the norms, the difference (2 * dot is exact), none for the clamp
        double v = fmax(0.0, (a.normX[i] + nyj) - 2.0 * acc[x][y][r]);
        if (a.self_offset >= 0 && (int64_t)j == a.self_offset + i) v = __builtin_huge_val();
        a.out[(int64_t)i * a.ldo + j] = v;
      }
    }
}

// ---------------------------------------------------------------- k-th smallest of every row
// A wave per row.  Lane l keeps the KS smallest of elements l, l + 64, ... ascending in registers (a new element below the largest
// kept is carried through the list by compare-and-swap; all indices are compile-time).  The k smallest of the row are among the
// 64 lists' heads and successors: k rounds of a wave-wide minimum over the heads, each popping the head of the lowest lane that
// holds the minimum, leave the k-th smallest -- counted with multiplicity, so ties do not matter.  Empty slots hold +inf, which
// therefore sorts last; a NaN never enters a list.
template <int KS>
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void row_kth_kernel(const double* __restrict__ d, int rows, int n, int64_t ld, int k,
                                                                      double* __restrict__ out) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= rows) return;      // (uniform over the wave; no barrier in this kernel)
  const double inf = __builtin_huge_val();
  const double* p = d + (int64_t)row * ld;
  double a[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) a[s] = inf;
  for (int j = lane; j < n; j += 64) {
    double v = p[j];
    if (v < a[KS - 1]) {
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const double lo = fmin(a[s], v), hi = fmax(a[s], v);
        a[s] = lo;
        v = hi;
      }
    }
  }
  double m = inf;
  for (int round = 0; round < k; ++round) {
    m = wave_min(a[0]);
    const unsigned long long holders = __ballot(a[0] == m);
    const int owner = holders ? __ffsll((long long)holders) - 1 : -1;
    if (lane == owner) {
#pragma unroll
      for (int s = 0; s + 1 < KS; ++s) a[s] = a[s + 1];
      a[KS - 1] = inf;
    }
  }
  if (lane == 0) out[row] = m;
}

// ---------------------------------------------------------------- ball counts and the row minimum
// cnt[i] = #{ j : d[i][j] < r_col[j] } and dmin[i] = min_j d[i][j]: a wave per row, lane l walks columns l, l + 64, ...; an integer
// sum and a minimum, exact in any order
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void row_ball_kernel(const double* __restrict__ d, const double* __restrict__ r_col,
                                                                       int rows, int n, int64_t ld, int32_t* __restrict__ cnt,
                                                                       double* __restrict__ dmin) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (row >= rows) return;      // (uniform over the wave; no barrier in this kernel)
  const double* p = d + (int64_t)row * ld;
  int c = 0;
  double m = __builtin_huge_val();
  for (int j = lane; j < n; j += 64) {
    const double v = p[j];
    c += v < r_col[j] ? 1 : 0;
    m = fmin(m, v);
  }
  c = wave_sum(c);
  m = wave_min(m);
  if (lane == 0) {
    if (cnt) cnt[row] = c;
    if (dmin) dmin[row] = m;
  }
}

inline dim3 row_grid(int rows) { return dim3((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK); }

}  // namespace
}  // namespace hrv

using namespace hrv;

extern "C" int hrv_row_sqnorm_f64(const float* x, int32_t n, int32_t D, int64_t ld, double* out, hrv_stream_t stream) {
  HRV_REQUIRE(x && out && n > 0 && D > 0, "row_sqnorm_f64: bad args");
  HRV_REQUIRE(ld >= D, "row_sqnorm_f64: leading dimension %lld below D=%d", (long long)ld, D);
  hipLaunchKernelGGL(row_sqnorm_kernel, row_grid(n), dim3(64 * ROWS_PER_BLOCK), 0, (hipStream_t)stream, x, n, D, ld, out);
  return check_launch("row_sqnorm_kernel");
}

extern "C" int hrv_sqdist_nt_f64(const float* X, const float* Y, int32_t nx, int32_t ny, int32_t D, int64_t ldx, int64_t ldy,
                                 const double* normX, const double* normY, int64_t self_offset, double* out, int64_t ldo,
                                 hrv_stream_t stream) {
  HRV_REQUIRE(X && Y && normX && normY && out && nx > 0 && ny > 0 && D > 0, "sqdist_nt_f64: bad args");
  HRV_REQUIRE(ldx >= D && ldy >= D && ldo >= ny, "sqdist_nt_f64: leading dimensions (%lld, %lld, %lld) below D=%d / ny=%d",
              (long long)ldx, (long long)ldy, (long long)ldo, D, ny);
  HRV_REQUIRE(self_offset >= -1 && (self_offset < 0 || self_offset + nx <= ny),
              "sqdist_nt_f64: self_offset %lld with nx=%d, ny=%d (-1, or a slab of nx rows inside ny)", (long long)self_offset, nx, ny);
  HRV_REQUIRE((nx + GT - 1) / GT <= 65535, "sqdist_nt_f64: nx=%d too large", nx);
  SqdistArgs a;
  a.X = X; a.Y = Y; a.normX = normX; a.normY = normY; a.out = out; a.nx = nx; a.ny = ny; a.D = D;
  a.ldx = ldx; a.ldy = ldy; a.ldo = ldo; a.self_offset = self_offset;
  hipLaunchKernelGGL(sqdist_nt_f64_kernel, dim3((ny + GT - 1) / GT, (nx + GT - 1) / GT), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("sqdist_nt_f64_kernel");
}

extern "C" int hrv_row_kth_max(void) { return KTH_MAX; }

extern "C" int hrv_row_kth_f64(const double* d, int32_t rows, int32_t n, int64_t ld, int32_t k, double* out, hrv_stream_t stream) {
  HRV_REQUIRE(d && out && rows > 0 && n > 0, "row_kth_f64: bad args");
  HRV_REQUIRE(ld >= n, "row_kth_f64: leading dimension %lld below n=%d", (long long)ld, n);
  HRV_REQUIRE(k >= 1 && k <= KTH_MAX && k <= n, "row_kth_f64: k=%d outside 1 .. min(%d, n=%d)", k, KTH_MAX, n);
  const dim3 grid = row_grid(rows), block(64 * ROWS_PER_BLOCK);
  if (k <= 8) hipLaunchKernelGGL(row_kth_kernel<8>, grid, block, 0, (hipStream_t)stream, d, rows, n, ld, k, out);
  else hipLaunchKernelGGL(row_kth_kernel<KTH_MAX>, grid, block, 0, (hipStream_t)stream, d, rows, n, ld, k, out);
  return check_launch("row_kth_kernel");
}

extern "C" int hrv_row_ball_f64(const double* d, const double* r_col, int32_t rows, int32_t n, int64_t ld, int32_t* cnt, double* dmin,
                                hrv_stream_t stream) {
  HRV_REQUIRE(d && r_col && rows > 0 && n > 0, "row_ball_f64: bad args");
  HRV_REQUIRE(cnt || dmin, "row_ball_f64: both outputs are null");
  HRV_REQUIRE(ld >= n, "row_ball_f64: leading dimension %lld below n=%d", (long long)ld, n);
  hipLaunchKernelGGL(row_ball_kernel, row_grid(rows), dim3(64 * ROWS_PER_BLOCK), 0, (hipStream_t)stream, d, r_col, rows, n, ld, cnt,
                     dmin);
  return check_launch("row_ball_kernel");
}
