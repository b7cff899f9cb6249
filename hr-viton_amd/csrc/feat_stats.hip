// Statistics over banks of Inception features for evaluate.py's FID and KID on gfx950, in float64:
//   - one GEMM skeleton C[i][j] = epi(sum_k A[i][k] * B[j][k]) on v_mfma_f64_16x16x4_f64 (both operands row-major with k contiguous,
//     fp32 or fp64 in memory, products and sums in fp64), with a `linear` epilogue (the covariance) and a `poly3` one (KID's kernel);
//   - the column mean of an fp32 bank summed in fp64 in row order, and the centred transpose (X - mean)^T as fp64;
//   - KID's per-subset sums over gathered sub-matrices of the three Gram matrices.
// No atomics, no split-K: every output element is the work of one thread of one block walking k (or its gather) in a fixed order,
// so results do not depend on the grid and are bit-identical from run to run.
#include "hrv_common.h"

namespace hrv {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- fp64 GEMM, A [M][K] x B [N][K]^T
// A block of 256 threads (4 waves, 2 x 2) owns a 64 x 64 tile of C; a wave owns 32 x 32 of it as 2 x 2 MFMA tiles of 16 x 16.
// Per chunk of GK = 16 k the block stages 64 rows of A and 64 rows of B in LDS as fp64 (row stride GK + 1 doubles: the staging
// writes are consecutive, the fragment reads of 16 rows x 4 k spread over the banks), zero-filled past M, N and K -- edges in all
// three extents cost nothing else.  Chunks go in ascending k, the four MFMA steps of a chunk too.
//
// Fragment maps of v_mfma_f64_16x16x4_f64 (D = A * B + C, 16 x 16 x 4): lane l feeds A[row l & 15][k l >> 4] and
// B[k l >> 4][col l & 15]; it receives, in register r of 4, D[row (l >> 4) + 4 r][col l & 15] -- NOT the (l >> 4) * 4 + r of the
// fp32-accumulating instructions.
constexpr int GT = 64;          // tile extent in rows and columns of C
constexpr int GK = 16;          // k per LDS stage
constexpr int GS = GK + 1;      // LDS row stride in doubles

enum { EPI_LINEAR = 0, EPI_POLY3 = 1 };

struct GemmArgs {
  const void* A; const void* B; double* C;
  int M, N, K;
  int64_t lda, ldb, ldc;
  double param;        // linear: the factor; poly3: D of (s / D + 1)^3
  int symmetric;       // A == B, M == N: tiles on and above the diagonal only, each element written to (i, j) and (j, i)
};

template <int EPI>
__device__ __forceinline__ double epilogue(double s, double p) {
  if constexpr (EPI == EPI_LINEAR) {
    return s * p;
  } else {
    const double t = s / p + 1.0;
    return (t * t) * t;
  }
}

template <typename T>
__device__ __forceinline__ void stage_tile(double (*dst)[GS], const T* __restrict__ src, int64_t ld, int row0, int rows, int k0, int K) {
  const int kk = threadIdx.x & (GK - 1), r0 = threadIdx.x >> 4;      // 16 k x 16 rows per pass
#pragma unroll
  for (int p = 0; p < GT / 16; ++p) {
    const int r = r0 + 16 * p;
    const int gr = row0 + r, gk = k0 + kk;
    dst[r][kk] = (gr < rows && gk < K) ? (double)src[(int64_t)gr * ld + gk] : 0.0;
  }
}

template <typename T, int EPI>
__global__ __launch_bounds__(256) void gemm_nt_f64_kernel(GemmArgs a) {
  __shared__ double As[GT][GS];
  __shared__ double Bs[GT][GS];
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (a.symmetric && tj < ti) return;      // (uniform over the block: before any barrier)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
  const int fr = lane & 15, fk = lane >> 4;
  f64x4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = f64x4{0.0, 0.0, 0.0, 0.0};
  const T* A = (const T*)a.A;
  const T* B = (const T*)a.B;
  for (int k0 = 0; k0 < a.K; k0 += GK) {
    stage_tile<T>(As, A, a.lda, ti * GT, a.M, k0, a.K);
    stage_tile<T>(Bs, B, a.ldb, tj * GT, a.N, k0, a.K);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < GK; ks += 4) {
      const double a0 = As[wi + fr][ks + fk], a1 = As[wi + 16 + fr][ks + fk];
      const double b0 = Bs[wj + fr][ks + fk], b1 = Bs[wj + 16 + fr][ks + fk];
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
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ti * GT + wi + 16 * x + fk + 4 * r;
        const int j = tj * GT + wj + 16 * y + fr;
        if (i >= a.M || j >= a.N) continue;
        const double v = epilogue<EPI>(acc[x][y][r], a.param);
        if (!a.symmetric) {
          a.C[(int64_t)i * a.ldc + j] = v;
        } else if (j >= i) {      // the diagonal tile holds both (i, j) and (j, i): one of them is written to both places
          a.C[(int64_t)i * a.ldc + j] = v;
          a.C[(int64_t)j * a.ldc + i] = v;
        }
      }
}

template <typename T>
int launch_gemm(const GemmArgs& a, int epi, hipStream_t s) {
  const dim3 grid((a.N + GT - 1) / GT, (a.M + GT - 1) / GT);
  if (epi == EPI_LINEAR) hipLaunchKernelGGL((gemm_nt_f64_kernel<T, EPI_LINEAR>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((gemm_nt_f64_kernel<T, EPI_POLY3>), grid, dim3(256), 0, s, a);
  return check_launch("gemm_nt_f64_kernel");
}

// ---------------------------------------------------------------- moments of a feature bank
// mean[c] = (x[0][c] + x[1][c] + ... in row order, in fp64) / n: a thread per column, a wave reads 256-byte runs of a row
__global__ __launch_bounds__(64) void feat_mean_kernel(const float* __restrict__ x, int n, int D, double* __restrict__ mean) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= D) return;
  double s = 0.0;
  for (int r = 0; r < n; ++r) s += (double)x[(int64_t)r * D + c];
  mean[c] = s / (double)n;
}

// xt[c][r] = (double)x[r][c] - mean[c]: 32 x 32 tiles through LDS, both sides coalesced
__global__ __launch_bounds__(256) void feat_center_t_kernel(const float* __restrict__ x, const double* __restrict__ mean, int n, int D,
                                                           double* __restrict__ xt) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int r = r0 + ty + 8 * p, c = c0 + tx;
    if (r < n && c < D) tile[ty + 8 * p][tx] = (double)x[(int64_t)r * D + c] - mean[c];
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int c = c0 + ty + 8 * p, r = r0 + tx;
    if (r < n && c < D) xt[(int64_t)c * n + r] = tile[tx][ty + 8 * p];
  }
}

// ---------------------------------------------------------------- KID subset sums
// Block (s, w): w = 0 the off-diagonal sum of Kxx[ix_s, ix_s], w = 1 that of Kyy[iy_s, iy_s], w = 2 the full sum of Kxy[ix_s, iy_s].
// Thread t adds the gathered elements e = t, t + 256, ... (e = a * m + b) in that order, then the 256 partials meet in a fixed
// tree.  An index outside its matrix is not dereferenced: it makes the sum NaN.
__global__ __launch_bounds__(256) void kid_subset_sums_kernel(const double* __restrict__ Kxx, int nx, const double* __restrict__ Kyy,
                                                             int ny, const double* __restrict__ Kxy, const int32_t* __restrict__ ix,
                                                             const int32_t* __restrict__ iy, int m, double* __restrict__ out) {
  __shared__ double red[256];
  const int s = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
  const double* K = w == 0 ? Kxx : (w == 1 ? Kyy : Kxy);
  const int32_t* ri = (w == 1 ? iy : ix) + (int64_t)s * m;
  const int32_t* ci = (w == 0 ? ix : iy) + (int64_t)s * m;
  const int nr = w == 1 ? ny : nx, nc = w == 0 ? nx : ny;
  const int64_t total = (int64_t)m * m;
  double acc = 0.0;
  for (int64_t e = tid; e < total; e += 256) {
    const int a = (int)(e / m), b = (int)(e - (int64_t)a * m);
    if (w < 2 && a == b) continue;
    const int r = ri[a], c = ci[b];
    if (r < 0 || r >= nr || c < 0 || c >= nc) { acc = __builtin_nan(""); continue; }
    acc += K[(int64_t)r * nc + c];
  }
  red[tid] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) out[(int64_t)s * 3 + w] = red[0];
}

}  // namespace
}  // namespace hrv

using namespace hrv;

extern "C" int hrv_gemm_nt_f64(const void* A, const void* B, int32_t operands_f64, int32_t M, int32_t N, int32_t K, int64_t lda,
                               int64_t ldb, int32_t epilogue, double param, int32_t symmetric, double* C, int64_t ldc,
                               hrv_stream_t stream) {
  HRV_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0, "gemm_nt_f64: bad args");
  HRV_REQUIRE(lda >= K && ldb >= K && ldc >= N, "gemm_nt_f64: leading dimensions (%lld, %lld, %lld) below K=%d / N=%d", (long long)lda,
              (long long)ldb, (long long)ldc, K, N);
  HRV_REQUIRE(epilogue == EPI_LINEAR || epilogue == EPI_POLY3, "gemm_nt_f64: epilogue %d (0: linear, 1: poly3)", epilogue);
  HRV_REQUIRE(epilogue != EPI_POLY3 || param != 0.0, "gemm_nt_f64: poly3 divides by its parameter, which is 0");
  HRV_REQUIRE(!symmetric || (A == B && M == N && lda == ldb), "gemm_nt_f64: symmetric needs A == B and M == N");
  HRV_REQUIRE((M + GT - 1) / GT <= 65535, "gemm_nt_f64: M=%d too large", M);
  GemmArgs a;
  a.A = A; a.B = B; a.C = C; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.param = param;
  a.symmetric = symmetric ? 1 : 0;
  return operands_f64 ? launch_gemm<double>(a, epilogue, (hipStream_t)stream) : launch_gemm<float>(a, epilogue, (hipStream_t)stream);
}

extern "C" int hrv_feat_mean_f64(const float* x, int32_t n, int32_t D, double* mean, hrv_stream_t stream) {
  HRV_REQUIRE(x && mean && n > 0 && D > 0, "feat_mean: bad args");
  hipLaunchKernelGGL(feat_mean_kernel, dim3((D + 63) / 64), dim3(64), 0, (hipStream_t)stream, x, n, D, mean);
  return check_launch("feat_mean_kernel");
}

extern "C" int hrv_feat_center_t_f64(const float* x, const double* mean, int32_t n, int32_t D, double* xt, hrv_stream_t stream) {
  HRV_REQUIRE(x && mean && xt && n > 0 && D > 0, "feat_center_t: bad args");
  HRV_REQUIRE((n + 31) / 32 <= 65535, "feat_center_t: n=%d too large", n);
  hipLaunchKernelGGL(feat_center_t_kernel, dim3((D + 31) / 32, (n + 31) / 32), dim3(256), 0, (hipStream_t)stream, x, mean, n, D, xt);
  return check_launch("feat_center_t_kernel");
}

extern "C" int hrv_kid_subset_sums_f64(const double* Kxx, int32_t nx, const double* Kyy, int32_t ny, const double* Kxy,
                                       const int32_t* ix, const int32_t* iy, int32_t S, int32_t m, double* out, hrv_stream_t stream) {
  HRV_REQUIRE(Kxx && Kyy && Kxy && ix && iy && out && nx > 0 && ny > 0 && S > 0 && m > 0, "kid_subset_sums: bad args");
  HRV_REQUIRE(m <= nx && m <= ny, "kid_subset_sums: subset size %d exceeds a set (%d, %d)", m, nx, ny);
  hipLaunchKernelGGL(kid_subset_sums_kernel, dim3(S, 3), dim3(256), 0, (hipStream_t)stream, Kxx, nx, Kyy, ny, Kxy, ix, iy, m, out);
  return check_launch("kid_subset_sums_kernel");
}
