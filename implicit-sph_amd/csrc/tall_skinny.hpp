// tall_skinny.hpp -- the two dense contractions of a tall block of vectors (n rows, at most 64 columns) with a small
// matrix, for the recycle step of GCRO-DR (gcrodr.hpp) and the Cholesky-QR of a carried recycle space:
//
//   k_tall_gemm    Out[:, c] (+)= sum_i coef[i][c] Basis_i     (C = W Q, U = Vh P R^-1, X <- X R^-1)
//   k_block_gram   G[a][c] = sum_rows X_a Y_c                  (W^T U, Cn^T Cn)
//
// Both read every element of the block once per sweep where the per-column launches they replace (combine /
// multi_dot_host of gcrodr.hpp) read the whole block once per output column.  Blocks are vector-major (vector v at
// base + v * ld) and may come in two pieces, [C | V] or [U | V].
#pragma once
#include "solver.hpp"

namespace isph {

constexpr int kTallMax = 64;   // vectors of a block, and outputs, at most
constexpr int kTallTile = 24;  // outputs whose running sums a thread keeps in registers; more outputs: more tiles

// One tile of outputs [c0, c0 + qt), qt <= QT: a thread owns a row, keeps the QT running sums in registers and walks the
// basis vectors in ascending order -- per output ONE fma chain from 0.0 (ACC: from the stored value), the chain that
// k_fill + k_multi_axpy make for that column, so the result has the bits of the per-column launches.
// coef: device, row i = the coefficients of basis vector i, ldc doubles apart, zero beyond q up to a multiple of
// kTallTile (the sums beyond qt are computed on those zeros and not stored).
template <int QT, bool ACC>
__global__ __launch_bounds__(kBlock) void k_tall_gemm(int n, int pa, const double *__restrict__ A, long long lda, int pb,
                                                      const double *__restrict__ B, long long ldb,
                                                      const double *__restrict__ coef, int ldc, int c0, int qt,
                                                      double *__restrict__ Out, long long ldo) {
  const double *__restrict__ cf0 = coef + c0;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    double acc[QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) acc[u] = (ACC && u < qt) ? Out[(long long)(c0 + u) * ldo + i] : 0.0;
    for (int v = 0; v < pa; ++v) {
      const double b = A[(long long)v * lda + i];
      const double *__restrict__ cf = cf0 + (long long)v * ldc;
#pragma unroll
      for (int u = 0; u < QT; ++u) acc[u] = fma(cf[u], b, acc[u]);
    }
    for (int v = 0; v < pb; ++v) {
      const double b = B[(long long)v * ldb + i];
      const double *__restrict__ cf = cf0 + (long long)(pa + v) * ldc;
#pragma unroll
      for (int u = 0; u < QT; ++u) acc[u] = fma(cf[u], b, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < QT; ++u)
      if (u < qt) Out[(long long)(c0 + u) * ldo + i] = acc[u];
  }
}

// X <- X T in place, T upper triangular (p x p): a thread owns a row and loads its p inputs before it stores, so no
// tile order can read a value that was already replaced.  coefT: device, row c = column c of T (coefT[c * ldc + i] =
// T[i][c]), rows and columns up to P present (zero beyond p).  Output c is the chain over i = 0..c from 0.0.
template <int P>
__global__ __launch_bounds__(kBlock) void k_tall_gemm_inplace(int n, int p, double *__restrict__ X, long long ld,
                                                              const double *__restrict__ coefT, int ldc) {
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    double x[P];
#pragma unroll
    for (int u = 0; u < P; ++u) x[u] = u < p ? X[(long long)u * ld + i] : 0.0;
#pragma unroll
    for (int c = 0; c < P; ++c) {
      if (c < p) {  // uniform
        const double *__restrict__ cf = coefT + (long long)c * ldc;
        double s = 0.0;
#pragma unroll
        for (int u = 0; u <= c; ++u) s = fma(cf[u], x[u], s);
        X[(long long)c * ld + i] = s;
      }
    }
  }
}

constexpr int kGramRows = 32;  // rows of a chunk staged in LDS
constexpr int kGramLd = 66;    // doubles between two staged rows: 64 vectors + 2 (16-byte reads stay aligned, the staging
                               // writes of 32 consecutive rows spread over the banks)

// partial[(a * q + c) * gridDim.x + blockIdx.x] = this workgroup's part of G[a][c] = sum_rows X_a Y_c, X = [XA | XB].
// One sweep over the rows: a chunk of kGramRows rows of all p + q vectors is staged in LDS (row-major there), and the 256
// threads, as 16 x 16, each add the chunk's contribution to a TA x TC tile of G they keep in registers (TA = 1, 2, 4 for
// p <= 16, 32, 64, TC likewise for q: a 51 x 10 product keeps 130 threads busy with 4 x 1 tiles where square tiles would
// keep 39).  The order of the sums depends on n and the grid only, never on timing.
template <int TA, int TC>
__global__ __launch_bounds__(kBlock) void k_block_gram(int n, int pa, const double *__restrict__ XA, long long lda, int pb,
                                                       const double *__restrict__ XB, long long ldb, int q,
                                                       const double *__restrict__ Y, long long ldy,
                                                       double *__restrict__ partial) {
  __shared__ double xs[kGramRows][kGramLd], ys[kGramRows][kGramLd];
  const int p = pa + pb;
  const int ta = threadIdx.x >> 4, tc = threadIdx.x & 15;
  const int lr = threadIdx.x & (kGramRows - 1), lv = threadIdx.x / kGramRows;  // staging: row of the chunk, first vector
  const bool mine = TA * ta < p && TC * tc < q;
  double acc[TA][TC];
#pragma unroll
  for (int e = 0; e < TA; ++e)
#pragma unroll
    for (int f = 0; f < TC; ++f) acc[e][f] = 0.0;
  for (long long r0 = (long long)blockIdx.x * kGramRows; r0 < n; r0 += (long long)gridDim.x * kGramRows) {
    const long long row = r0 + lr;
    const bool in = row < n;
    for (int v = lv; v < 16 * TA; v += kBlock / kGramRows) {  // the columns the tiles read: 16 TA of X, 16 TC of Y
      double xv = 0.0;
      if (in && v < p) xv = v < pa ? XA[(long long)v * lda + row] : XB[(long long)(v - pa) * ldb + row];
      xs[lr][v] = xv;
    }
    for (int v = lv; v < 16 * TC; v += kBlock / kGramRows) {
      double yv = 0.0;
      if (in && v < q) yv = Y[(long long)v * ldy + row];
      ys[lr][v] = yv;
    }
    __syncthreads();
    if (mine) {
#pragma unroll 4
      for (int r = 0; r < kGramRows; ++r) {
        double xa[TA], yc[TC];
#pragma unroll
        for (int e = 0; e < TA; ++e) xa[e] = xs[r][TA * ta + e];
#pragma unroll
        for (int f = 0; f < TC; ++f) yc[f] = ys[r][TC * tc + f];
#pragma unroll
        for (int e = 0; e < TA; ++e)
#pragma unroll
          for (int f = 0; f < TC; ++f) acc[e][f] = fma(xa[e], yc[f], acc[e][f]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < TA; ++e)
#pragma unroll
    for (int f = 0; f < TC; ++f) {
      const int a = TA * ta + e, c = TC * tc + f;
      if (a < p && c < q) partial[((long long)a * q + c) * gridDim.x + blockIdx.x] = acc[e][f];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
inline int tall_ldc(int q) { return (q + kTallTile - 1) / kTallTile * kTallTile; }

// Out[:, c] (+)= sum_i coef[i * q + c] Basis_i for c < q, Basis = [A (pa vectors) | B (pb vectors)], coefficients from
// the host (row-major p x q).  cbuf: device scratch of the caller.
inline int tall_gemm(isph_ctx *ctx, int n, int pa, const double *A, long long lda, int pb, const double *B, long long ldb,
                     int q, const double *coef, double *Out, long long ldo, bool accumulate, DevBuf<double> &cbuf) {
  const int p = pa + pb;
  ISPH_REQUIRE(pa >= 0 && pb >= 0 && p <= kTallMax && q >= 1 && q <= kTallMax, "tall_gemm: at most 64 vectors and 64 outputs");
  ISPH_REQUIRE(lda >= n && ldb >= n && ldo >= n, "tall_gemm: a leading dimension is shorter than the vectors");
  const int ldc = tall_ldc(q);
  std::vector<double> h((size_t)(p > 0 ? p : 1) * ldc, 0.0);
  for (int i = 0; i < p; ++i)
    for (int c = 0; c < q; ++c) h[(size_t)i * ldc + c] = coef[(size_t)i * q + c];
  ISPH_CHECK(cbuf.reserve((size_t)kTallMax * tall_ldc(kTallMax)));
  ISPH_CHECK_HIP(hipMemcpyAsync(cbuf.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, ctx->stream));
  const int sg = stream_grid(n);
  for (int c0 = 0; c0 < q; c0 += kTallTile) {
    const int qt = std::min(kTallTile, q - c0);
#define ISPH_TALL_LAUNCH(QT)                                                                                             \
  do {                                                                                                                   \
    if (accumulate)                                                                                                      \
      hipLaunchKernelGGL((k_tall_gemm<QT, true>), dim3(sg), dim3(kBlock), 0, ctx->stream, n, pa, A, lda, pb, B, ldb,     \
                         (const double *)cbuf.p, ldc, c0, qt, Out, ldo);                                                 \
    else                                                                                                                 \
      hipLaunchKernelGGL((k_tall_gemm<QT, false>), dim3(sg), dim3(kBlock), 0, ctx->stream, n, pa, A, lda, pb, B, ldb,    \
                         (const double *)cbuf.p, ldc, c0, qt, Out, ldo);                                                 \
  } while (0)
    if (qt <= 8) ISPH_TALL_LAUNCH(8);
    else if (qt <= 16) ISPH_TALL_LAUNCH(16);
    else ISPH_TALL_LAUNCH(24);
#undef ISPH_TALL_LAUNCH
  }
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));  // the pageable source must outlive the copy
  return ISPH_SUCCESS;
}

// X <- X T, T (p x p, row-major, host) upper triangular: what lies below the diagonal is not read
inline int tall_gemm_inplace(isph_ctx *ctx, int n, int p, double *X, long long ld, const double *T, DevBuf<double> &cbuf) {
  ISPH_REQUIRE(p >= 1 && p <= kTallMax, "tall_gemm_inplace: 1 to 64 vectors");
  ISPH_REQUIRE(ld >= n, "tall_gemm_inplace: the leading dimension is shorter than the vectors");
  const int ldc = kTallMax;
  std::vector<double> h((size_t)kTallMax * ldc, 0.0);
  for (int c = 0; c < p; ++c)
    for (int i = 0; i <= c; ++i) h[(size_t)c * ldc + i] = T[(size_t)i * p + c];
  ISPH_CHECK(cbuf.reserve((size_t)kTallMax * tall_ldc(kTallMax)));
  ISPH_CHECK_HIP(hipMemcpyAsync(cbuf.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, ctx->stream));
  const int sg = stream_grid(n);
#define ISPH_TALL_INPLACE(P) \
  hipLaunchKernelGGL((k_tall_gemm_inplace<P>), dim3(sg), dim3(kBlock), 0, ctx->stream, n, p, X, ld, (const double *)cbuf.p, ldc)
  if (p <= 8) ISPH_TALL_INPLACE(8);
  else if (p <= 16) ISPH_TALL_INPLACE(16);
  else if (p <= 24) ISPH_TALL_INPLACE(24);
  else if (p <= 32) ISPH_TALL_INPLACE(32);
  else if (p <= 48) ISPH_TALL_INPLACE(48);
  else ISPH_TALL_INPLACE(64);
#undef ISPH_TALL_INPLACE
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return ISPH_SUCCESS;
}

inline int gram_grid(int n) {
  long long g = ((long long)n + kGramRows - 1) / kGramRows;
  if (g > 1024) g = 1024;  // four workgroups per CU (their LDS allows it) hide the staging loads; p q partials each
  if (g < 1) g = 1;
  return (int)g;
}

// G (p x q, row-major, host) = [XA | XB]^T Y, summed over the ranks when `reduce`.  scratch: device scratch of the caller.
inline int block_gram(isph_ctx *ctx, int n, int pa, const double *XA, long long lda, int pb, const double *XB, long long ldb,
                      int q, const double *Y, long long ldy, double *G, DevBuf<double> &scratch, bool reduce) {
  const int p = pa + pb;
  ISPH_REQUIRE(pa >= 0 && pb >= 0 && p >= 1 && p <= kTallMax && q >= 1 && q <= kTallMax, "block_gram: 1 to 64 vectors on either side");
  ISPH_REQUIRE(lda >= n && ldb >= n && ldy >= n, "block_gram: a leading dimension is shorter than the vectors");
  const int g = gram_grid(n), pq = p * q;
  ISPH_CHECK(scratch.reserve((size_t)pq * (size_t)(g + 1)));
  double *out = scratch.p + (size_t)pq * (size_t)g;
#define ISPH_GRAM_LAUNCH(TA, TC) \
  hipLaunchKernelGGL((k_block_gram<TA, TC>), dim3(g), dim3(kBlock), 0, ctx->stream, n, pa, XA, lda, pb, XB, ldb, q, Y, ldy, scratch.p)
#define ISPH_GRAM_ROWS(TA)               \
  do {                                   \
    if (q <= 16) ISPH_GRAM_LAUNCH(TA, 1); \
    else if (q <= 32) ISPH_GRAM_LAUNCH(TA, 2); \
    else ISPH_GRAM_LAUNCH(TA, 4);        \
  } while (0)
  if (p <= 16) ISPH_GRAM_ROWS(1);
  else if (p <= 32) ISPH_GRAM_ROWS(2);
  else ISPH_GRAM_ROWS(4);
#undef ISPH_GRAM_ROWS
#undef ISPH_GRAM_LAUNCH
  hipLaunchKernelGGL(k_reduce_partials, dim3(pq), dim3(kBlock), 0, ctx->stream, pq, g, (const double *)scratch.p, out,
                     (const double *)nullptr);
  if (reduce) ISPH_CHECK(allreduce_inplace(ctx, out, pq));
  ISPH_CHECK_HIP(hipMemcpyAsync(G, out, sizeof(double) * (size_t)pq, hipMemcpyDeviceToHost, ctx->stream));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return ISPH_SUCCESS;
}

}  // namespace isph
