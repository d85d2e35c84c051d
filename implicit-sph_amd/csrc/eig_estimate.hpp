// eig_estimate.hpp -- an estimate of lambda_max(D^-1 A) by k Arnoldi steps: ML's "eigen-analysis: type" = "cg" for the
// damping of the SA-AMG prolongator and for the Chebyshev intervals (isph_cheb_params::eig_type = 1,
// isph_amg_params::eig_type = 1), in place of the row-sum bound rho = ||D^-1 A||_inf.
//
// ML's "cg" is symmetric Lanczos; the project's matrices are nonsymmetric after particle shifting and on wall rows, where
// Lanczos returns numbers far outside the spectrum, so the projection here is Arnoldi -- the same Krylov projection for
// a symmetric matrix, and correct in general (a declared departure):
//     B = D^-1 A of the level operator as it is applied (halo exchange on several ranks, the float plane of a
//         value_bits = 32 Chebyshev), v_0 = u / |u| with the deterministic start vector below,
//     step j: w = B v_j, classical Gram-Schmidt against v_0..v_j TWICE (cgs_pass: the two-stage deterministic multi-dot
//             and update of the Krylov solvers, all-reduced), h_{ij} = c1_i + c2_i, h_{j+1,j} = |w|, v_{j+1} = w / |w|;
//             stop at h_{j+1,j} <= 1e-14 |h_00| (an invariant subspace),
//     lambda_est = the largest real part of the eigenvalues of the leading m x m Hessenberg block (host, complex
//                  Hessenberg-QR of dense_small.hpp),
//     lambda_used = min(lambda_est, rho) -- rho is a rigorous bound; rho itself when lambda_est is not finite or <= 0.
// Start vector: u_g = (w + 0.5) / 2^31 - 1 with w the first word of Philox4x32-10, key (0x15B4, 0), counter
// (g, level, 0, 0).  On level 0 g is the row number in the CALLER's numbering plus the row counts of all lower ranks, so
// the estimate depends neither on the library's brick numbering nor on the rank count (up to summation rounding); on a
// coarse level g is the level's own row index plus the rank offset.
//
// The product is ONE sweep of the SELL-64 layout with the scaling in the epilogue (k_sell_dinv_spmv: the slice walk of
// k_sell_cheby_step).  ISPH_EIG_UNFUSED=1 (read at create time) runs spmv_dev plus a scaling kernel instead: the
// cross-check and the timing baseline.
#pragma once
#include <cmath>
#include <vector>

#include "dense_small.hpp"
#include "philox.hpp"
#include "solver.hpp"

namespace isph {

constexpr int kEigMaxIters = 50;

struct EigResult {
  double lambda_used = 0.0, rho = 0.0, lambda_est = 0.0;
  int steps = 0;
};

inline bool eig_unfused_env() {
  const char *env = getenv("ISPH_EIG_UNFUSED");
  return env && env[0] == '1';
}

// u_i of the start vector; perm (level 0 of a matrix in the library's numbering): internal row i is the caller's perm[i]
__global__ __launch_bounds__(kBlock) void k_eig_start(int n, long long offset, unsigned level, const int *__restrict__ perm,
                                                      double *__restrict__ u) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long g = offset + (perm ? perm[i] : (int)i);
    unsigned o[4];
    philox4x32_10((unsigned)g, level, 0u, 0u, 0x15B4u, 0u, o);
    u[i] = ((double)o[0] + 0.5) * 0x1.0p-31 - 1.0;
  }
}

// y = a x (y may be x)
__global__ __launch_bounds__(kBlock) void k_eig_scale(int n, double a, const double *x, double *y) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    y[i] = a * x[i];
}

// ISPH_EIG_UNFUSED=1: w <- dinv (.) w behind a separate w = A v
__global__ __launch_bounds__(kBlock) void k_eig_dinv_scale(int n, const double *__restrict__ dinv, double *__restrict__ w) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    w[i] = dinv[i] * w[i];
}

// ---- w = dinv (.) (A v) in one sweep of the matrix ----------------------------------------------------------------------
// (A v)_i by the slice walk of k_sell_cheby_step (C16: pair-interleaved SELL-64, lane == row, 16-bit windowed columns
// through the per-wave LDS table; otherwise 32-bit columns: the level operators of the AMG), non-temporal matrix loads, XCD
// remap, the same launch geometry; then  w_i = dinv_i (A v)_i  -- the bits of the product followed by k_eig_dinv_scale.
// w must NOT alias v: other waves still gather v.  VT = float: sval is the float plane of a value_bits = 32 Chebyshev,
// each value widened before its fma.
template <bool C16, bool LIST, bool GHOST, class VT>
__global__ __launch_bounds__(kBlock) void k_sell_dinv_spmv(int nrow, int nslices, int nblocks_padded,
                                                           const long long *__restrict__ slice_off,
                                                           const void *__restrict__ cols, const int *__restrict__ wtab,
                                                           const VT *__restrict__ sval, const double *__restrict__ v,
                                                           const double *__restrict__ vg, const double *__restrict__ dinv,
                                                           double *__restrict__ w, const int *__restrict__ slice_list) {
  constexpr int UNROLL = 8;
  typedef typename SellPair<VT>::type VT2;
  __shared__ int tab[C16 ? kBlock / kWave : 1][64];
  const int blk = xcd_remap(blockIdx.x, nblocks_padded);
  const int wave = threadIdx.x >> 6;
  int slice = blk * (kBlock / kWave) + wave;
  if (slice >= nslices) return;
  if (LIST) slice = slice_list[slice];
  const int lane = threadIdx.x & 63;
  if (C16) {
    tab[wave][lane] = wtab[(long long)slice * 64 + lane] << 10;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  const int *__restrict__ tw = tab[C16 ? wave : 0];
  const long long off = slice_off[slice];
  const int npair = (int)((slice_off[slice + 1] - off) >> 7);
  const VT2 *__restrict__ a = reinterpret_cast<const VT2 *>(sval + off) + lane;
  const unsigned *__restrict__ c16 = reinterpret_cast<const unsigned *>(static_cast<const unsigned short *>(cols) + off) + lane;
  const int2 *__restrict__ c32 = reinterpret_cast<const int2 *>(static_cast<const int *>(cols) + off) + lane;
  double acc0 = 0.0, acc1 = 0.0;
  int q = 0;
  for (; q + UNROLL <= npair; q += UNROLL) {
    VT2 vv[UNROLL];
    int ca[UNROLL], cb[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      vv[u].x = __builtin_nontemporal_load(&a[(q + u) * 64].x);
      vv[u].y = __builtin_nontemporal_load(&a[(q + u) * 64].y);
      if (C16) {
        ca[u] = (int)__builtin_nontemporal_load(&c16[(q + u) * 64]);
      } else {
        ca[u] = __builtin_nontemporal_load(&c32[(q + u) * 64].x);
        cb[u] = __builtin_nontemporal_load(&c32[(q + u) * 64].y);
      }
    }
    double xa[UNROLL], xb[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if (C16) {
        const unsigned lo = (unsigned)ca[u] & 0xffffu, hi = (unsigned)ca[u] >> 16;
        xa[u] = x_at<GHOST>(v, vg, nrow, tw[lo >> 10] | (int)(lo & 1023u));
        xb[u] = x_at<GHOST>(v, vg, nrow, tw[hi >> 10] | (int)(hi & 1023u));
      } else {
        xa[u] = x_at<GHOST>(v, vg, nrow, ca[u]);
        xb[u] = x_at<GHOST>(v, vg, nrow, cb[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      acc0 = fma((double)vv[u].x, xa[u], acc0);
      acc1 = fma((double)vv[u].y, xb[u], acc1);
    }
  }
  for (; q < npair; ++q) {
    const VT2 vv = a[q * 64];
    int ca, cb;
    if (C16) {
      const unsigned cc = c16[q * 64];
      const unsigned lo = cc & 0xffffu, hi = cc >> 16;
      ca = tw[lo >> 10] | (int)(lo & 1023u);
      cb = tw[hi >> 10] | (int)(hi & 1023u);
    } else {
      const int2 cc = c32[q * 64];
      ca = cc.x;
      cb = cc.y;
    }
    acc0 = fma((double)vv.x, x_at<GHOST>(v, vg, nrow, ca), acc0);
    acc1 = fma((double)vv.y, x_at<GHOST>(v, vg, nrow, cb), acc1);
  }
  const int row = slice * kSlice + lane;
  if (row < nrow) w[row] = dinv[row] * (acc0 + acc1);
}

template <bool LIST, bool GHOST, class VT>
inline void dinv_spmv_launch(isph_ctx *ctx, const Sell &S, bool c16, int nsl, const int *list, const VT *val, const double *dinv,
                             const double *v, const double *vg, double *w) {
  if (nsl <= 0) return;
  int nbp = 0;
  const int grid = spmv_grid(nsl, &nbp);
  if (c16)
    hipLaunchKernelGGL((k_sell_dinv_spmv<true, LIST, GHOST, VT>), dim3(grid), dim3(kBlock), 0, ctx->stream, S.nrow, nsl, nbp,
                       (const long long *)S.slice_off.p, (const void *)S.col16.p, (const int *)S.wtab.p, val, v, vg, dinv, w, list);
  else
    hipLaunchKernelGGL((k_sell_dinv_spmv<false, LIST, GHOST, VT>), dim3(grid), dim3(kBlock), 0, ctx->stream, S.nrow, nsl, nbp,
                       (const long long *)S.slice_off.p, (const void *)S.col.p, (const int *)nullptr, val, v, vg, dinv, w, list);
}

template <class VT>
inline int dinv_spmv_fused(isph_ctx *ctx, const isph_mat *A, const VT *val, bool halo, bool c16, const double *dinv,
                           const double *v, double *w) {
  const Sell &S = A->S;
  if (!halo) {
    dinv_spmv_launch<false, false, VT>(ctx, S, c16, S.nslices, nullptr, val, dinv, v, nullptr, w);
  } else {   // the exchange of v overlaps the interior slices exactly as in spmv_dev
    const isph_halo &H = A->halo;
    ISPH_CHECK(halo_begin(ctx, A, v));
    dinv_spmv_launch<true, false, VT>(ctx, S, c16, H.n_int, H.list_int.p, val, dinv, v, nullptr, w);
    ISPH_CHECK_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_halo, 0));
    dinv_spmv_launch<true, true, VT>(ctx, S, c16, H.n_bnd, H.list_bnd.p, val, dinv, v, ctx->xghost.p, w);
  }
  return ISPH_SUCCESS;
}

// w = dinv (.) (A v), w != v; val32 != NULL: the product reads this float plane of A's values
inline int dinv_spmv(isph_ctx *ctx, const isph_mat *A, const float *val32, const double *dinv, const double *v, double *w,
                     bool unfused) {
  const Sell &S = A->S;
  if (unfused) {
    ISPH_CHECK(spmv_dev(ctx, A, v, w, nullptr, nullptr, 1.0, val32));
    hipLaunchKernelGGL(k_eig_dinv_scale, dim3(stream_grid(S.nrow)), dim3(kBlock), 0, ctx->stream, S.nrow, dinv, w);
    ISPH_CHECK_HIP(hipGetLastError());
    return ISPH_SUCCESS;
  }
  const bool halo = !A->local && (S.ncol != S.nrow || A->halo.nsend > 0);
  const bool c16 = !A->local && !A->aux && sell_cols16(ctx, S);
  if (val32) ISPH_CHECK(dinv_spmv_fused<float>(ctx, A, val32, halo, c16, dinv, v, w));
  else ISPH_CHECK(dinv_spmv_fused<double>(ctx, A, (const double *)S.val.p, halo, c16, dinv, v, w));
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

// largest real part of the eigenvalues of the leading m x m block of H (row-major, leading dimension ldh); NaN when the
// QR iteration does not converge
inline double eig_ritz_max(int m, const std::vector<double> &H, int ldh) {
  std::vector<double> B((size_t)m * m);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) B[(size_t)i * m + j] = H[(size_t)i * ldh + j];
  std::vector<dense::cplx> lam, X;
  if (!dense::eig_general(m, B, lam, X)) return NAN;
  double best = lam[0].real();
  for (int i = 1; i < m; ++i) best = lam[(size_t)i].real() > best ? lam[(size_t)i].real() : best;
  return best;
}

inline double eig_clip(double lambda_est, double rho) {
  if (!std::isfinite(lambda_est) || !(lambda_est > 0.0)) return rho;
  return lambda_est < rho ? lambda_est : rho;
}

// The estimate for the operator A (val32 != NULL: its float plane) with the inverse diagonal dinv [A->S.nrow] and the
// bound rho.  iters: the caller has checked 1..kEigMaxIters.  level: the counter word of the start vector; level 0 of a
// matrix in the library's numbering starts from the caller's row numbers (A->order).
// collective: every rank of the context calls this together -- the rank offsets, the dots and the norms are all-reduced;
// a rank that cannot reserve its basis tells the others in the first of these, so that all of them fail together.
inline int eig_estimate(isph_ctx *ctx, const isph_mat *A, const float *val32, const double *dinv, double rho, int iters, int level,
                        bool unfused, bool collective, EigResult *out) {
  const Sell &S = A->S;
  const int n = S.nrow;
  out->rho = rho; out->lambda_used = rho; out->lambda_est = 0.0; out->steps = 0;
  const long long ld = ((long long)(n > 0 ? n : 1) + 63) / 64 * 64 + 64;
  DevTmp<double> V, w;   // the basis: (k + 1) ld doubles, back in the pool when this returns
  int rc = ensure_scalars(ctx);
  if (rc == ISPH_SUCCESS) rc = V.reserve((size_t)(iters + 1) * (size_t)ld);
  if (rc == ISPH_SUCCESS) rc = w.reserve((size_t)ld);
  long long offset = 0, nglob = n;
  if (!comm_rank_offsets(ctx, collective, "eigenvalue estimate", "eigenvalue estimate: the all-reduce of the row counts failed", n,
                         &offset, &nglob, rc))
    return rc;
  const int k = (long long)iters < nglob ? iters : (int)nglob;
  if (k <= 0) return ISPH_SUCCESS;   // no rows anywhere: rho stands
  const int *perm = (level == 0 && A->order && n > 0) ? (const int *)A->order->perm.p : nullptr;
  const int g = stream_grid(n);
  hipLaunchKernelGGL(k_eig_start, dim3(g), dim3(kBlock), 0, ctx->stream, n, offset, (unsigned)level, perm, w.p);
  double nrm = 0.0;
  ISPH_CHECK(norm_host(ctx, n, w.p, &nrm));
  if (!(nrm > 0.0) || !std::isfinite(nrm)) return ISPH_SUCCESS;
  hipLaunchKernelGGL(k_eig_scale, dim3(g), dim3(kBlock), 0, ctx->stream, n, 1.0 / nrm, (const double *)w.p, V.p);
  const int ldh = k;
  std::vector<double> H((size_t)k * k, 0.0), c1((size_t)k);
  int m = 0;
  for (int j = 0; j < k; ++j) {
    const int nk = j + 1;
    ISPH_CHECK(dinv_spmv(ctx, A, val32, dinv, V.p + (long long)j * ld, w.p, unfused));
    ISPH_CHECK(cgs_pass(ctx, n, nk, V.p, ld, w.p));
    for (int i = 0; i < nk; ++i) c1[(size_t)i] = ctx->hscal[SC_DOT + i];
    ISPH_CHECK(cgs_pass(ctx, n, nk, V.p, ld, w.p));
    for (int i = 0; i < nk; ++i) H[(size_t)i * ldh + j] = c1[(size_t)i] + ctx->hscal[SC_DOT + i];
    const double hn = std::sqrt(ctx->hscal[SC_DOT + nk + 1]);
    m = nk;
    if (!std::isfinite(hn)) break;
    if (hn <= 1e-14 * std::fabs(H[0])) break;   // an invariant subspace: the Ritz values of the block are eigenvalues
    if (nk < k) {
      H[(size_t)nk * ldh + j] = hn;
      hipLaunchKernelGGL(k_eig_scale, dim3(g), dim3(kBlock), 0, ctx->stream, n, 1.0 / hn, (const double *)w.p, V.p + (long long)nk * ld);
    }
  }
  ISPH_CHECK_HIP(hipGetLastError());
  out->steps = m;
  out->lambda_est = eig_ritz_max(m, H, ldh);
  out->lambda_used = eig_clip(out->lambda_est, rho);
  return ISPH_SUCCESS;
}

}  // namespace isph
