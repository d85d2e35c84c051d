// gmres_poly.hpp -- the GMRES polynomial in D^-1 A as a fixed linear preconditioner ("gmres-poly<d>",
// isph_prec_create_gmres_poly): what Belos' GmresPolySolMgr builds, restated from the algorithm (Trilinos is not vendored:
// unpinned against it).  No interval, no ratio, and a complex spectrum is handled.
//
//     B = D^-1 A,  v_0 = u / |u| with u the start vector of eig_estimate.hpp (k_eig_start, level 0: keyed by the caller's
//     global row, so the polynomial depends neither on the brick numbering nor on the rank count).  With a null vector n
//     (normalised here) u and every set-up product are projected: w <- w - (w.n) n.
//     d Arnoldi steps with cgs_pass (classical Gram-Schmidt twice, deterministic multi-dot) give H, (d + 1) x d.
//     Host: H^ = H_d + h_{d+1,d}^2 f e_d^T with H_d^T f = e_d; the roots theta_1..theta_d of the polynomial are the
//     eigenvalues of H^ (the harmonic Ritz values; dense_small.hpp), put in modified Leja order: largest modulus first, then
//     always the root with the largest product of distances to the ones chosen, a conjugate directly behind its partner.
//     A root with |Im theta| <= 1e-8 |theta| counts as real.
//     z = M^-1 r = p(B) D^-1 r in product form:  r <- D^-1 r, z = 0, then root by root
//         real theta:        z += r / theta,                          r <- r - (B r) / theta
//         pair a +- ib:      t = 2a r - B r,  z += t / (a^2 + b^2),   r <- r - (B t) / (a^2 + b^2)
//     without the product behind the last root: d - 1 sweeps of the matrix per application.  The application takes no
//     projection: B 1 = 0 keeps a null component bounded and the solver removes it.
//     A breakdown h_{j+1,j} <= 1e-14 |h_00| at step j < d gives degree j (H^ = H_j).  A root with |theta| <= 1e-10 max|theta|
//     fails the create by name: a singular matrix needs the null vector.
//
// One sweep is k_sell_poly_step: the slice walk of k_sell_cheby_step with y_i = dinv_i (A x)_i in the epilogue, then
//     out_i = c_own s_i + c_prod y_i   (s = x, or what out holds: the second half of a pair, whose r waits in the buffer
//                                       the first half read it from),      z_i += c_z out_i.
// The buffers ping-pong: other waves still gather x.  Every z term is written as a multiple of a step's OUT vector -- the
// r / theta of a real root joins the sweep (or the first, pointwise step r <- dinv r) that produces that r -- so an
// application is one streaming kernel and d - 1 sweeps, nothing else.  ISPH_POLY_UNFUSED=1 (read at create time) runs
// dinv_spmv plus k_poly_update with the same expressions (poly_out, poly_z): the cross-check, bit for bit, and the
// timing baseline.  With a halo plan the fused sweep runs over the interior slices while the exchange of x is under way and
// over the boundary slices behind it (LIST, GHOST), as every sweep of the library does.
#pragma once
#include <cmath>
#include <complex>
#include <vector>

#include "chebyshev.hpp"
#include "eig_estimate.hpp"

namespace isph {

constexpr int kPolyMaxDegree = 25;   // Belos' maximum
constexpr int kPolyHessLd = kPolyMaxDegree + 1;

struct PolyStep {
  double c_own, c_prod, c_z;
  int own_from_out;   // s = what out holds (the pair's second half) in place of x
};

struct Poly {
  int n = 0, degree_in = 0, degree = 0, unfused = 0;
  bool held = false, has_null = false;
  double re[kPolyMaxDegree], im[kPolyMaxDegree];   // the roots in application order
  double hess[kPolyHessLd * kPolyMaxDegree];        // H, column-major with leading dimension 26; (degree + 1) x degree is set
  double first_cz = 0.0;                            // z = first_cz dinv r of the pointwise step
  int nsteps = 0;
  PolyStep steps[kPolyMaxDegree];
  DevBuf<double> dinv, ra, rb, y, nullv;            // y: the product of the unfused form; nullv: n / |n|, the matrix' numbering
};

inline void poly_destroy(Poly *P) {
  if (!P) return;
  P->dinv.release(); P->ra.release(); P->rb.release(); P->y.release(); P->nullv.release();
  delete P;
}

// the two expressions of a step, shared by the fused and the unfused kernels (same bits from the same operands)
__device__ __forceinline__ double poly_out(double c_own, double c_prod, double s, double y) { return fma(c_prod, y, c_own * s); }
__device__ __forceinline__ double poly_z(double c_z, double out, double z) { return fma(c_z, out, z); }

// ---- the pointwise first step: r = dinv (.) rin, z = c_z r ---------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_poly_first(int n, double c_z, const double *__restrict__ dinv, const double *rin,
                                                       double *__restrict__ r, double *z) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const double v = dinv[i] * rin[i];
    r[i] = v;
    z[i] = c_z * v;
  }
}

// ISPH_POLY_UNFUSED=1: the update behind a separate y = dinv (.) (A x)
__global__ __launch_bounds__(kBlock) void k_poly_update(int n, double c_own, double c_prod, double c_z, int own_from_out,
                                                        const double *__restrict__ x, const double *__restrict__ y,
                                                        double *__restrict__ out, double *__restrict__ z) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const double o = poly_out(c_own, c_prod, own_from_out ? out[i] : x[i], y[i]);
    out[i] = o;
    if (c_z != 0.0) z[i] = poly_z(c_z, o, z[i]);
  }
}

// ---- one step in one sweep of the matrix ------------------------------------------------------------------------------
// (A x)_i by the slice walk of k_sell_cheby_step (C16: pair-interleaved SELL-64, lane == row, 16-bit windowed columns through
// the per-wave LDS table; otherwise 32-bit columns), non-temporal matrix loads, XCD remap, the same launch geometry; then
// y = dinv_i (acc0 + acc1) rounded as k_sell_dinv_spmv stores it, out_i = poly_out(..), z_i = poly_z(..).
// out must NOT alias x: other waves still gather x.  A lane reads out[row] (own_from_out) before it writes it, and nobody
// else touches that element.  c_z == 0: z is neither read nor written.
template <bool C16, bool LIST, bool GHOST>
__global__ __launch_bounds__(kBlock) void k_sell_poly_step(int nrow, int nslices, int nblocks_padded,
                                                           const long long *__restrict__ slice_off,
                                                           const void *__restrict__ cols, const int *__restrict__ wtab,
                                                           const double *__restrict__ sval, const double *__restrict__ x,
                                                           const double *__restrict__ xg, const double *__restrict__ dinv,
                                                           double *__restrict__ out, double *__restrict__ z, double c_own,
                                                           double c_prod, double c_z, int own_from_out,
                                                           const int *__restrict__ slice_list) {
  constexpr int UNROLL = 8;
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
  const double2 *__restrict__ v = reinterpret_cast<const double2 *>(sval + off) + lane;
  const unsigned *__restrict__ c16 = reinterpret_cast<const unsigned *>(static_cast<const unsigned short *>(cols) + off) + lane;
  const int2 *__restrict__ c32 = reinterpret_cast<const int2 *>(static_cast<const int *>(cols) + off) + lane;
  double acc0 = 0.0, acc1 = 0.0;
  int q = 0;
  for (; q + UNROLL <= npair; q += UNROLL) {
    double2 vv[UNROLL];
    int ca[UNROLL], cb[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      vv[u].x = __builtin_nontemporal_load(&v[(q + u) * 64].x);
      vv[u].y = __builtin_nontemporal_load(&v[(q + u) * 64].y);
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
        xa[u] = x_at<GHOST>(x, xg, nrow, tw[lo >> 10] | (int)(lo & 1023u));
        xb[u] = x_at<GHOST>(x, xg, nrow, tw[hi >> 10] | (int)(hi & 1023u));
      } else {
        xa[u] = x_at<GHOST>(x, xg, nrow, ca[u]);
        xb[u] = x_at<GHOST>(x, xg, nrow, cb[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      acc0 = fma(vv[u].x, xa[u], acc0);
      acc1 = fma(vv[u].y, xb[u], acc1);
    }
  }
  for (; q < npair; ++q) {
    const double2 vv = v[q * 64];
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
    acc0 = fma(vv.x, x_at<GHOST>(x, xg, nrow, ca), acc0);
    acc1 = fma(vv.y, x_at<GHOST>(x, xg, nrow, cb), acc1);
  }
  const int row = slice * kSlice + lane;
  if (row < nrow) {
    const double y = dinv[row] * (acc0 + acc1);
    const double o = poly_out(c_own, c_prod, own_from_out ? out[row] : x[row], y);
    out[row] = o;
    if (c_z != 0.0) z[row] = poly_z(c_z, o, z[row]);
  }
}

// ---- host: roots, order, steps ---------------------------------------------------------------------------------------------
// a root of the polynomial as the application sees it: a real one (b == 0) or the pair a +- ib (b > 0)
struct PolyRoot {
  double a, b;
};

// the eigenvalues lam of a real matrix as real roots and conjugate pairs: |Im| <= 1e-8 |lam| is a real root; every other
// one with Im > 0 takes the nearest unused one with Im < 0 as its partner (a, b averaged over the two); a root that finds
// no partner is kept as a real one
inline std::vector<PolyRoot> poly_pair_roots(const std::vector<dense::cplx> &lam) {
  const size_t m = lam.size();
  std::vector<PolyRoot> out;
  std::vector<char> used(m, 0);
  for (size_t i = 0; i < m; ++i)
    if (std::fabs(lam[i].imag()) <= 1e-8 * std::abs(lam[i])) { out.push_back({lam[i].real(), 0.0}); used[i] = 1; }
  for (size_t i = 0; i < m; ++i) {
    if (used[i] || lam[i].imag() < 0.0) continue;
    used[i] = 1;
    size_t best = m;
    double dist = INFINITY;
    for (size_t j = 0; j < m; ++j) {
      if (used[j] || lam[j].imag() >= 0.0) continue;
      const double dd = std::abs(lam[j] - std::conj(lam[i]));
      if (dd < dist) { dist = dd; best = j; }
    }
    if (best == m) { out.push_back({lam[i].real(), 0.0}); continue; }
    used[best] = 1;
    out.push_back({0.5 * (lam[i].real() + lam[best].real()), 0.5 * (lam[i].imag() - lam[best].imag())});
  }
  for (size_t i = 0; i < m; ++i)
    if (!used[i]) out.push_back({lam[i].real(), 0.0});
  return out;
}

// modified Leja order: the root of largest modulus first, then always the one with the largest sum of log distances to the
// roots chosen so far (both members of a chosen pair count); a pair stays together.  Ties: the earlier root.
inline std::vector<PolyRoot> poly_leja_order(const std::vector<PolyRoot> &in) {
  const size_t m = in.size();
  std::vector<PolyRoot> out;
  std::vector<char> used(m, 0);
  std::vector<double> score(m, 0.0);
  for (size_t k = 0; k < m; ++k) {
    size_t best = m;
    double sb = -INFINITY;
    for (size_t i = 0; i < m; ++i) {
      if (used[i]) continue;
      const double s = k == 0 ? std::hypot(in[i].a, in[i].b) : score[i];
      if (best == m || s > sb) { sb = s; best = i; }
    }
    used[best] = 1;
    out.push_back(in[best]);
    const std::complex<double> c(in[best].a, in[best].b);
    for (size_t i = 0; i < m; ++i) {
      if (used[i]) continue;
      const std::complex<double> t(in[i].a, in[i].b);
      score[i] += std::log(std::abs(t - c));
      if (in[best].b > 0.0) score[i] += std::log(std::abs(t - std::conj(c)));
    }
  }
  return out;
}

// H (column-major, leading dimension 26, m + 1 rows and m columns set; `breakdown`: h_{m+1,m} counts as 0) -> the roots in
// application order and the steps of the application.  Fails by name on a QR that does not converge and on a near-zero root.
inline int poly_from_hessenberg(Poly *P, int m, bool breakdown) {
  const double *H = P->hess;
  std::vector<double> Hh((size_t)m * m);   // row-major H^
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) Hh[(size_t)i * m + j] = H[i + kPolyHessLd * j];
  const double h = breakdown ? 0.0 : H[m + kPolyHessLd * (m - 1)];
  if (h != 0.0) {
    std::vector<double> Ht((size_t)m * m), f((size_t)m, 0.0);
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) Ht[(size_t)i * m + j] = Hh[(size_t)j * m + i];
    f[(size_t)m - 1] = 1.0;
    if (!dense::lu_solve(m, Ht, 1, f))
      return fail("GMRES polynomial: the Hessenberg matrix is singular (near-zero root: a singular matrix needs the null vector)", __FILE__, __LINE__);
    for (int i = 0; i < m; ++i) Hh[(size_t)i * m + (m - 1)] += h * h * f[(size_t)i];
  }
  std::vector<dense::cplx> lam, X;
  if (!dense::eig_general(m, Hh, lam, X)) return fail("GMRES polynomial: the QR iteration for the roots did not converge", __FILE__, __LINE__);
  for (const auto &l : lam)
    if (!std::isfinite(l.real()) || !std::isfinite(l.imag())) return fail("GMRES polynomial: a root is not finite", __FILE__, __LINE__);
  const std::vector<PolyRoot> roots = poly_leja_order(poly_pair_roots(lam));
  double big = 0.0;
  for (const auto &r : roots) big = std::max(big, std::hypot(r.a, r.b));
  for (const auto &r : roots)
    if (!(std::hypot(r.a, r.b) > 1e-10 * big))
      return fail("GMRES polynomial: near-zero root: a singular matrix needs the null vector", __FILE__, __LINE__);
  int k = 0;
  for (const auto &r : roots) {
    P->re[k] = r.a; P->im[k] = r.b; ++k;
    if (r.b > 0.0) { P->re[k] = r.a; P->im[k] = -r.b; ++k; }
  }
  P->degree = k;
  // the steps.  z collects  r / theta  of a real root and  t / (a^2 + b^2)  of a pair, each as a multiple of the OUT vector
  // of the step that produces it; the product behind the last root is not made
  auto cz_of = [&roots](size_t u) { return (u < roots.size() && roots[u].b == 0.0) ? 1.0 / roots[u].a : 0.0; };
  P->first_cz = cz_of(0);
  P->nsteps = 0;
  for (size_t u = 0; u < roots.size(); ++u) {
    const bool last = u + 1 == roots.size();
    const double a = roots[u].a, b = roots[u].b;
    if (b == 0.0) {
      if (!last) P->steps[P->nsteps++] = {1.0, -1.0 / a, cz_of(u + 1), 0};
    } else {
      const double mod = a * a + b * b;
      P->steps[P->nsteps++] = {2.0 * a, -1.0, 1.0 / mod, 0};
      if (!last) P->steps[P->nsteps++] = {1.0, -1.0 / mod, cz_of(u + 1), 1};
    }
  }
  return ISPH_SUCCESS;
}

// ---- set-up ----------------------------------------------------------------------------------------------------------------
// Everything numeric of a create call, from P->degree_in and P->nullv (has_null: n / |n| in the matrix' numbering):
// isph_prec_refactor runs it again on the new values and gets the bits of a fresh create.
// collective: every rank of the context calls this together -- rank offsets, dots and norms are all-reduced, so H and
// with it every decision taken from H is the same on all ranks; a rank that fails on its own tells the others.
inline int poly_build(isph_ctx *ctx, const isph_mat *A, Poly *P, bool collective) {
  const Sell &S = A->S;
  const int n = S.nrow, d = P->degree_in;
  P->n = n;
  const size_t mv = (size_t)(n > 0 ? n : 1) + 64;
  DevTmp<unsigned long long> flag;
  int rc = ensure_scalars(ctx);
  if (rc == ISPH_SUCCESS) rc = flag.reserve(3);
  if (rc == ISPH_SUCCESS) rc = P->dinv.reserve(mv);
  if (rc == ISPH_SUCCESS) rc = P->ra.reserve(mv);
  if (rc == ISPH_SUCCESS) rc = P->rb.reserve(mv);
  if (rc == ISPH_SUCCESS && P->unfused) rc = P->y.reserve(mv);
  if (rc == ISPH_SUCCESS) {
    unsigned long long hb[3] = {0ull, 0ull, 0ull};
    if (hipMemsetAsync(flag.p, 0, 3 * sizeof(unsigned long long), ctx->stream) != hipSuccess) rc = fail("memset failed", __FILE__, __LINE__);
    if (rc == ISPH_SUCCESS && S.nslices > 0)
      hipLaunchKernelGGL((k_cheby_setup<double>), dim3((S.nslices + 3) / 4), dim3(kBlock), 0, ctx->stream, S.nrow, S.nslices,
                         (const long long *)S.slice_off.p, (const int *)S.col.p, (const double *)S.val.p, 0, P->dinv.p, flag.p);
    if (rc == ISPH_SUCCESS && (hipMemcpyAsync(hb, flag.p, sizeof(hb), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                               hipStreamSynchronize(ctx->stream) != hipSuccess || hipGetLastError() != hipSuccess))
      rc = fail("GMRES polynomial set-up failed", __FILE__, __LINE__);
    if (rc == ISPH_SUCCESS && hb[1] != 0ull)
      rc = fail("GMRES polynomial: the matrix has a zero diagonal entry (the polynomial acts on D^-1 A)", __FILE__, __LINE__);
  }
  const long long ld = ((long long)(n > 0 ? n : 1) + 63) / 64 * 64 + 64;
  DevTmp<double> V, w;   // the basis: (d + 1) ld doubles, back in the pool when this returns
  if (rc == ISPH_SUCCESS) rc = V.reserve((size_t)(d + 1) * (size_t)ld);
  if (rc == ISPH_SUCCESS) rc = w.reserve((size_t)ld);
  long long offset = 0, nglob = n;
  if (!comm_rank_offsets(ctx, collective, "GMRES polynomial", "GMRES polynomial: the all-reduce of the row counts failed", n, &offset,
                         &nglob, rc))
    return rc;
  const int k = (long long)d < nglob ? d : (int)nglob;
  ISPH_REQUIRE(k >= 1, "GMRES polynomial: the matrix has no rows");
  const double *nv = P->has_null ? (const double *)P->nullv.p : nullptr;
  const int *perm = (A->order && n > 0) ? (const int *)A->order->perm.p : nullptr;
  const int g = stream_grid(n);
  hipLaunchKernelGGL(k_eig_start, dim3(g), dim3(kBlock), 0, ctx->stream, n, offset, 0u, perm, w.p);
  if (nv) ISPH_CHECK(project_dev(ctx, n, nv, w.p));
  double nrm = 0.0;
  ISPH_CHECK(norm_host(ctx, n, w.p, &nrm));
  ISPH_REQUIRE(nrm > 0.0 && std::isfinite(nrm), "GMRES polynomial: the start vector vanishes");
  hipLaunchKernelGGL(k_eig_scale, dim3(g), dim3(kBlock), 0, ctx->stream, n, 1.0 / nrm, (const double *)w.p, V.p);
  for (double &h : P->hess) h = 0.0;
  std::vector<double> c1((size_t)k);
  int m = 0;
  bool breakdown = false;
  for (int j = 0; j < k; ++j) {
    const int nk = j + 1;
    ISPH_CHECK(dinv_spmv(ctx, A, nullptr, P->dinv.p, V.p + (long long)j * ld, w.p, /*unfused=*/false));
    if (nv) ISPH_CHECK(project_dev(ctx, n, nv, w.p));
    ISPH_CHECK(cgs_pass(ctx, n, nk, V.p, ld, w.p));
    for (int i = 0; i < nk; ++i) c1[(size_t)i] = ctx->hscal[SC_DOT + i];
    ISPH_CHECK(cgs_pass(ctx, n, nk, V.p, ld, w.p));
    for (int i = 0; i < nk; ++i) P->hess[i + kPolyHessLd * j] = c1[(size_t)i] + ctx->hscal[SC_DOT + i];
    const double hn = std::sqrt(ctx->hscal[SC_DOT + nk + 1]);
    ISPH_REQUIRE(std::isfinite(hn), "GMRES polynomial: the Arnoldi process met a value that is not finite");
    P->hess[nk + kPolyHessLd * j] = hn;
    m = nk;
    if (hn <= 1e-14 * std::fabs(P->hess[0])) { breakdown = true; break; }   // an invariant subspace: degree j
    if (nk < k)
      hipLaunchKernelGGL(k_eig_scale, dim3(g), dim3(kBlock), 0, ctx->stream, n, 1.0 / hn, (const double *)w.p, V.p + (long long)nk * ld);
  }
  ISPH_CHECK_HIP(hipGetLastError());
  return poly_from_hessenberg(P, m, breakdown);
}

// nullvec: NULL, or n device doubles in the matrix' numbering (any length > 0; normalised here)
inline int poly_create(isph_ctx *ctx, const isph_mat *A, int degree, const double *nullvec, bool collective, Poly **out) {
  Poly *P = new Poly();
  const int n = A->S.nrow;
  const char *env = getenv("ISPH_POLY_UNFUSED");
  P->unfused = env && env[0] == '1';
  P->degree_in = degree;
  int rc = ISPH_SUCCESS;
  if (nullvec) {
    double nrm = 0.0;
    rc = ensure_scalars(ctx);
    if (rc == ISPH_SUCCESS) rc = P->nullv.reserve((size_t)(n > 0 ? n : 1) + 64);
    if (rc == ISPH_SUCCESS) rc = norm_host(ctx, n, nullvec, &nrm);
    if (rc == ISPH_SUCCESS && !(nrm > 0.0 && std::isfinite(nrm))) rc = fail("GMRES polynomial: the null vector vanishes or is not finite", __FILE__, __LINE__);
    if (rc == ISPH_SUCCESS) {
      hipLaunchKernelGGL(k_eig_scale, dim3(stream_grid(n)), dim3(kBlock), 0, ctx->stream, n, 1.0 / nrm, nullvec, P->nullv.p);
      P->has_null = true;
    }
  }
  if (rc == ISPH_SUCCESS) rc = poly_build(ctx, A, P, collective);
  if (rc != ISPH_SUCCESS) { poly_destroy(P); return rc; }
  *out = P;
  return ISPH_SUCCESS;
}

// ---- application -----------------------------------------------------------------------------------------------------------
template <bool LIST, bool GHOST>
inline void poly_step_launch(isph_ctx *ctx, const Sell &S, bool c16, int nsl, const int *list, const Poly *P, const PolyStep &s,
                             const double *x, const double *xg, double *out, double *z) {
  if (nsl <= 0) return;
  int nbp = 0;
  const int grid = spmv_grid(nsl, &nbp);
  if (c16)
    hipLaunchKernelGGL((k_sell_poly_step<true, LIST, GHOST>), dim3(grid), dim3(kBlock), 0, ctx->stream, S.nrow, nsl, nbp,
                       (const long long *)S.slice_off.p, (const void *)S.col16.p, (const int *)S.wtab.p, (const double *)S.val.p, x, xg,
                       (const double *)P->dinv.p, out, z, s.c_own, s.c_prod, s.c_z, s.own_from_out, list);
  else
    hipLaunchKernelGGL((k_sell_poly_step<false, LIST, GHOST>), dim3(grid), dim3(kBlock), 0, ctx->stream, S.nrow, nsl, nbp,
                       (const long long *)S.slice_off.p, (const void *)S.col.p, (const int *)nullptr, (const double *)S.val.p, x, xg,
                       (const double *)P->dinv.p, out, z, s.c_own, s.c_prod, s.c_z, s.own_from_out, list);
}

// one step: out and z from x; out != x.  With a halo plan the exchange of x overlaps the interior slices exactly as in
// spmv_dev.
inline int poly_step(isph_ctx *ctx, const isph_mat *A, const Poly *P, const PolyStep &s, const double *x, double *out, double *z) {
  const Sell &S = A->S;
  if (P->unfused) {
    ISPH_CHECK(dinv_spmv(ctx, A, nullptr, P->dinv.p, x, P->y.p, /*unfused=*/false));
    hipLaunchKernelGGL(k_poly_update, dim3(stream_grid(S.nrow)), dim3(kBlock), 0, ctx->stream, S.nrow, s.c_own, s.c_prod, s.c_z,
                       s.own_from_out, x, (const double *)P->y.p, out, z);
    ISPH_CHECK_HIP(hipGetLastError());
    return ISPH_SUCCESS;
  }
  ProfScope prof((A->local || A->aux) ? nullptr : ctx, PROF_SPMV);   // a sweep of the caller's operator, like spmv_dev's
  const bool c16 = !A->local && !A->aux && sell_cols16(ctx, S);
  if (!mat_has_halo(A)) {
    poly_step_launch<false, false>(ctx, S, c16, S.nslices, nullptr, P, s, x, nullptr, out, z);
  } else {
    const isph_halo &H = A->halo;
    ISPH_CHECK(halo_begin(ctx, A, x));
    poly_step_launch<true, false>(ctx, S, c16, H.n_int, H.list_int.p, P, s, x, nullptr, out, z);
    ISPH_CHECK_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_halo, 0));
    poly_step_launch<true, true>(ctx, S, c16, H.n_bnd, H.list_bnd.p, P, s, x, ctx->xghost.p, out, z);
  }
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

// z = p(D^-1 A) D^-1 r; r and z are n device doubles in the matrix' numbering (z may be r)
inline int poly_apply(isph_ctx *ctx, const isph_mat *A, const Poly *P, const double *r, double *z) {
  ISPH_REQUIRE(P != nullptr && P->n == A->S.nrow, "GMRES polynomial: not set up for this matrix");
  const int n = P->n;
  if (n <= 0) return ISPH_SUCCESS;
  hipLaunchKernelGGL(k_poly_first, dim3(stream_grid(n)), dim3(kBlock), 0, ctx->stream, n, P->first_cz, (const double *)P->dinv.p, r,
                     P->ra.p, z);
  double *cur = P->ra.p, *other = P->rb.p;
  for (int k = 0; k < P->nsteps; ++k) {
    ISPH_CHECK(poly_step(ctx, A, P, P->steps[k], cur, other, z));
    std::swap(cur, other);
  }
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

}  // namespace isph
