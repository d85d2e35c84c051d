// poisson_boltzmann.hpp -- the nonlinear Poisson-Boltzmann solve on the device: PairISPH::computePoissonBoltzmann
// (ref: pair_isph.cpp:573-600) with the functors it hands to SolverNOX_Stratimikos (pair_isph.h:78).
//
//   F_i = (-div(eps grad psi))_i + kappa^2 g(psi_i) + f_i     rows of kind Fluid / BufferDirichlet / BufferNeumann
//   F_i = psi0_i - psi_i (+ f_i on Boundary rows)              rows of kind Solid / Boundary
//   (functor_poisson_boltzmann_f.h:40-86, functor_poisson_boltzmann_extra_f.h:79-81)
//   g(psi) = sinh(psi) / (1 + 2 gamma sinh^2(psi/2)), linearized: psi / (1 + 2 gamma (psi/2)^2)
//   J = the Laplacian rows assembled once (MODE 3 of assemble.hpp k_asm_helmholtz) with the diagonal replaced on every
//   call (functor_poisson_boltzmann_jacobian.h:38-108): L_ii + kappa^2 g'(psi_i), -1 on the Solid / Boundary rows.
//
// The diagonal is written into S.val in place at positions found once after assembly, so F, GMRES and the
// preconditioner set-up all read the one matrix.  Nothing on isph_mat caches values derived from S.val (the 16-bit
// column windows of the SpMV are derived from S.col only).  F is the SpMV J psi followed by one streaming kernel that
// subtracts s psi with s = J_ii - L_ii, so F does not depend on the diagonal J holds at the time.
//
// Newton driver (solver_nox_impl.h:78-145, solver_nox_stratimikos.h:84-122): full step, constant forcing term, FGMRES
// with right preconditioning from x0 = 0 on J delta = -F, the preconditioner rebuilt when its age reaches "Max Age Of
// Prec" (policy Reuse), stop on FiniteValue OR MaxIters OR (NormF AND NormUpdate), unscaled global 2-norms, NormUpdate
// not satisfied before the first step.  One host read per Newton step (||F||^2, the non-finite count and the
// preceding ||delta||^2 together).

struct isph_pb_rows {
  int n = 0;
  isph::DevBuf<int> cls;          // 0 Fluid / buffer rows, 1 Solid, 2 Boundary
  isph::DevBuf<long long> dpos;   // position of the row's diagonal entry in S.val
  isph::DevBuf<double> psi0, ldiag, shift;
  isph::DevBuf<double> psi, f, F, y, rhs, delta, stage;  // Newton workspaces, matrix numbering (stage: caller's)
  void release() {
    cls.release(); dpos.release(); psi0.release(); ldiag.release(); shift.release();
    psi.release(); f.release(); F.release(); y.release(); rhs.release(); delta.release(); stage.release();
  }
};

namespace isph {

void pb_rows_destroy(isph_pb_rows *R) {
  if (!R) return;
  R->release();
  delete R;
}

enum { SC_PB = SC_MISC + 24 };  // [0] ||F||^2  [1] non-finite entries of F  [2] ||delta||^2

__device__ __forceinline__ double pb_g(double psi, double gamma, int lin) {
  if (lin) { const double h = 0.5 * psi; return psi / (1.0 + 2.0 * gamma * (h * h)); }
  const double s = sinh(0.5 * psi);
  return sinh(psi) / (1.0 + 2.0 * gamma * (s * s));
}

// the two closed forms of functor_poisson_boltzmann_jacobian.h:86-97
__device__ __forceinline__ double pb_dg(double psi, double gamma, int lin) {
  if (lin) {
    const double p2 = psi * psi;
    return (4.0 - 2.0 * gamma * p2) / (gamma * gamma * (p2 * p2) + 4.0 * gamma * p2 + 4.0);
  }
  const double sh = sinh(0.5 * psi), ch = cosh(0.5 * psi);
  const double num = 2.0 * gamma * ch * sh * sinh(psi);
  const double den = 2.0 * gamma * (sh * sh) + 1.0;
  return cosh(psi) / den - num / (den * den);
}

// row class, Dirichlet value and diagonal position of every row; bad = rows without a diagonal entry
__global__ void k_pb_rows(int n, const int *__restrict__ type, const int *__restrict__ kind, const int *__restrict__ colmap,
                          const double *__restrict__ psi0, const int *__restrict__ rowlen, const long long *__restrict__ slice_off,
                          const int *__restrict__ col, const double *__restrict__ val, int *__restrict__ cls,
                          double *__restrict__ psi0_out, long long *__restrict__ dpos, double *__restrict__ ldiag,
                          double *__restrict__ shift, int *__restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int k = kind[type[i]];
  const int c = (k & KIND_FLUID) ? 0 : (k == KIND_BOUNDARY ? 2 : 1);
  cls[i] = c;
  psi0_out[i] = (c != 0 && psi0) ? psi0[i] : 0.0;
  const long long off = slice_off[i >> 6];
  const int own = colmap[i], len = rowlen[i];
  long long p = -1;
  for (int e = 0; e < len && p < 0; ++e) {
    const long long q = sell_pos(off, i & 63, e);
    if (col[q] == own) p = q;
  }
  dpos[i] = p;
  ldiag[i] = p >= 0 ? val[p] : 0.0;
  shift[i] = 0.0;
  if (p < 0) atomicAdd(bad, 1);
}

// J_ii in place; s_i = J_ii - L_ii
__global__ void k_pb_jacobian(int n, const int *__restrict__ cls, const long long *__restrict__ dpos,
                              const double *__restrict__ ldiag, const double *__restrict__ psi, double kappasq, double gamma,
                              int lin, double *__restrict__ val, double *__restrict__ shift) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (cls[i] == 0) {
      const double j = ldiag[i] + kappasq * pb_dg(psi[i], gamma, lin);
      val[dpos[i]] = j;
      shift[i] = j - ldiag[i];
    } else {
      val[dpos[i]] = -1.0;
      shift[i] = 0.0;
    }
  }
}

// F from y = J psi; partial[b] = sum F^2, partial[nblk + b] = non-finite entries of the block
__global__ __launch_bounds__(kBlock) void k_pb_residual(int n, const int *__restrict__ cls, const double *__restrict__ psi,
                                                        const double *__restrict__ y, const double *__restrict__ shift,
                                                        const double *__restrict__ psi0, const double *__restrict__ f,
                                                        double kappasq, double gamma, int lin, double *__restrict__ F,
                                                        double *__restrict__ partial) {
  __shared__ double s0[4], s1[4];
  double p = 0.0, q = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int c = cls[i];
    const double x = psi[i];
    double v;
    if (c == 0) v = (y[i] - shift[i] * x) + kappasq * pb_g(x, gamma, lin);
    else v = psi0[i] - x;
    if (f && c != 1) v += f[i];  // Extra F on every row whose kind has no bit of Solid (extra_f.h:79-81)
    F[i] = v;
    p = fma(v, v, p);
    if (!isfinite(v)) q += 1.0;
  }
  p = wave_sum(p);
  q = wave_sum(q);
  if ((threadIdx.x & 63) == 0) { s0[threadIdx.x >> 6] = p; s1[threadIdx.x >> 6] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = (s0[0] + s0[1]) + (s0[2] + s0[3]);
    partial[gridDim.x + blockIdx.x] = (s1[0] + s1[1]) + (s1[2] + s1[3]);
  }
}

// psi += delta; partial[b] = sum delta^2
__global__ __launch_bounds__(kBlock) void k_pb_update(int n, const double *__restrict__ delta, double *__restrict__ psi,
                                                      double *__restrict__ partial) {
  __shared__ double s0[4];
  double p = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double d = delta[i];
    psi[i] += d;
    p = fma(d, d, p);
  }
  p = wave_sum(p);
  if ((threadIdx.x & 63) == 0) s0[threadIdx.x >> 6] = p;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (s0[0] + s0[1]) + (s0[2] + s0[3]);
}

// the rows of a freshly assembled Laplacian -> a Jacobian.  P: the particle view the matrix was assembled from (rows in
// the matrix' numbering); psi0 [nall] in that numbering or NULL; device arrays when on_device.
inline int pb_attach(isph_ctx *ctx, isph_mat *A, const isph_particles *P, const double *psi0, int on_device) {
  const int n = A->S.nrow;
  isph_pb_rows *R = new isph_pb_rows();
  A->pb = R;
  R->n = n;
  const size_t m = (size_t)(n > 0 ? n : 1);
  ISPH_CHECK(R->cls.reserve(m));
  ISPH_CHECK(R->dpos.reserve(m));
  ISPH_CHECK(R->psi0.reserve(m));
  ISPH_CHECK(R->ldiag.reserve(m));
  ISPH_CHECK(R->shift.reserve(m));
  if (n == 0) return ISPH_SUCCESS;
  DevTmp<int> stype, scol, kind, bad;
  DevTmp<double> spsi0;
  const int *dtype = nullptr, *dcol = nullptr;
  const double *dpsi0 = nullptr;
  ISPH_CHECK(stage_in(ctx, P->type, (size_t)n, on_device, stype, &dtype));
  ISPH_CHECK(stage_in(ctx, P->colmap, (size_t)n, on_device, scol, &dcol));
  if (psi0) ISPH_CHECK(stage_in(ctx, psi0, (size_t)n, on_device, spsi0, &dpsi0));
  ISPH_CHECK(kind.reserve((size_t)P->ntypes + 1));
  ISPH_CHECK(bad.reserve(1));
  ISPH_CHECK_HIP(hipMemcpyAsync(kind.p, P->kind, sizeof(int) * ((size_t)P->ntypes + 1), hipMemcpyHostToDevice, ctx->stream));
  ISPH_CHECK_HIP(hipMemsetAsync(bad.p, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL(k_pb_rows, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, n, dtype, (const int *)kind.p, dcol,
                     dpsi0, (const int *)A->S.rowlen.p, (const long long *)A->S.slice_off.p, (const int *)A->S.col.p,
                     (const double *)A->S.val.p, R->cls.p, R->psi0.p, R->dpos.p, R->ldiag.p, R->shift.p, bad.p);
  int hbad = 0;
  ISPH_CHECK_HIP(hipMemcpyAsync(&hbad, bad.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  ISPH_CHECK_HIP(hipGetLastError());
  ISPH_REQUIRE(hbad == 0, "Poisson-Boltzmann Jacobian: a row without a diagonal entry");
  return ISPH_SUCCESS;
}

inline int pb_check_params(const isph_pb_params *p) {
  ISPH_REQUIRE(p->max_iters >= 0 && p->prec_max_age >= 1, "need max_iters >= 0 and prec_max_age >= 1");
  ISPH_REQUIRE(p->prec_kind == 0 || p->prec_kind == 1, "prec_kind: 0 SA-AMG, 1 block-Jacobi ILU(0)");
  ISPH_REQUIRE(p->linear.solver_type == 0, "the Newton step's linear solve is GMRES (solver_type 0)");
  ISPH_REQUIRE(!(p->prec_kind == 0 && p->amg.cycle_bits == 32 && p->linear.flexible == 0),
               "amg.cycle_bits = 32 needs linear.flexible = 1: the rounded cycle is not a linear operator");
  return ISPH_SUCCESS;
}

// a caller vector [nlocal] (host or device, caller's numbering) -> dst (device, matrix numbering)
inline int pb_in(isph_ctx *ctx, const isph_mat *J, const double *src, int on_device, double *dst) {
  const int n = J->S.nrow;
  isph_pb_rows *R = J->pb;
  if (n == 0) return ISPH_SUCCESS;
  const double *d = src;
  if (!on_device) {
    ISPH_REQUIRE(!is_device_pointer(src), "device pointer passed with on_device = 0");
    ISPH_CHECK(R->stage.reserve((size_t)n));
    ISPH_CHECK_HIP(hipMemcpyAsync(R->stage.p, src, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    d = R->stage.p;
  }
  if (J->order)
    order_gather(ctx, *J->order, n, 1, d, 0, dst, 0);
  else
    ISPH_CHECK_HIP(hipMemcpyAsync(dst, d, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
  return ISPH_SUCCESS;
}

// src (device, matrix numbering) -> the caller's vector [nlocal]; the stream is drained on return
inline int pb_out(isph_ctx *ctx, const isph_mat *J, const double *src, double *out, int on_device) {
  const int n = J->S.nrow;
  isph_pb_rows *R = J->pb;
  if (n > 0) {
    double *d = out;
    if (!on_device) { ISPH_CHECK(R->stage.reserve((size_t)n)); d = R->stage.p; }
    if (J->order)
      order_scatter(ctx, *J->order, n, 1, src, 0, d, 0);
    else
      ISPH_CHECK_HIP(hipMemcpyAsync(d, src, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
    if (!on_device) ISPH_CHECK_HIP(hipMemcpyAsync(out, d, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  }
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

inline int pb_workspaces(isph_pb_rows *R) {
  const size_t m = (size_t)R->n + 64;
  ISPH_CHECK(R->psi.reserve(m));
  ISPH_CHECK(R->f.reserve(m));
  ISPH_CHECK(R->F.reserve(m));
  ISPH_CHECK(R->y.reserve(m));
  ISPH_CHECK(R->rhs.reserve(m));
  ISPH_CHECK(R->delta.reserve(m));
  return ISPH_SUCCESS;
}

// computeF: F (matrix numbering) from psi / f (matrix numbering, f may be NULL); ||F||^2 and the non-finite count go to
// dscal[SC_PB], [SC_PB + 1], all-reduced (collective)
inline int pb_residual_dev(isph_ctx *ctx, const isph_mat *J, const isph_pb_params *p, const double *psi, const double *f, double *F) {
  isph_pb_rows *R = J->pb;
  const int n = R->n;
  ISPH_CHECK(ensure_scalars(ctx));
  ISPH_CHECK(spmv_dev(ctx, J, psi, R->y.p, nullptr));  // ghost values of psi through the matrix' halo
  const int g = stream_grid(n);
  hipLaunchKernelGGL(k_pb_residual, dim3(g), dim3(kBlock), 0, ctx->stream, n, (const int *)R->cls.p, psi, (const double *)R->y.p,
                     (const double *)R->shift.p, (const double *)R->psi0.p, f, p->kappasq, p->gamma, p->linearized, F,
                     ctx->partial.p);
  hipLaunchKernelGGL(k_reduce_partials, dim3(2), dim3(kBlock), 0, ctx->stream, 2, g, (const double *)ctx->partial.p,
                     ctx->dscal.p + SC_PB);
  return allreduce_inplace(ctx, ctx->dscal.p + SC_PB, 2);
}

// computeJacobian: the diagonal of J from psi (matrix numbering)
inline int pb_jacobian_dev(isph_ctx *ctx, isph_mat *J, const isph_pb_params *p, const double *psi) {
  isph_pb_rows *R = J->pb;
  if (R->n > 0)
    hipLaunchKernelGGL(k_pb_jacobian, dim3(stream_grid(R->n)), dim3(kBlock), 0, ctx->stream, R->n, (const int *)R->cls.p,
                       (const long long *)R->dpos.p, (const double *)R->ldiag.p, psi, p->kappasq, p->gamma, p->linearized,
                       J->S.val.p, R->shift.p);
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

inline int pb_build_prec(isph_ctx *ctx, const isph_mat *J, const isph_pb_params *p, isph_prec **M) {
  if (p->prec_kind == 0) return isph_prec_create_amg(ctx, J, &p->amg, nullptr, 1, M);
  // ILU(0) per brick of the library's numbering; blocks of 512 rows in the caller's
  return isph_prec_create(ctx, J, "bjacobi-ilu0", J->order ? 0 : 512, M);
}

}  // namespace isph

// the Poisson-Boltzmann Laplacian in the library's own row numbering when the context asks for it
static int assemble_pb(isph_ctx *ctx, const isph_particles *P, int antisym, const double *eps, const double *psi0, int ncol,
                       isph_mat **J_out, int on_device) {
  isph_mat *A = nullptr;
  int rc = ISPH_SUCCESS;
  if (!ctx->ordering || P->nlocal <= 0) {
    ISPH_CHECK(assemble_helmholtz(ctx, P, antisym, -1.0, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, ncol, &A,
                                  nullptr, P->nlocal, on_device, 3, nullptr, eps));
    rc = pb_attach(ctx, A, P, psi0, on_device);
  } else {
    OrderedAssembly W(ctx, P, on_device);
    ISPH_CHECK(W.begin(ncol));
    const double *deps = nullptr, *dpsi0 = nullptr;
    ISPH_CHECK(W.field(eps, 1, true, &deps));
    ISPH_CHECK(W.field(psi0, 1, true, &dpsi0));
    ISPH_CHECK(assemble_helmholtz(ctx, &W.Q, antisym, -1.0, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, ncol, &A,
                                  nullptr, P->nlocal, 1, 3, nullptr, deps));
    A->order = W.O;
    rc = pb_attach(ctx, A, &W.Q, dpsi0, 1);
  }
  if (rc != ISPH_SUCCESS) { isph_mat_destroy(A); return rc; }
  *J_out = A;
  return ISPH_SUCCESS;
}

extern "C" {

void isph_pb_params_default(isph_pb_params *p) {
  // PairISPH's pb defaults (pair_isph.cpp:1680-1698) and SolverNOX_Stratimikos' lists (solver_nox_impl.h:78-145,
  // solver_nox_stratimikos.h:84-122)
  p->kappasq = 1.0;
  p->gamma = 0.0;
  p->linearized = 0;
  p->max_iters = 100;
  p->f_tol = 1e-8;
  p->update_tol = 1e-5;
  p->prec_max_age = 10;
  p->prec_kind = 0;
  isph_amg_params_default(&p->amg);
  isph_solver_params_default(&p->linear);
  p->linear.solver_type = 0;
  p->linear.tol = 1e-6;
  p->linear.max_iters = 80;
  p->prec_refresh = 0;
}

int isph_assemble_poisson_boltzmann(isph_ctx *ctx, const isph_particles *P, int antisym, const double *eps, const double *psi0,
                                    int ncol, isph_mat **J_out, int on_device) {
  ISPH_REQUIRE(ctx && P && J_out, "NULL argument");
  return assemble_pb(ctx, P, antisym, eps, psi0, ncol, J_out, on_device);
}

int isph_pb_residual(isph_ctx *ctx, const isph_mat *J, const isph_pb_params *prm, const double *psi, const double *f,
                     double *F_out, int on_device) {
  ISPH_REQUIRE(ctx && J && prm && psi && F_out, "NULL argument");
  ISPH_REQUIRE(J->pb, "not a Poisson-Boltzmann Jacobian (isph_assemble_poisson_boltzmann)");
  isph_pb_rows *R = J->pb;
  ISPH_CHECK(pb_workspaces(R));
  ISPH_CHECK(pb_in(ctx, J, psi, on_device, R->psi.p));
  if (f) ISPH_CHECK(pb_in(ctx, J, f, on_device, R->f.p));
  ISPH_CHECK(pb_residual_dev(ctx, J, prm, R->psi.p, f ? R->f.p : nullptr, R->F.p));
  return pb_out(ctx, J, R->F.p, F_out, on_device);
}

int isph_pb_jacobian(isph_ctx *ctx, isph_mat *J, const isph_pb_params *prm, const double *psi, int on_device) {
  ISPH_REQUIRE(ctx && J && prm && psi, "NULL argument");
  ISPH_REQUIRE(J->pb, "not a Poisson-Boltzmann Jacobian (isph_assemble_poisson_boltzmann)");
  isph_pb_rows *R = J->pb;
  ISPH_CHECK(pb_workspaces(R));
  ISPH_CHECK(pb_in(ctx, J, psi, on_device, R->psi.p));
  ISPH_CHECK(pb_jacobian_dev(ctx, J, prm, R->psi.p));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

int isph_solve_poisson_boltzmann(isph_ctx *ctx, isph_mat *J, const isph_pb_params *prm_in, const double *f, double *psi,
                                 isph_pb_info *info, int on_device) {
  ISPH_REQUIRE(ctx && J && psi && info, "NULL argument");
  ISPH_REQUIRE(J->pb, "not a Poisson-Boltzmann Jacobian (isph_assemble_poisson_boltzmann)");
  isph_pb_params prm;
  if (prm_in) prm = *prm_in; else isph_pb_params_default(&prm);
  ISPH_CHECK(pb_check_params(&prm));
  memset(info, 0, sizeof(*info));
  isph_pb_rows *R = J->pb;
  const int n = R->n;
  ISPH_CHECK(ensure_scalars(ctx));
  ISPH_CHECK(pb_workspaces(R));
  hipStream_t st = ctx->stream;
  ISPH_CHECK_HIP(hipEventRecord(ctx->ev0, st));
  ISPH_CHECK(pb_in(ctx, J, psi, on_device, R->psi.p));
  if (f) ISPH_CHECK(pb_in(ctx, J, f, on_device, R->f.p));
  const double *df = f ? R->f.p : nullptr;
  isph_prec *M = nullptr;
  int age = 0, status = 2, it = 0, rc = ISPH_SUCCESS;
  double norm_f = 0.0, norm_u = 0.0;
  const int sg = stream_grid(n);
  for (;; ++it) {
    rc = pb_residual_dev(ctx, J, &prm, R->psi.p, df, R->F.p);
    if (rc == ISPH_SUCCESS) rc = fetch_scalars(ctx, SC_PB, 3);  // the step's one host read: ||F||^2, non-finite, ||delta||^2
    if (rc != ISPH_SUCCESS) break;
    norm_f = std::sqrt(ctx->hscal[SC_PB]);
    if (it > 0) norm_u = std::sqrt(ctx->hscal[SC_PB + 2]);
    // Combo OR in the reference's order: FiniteValue, MaxIters, Combo AND (NormF, NormUpdate)
    if (ctx->hscal[SC_PB + 1] != 0.0 || !std::isfinite(norm_f)) status = -1;
    else if (it >= prm.max_iters) status = 0;
    else if (it > 0 && norm_f < prm.f_tol && norm_u < prm.update_tol) status = 1;
    if (status != 2) break;
    rc = pb_jacobian_dev(ctx, J, &prm, R->psi.p);
    if (rc == ISPH_SUCCESS && (!M || age >= prm.prec_max_age)) {  // "Preconditioner Reuse Policy" = Reuse
      // prec_refresh: the preconditioner of the first step was created while the pattern was held; its values are redone
      // where the type can be refactored (an SA-AMG across ranks or on a matrix with a halo is not held: rebuilt)
      if (M && prm.prec_refresh && (prec_ilu(M) || (prec_amg(M) && M->amg->held))) {
        rc = isph_prec_refactor(ctx, M, J);
        ++info->prec_refreshes;
      } else {
        if (M) { isph_prec_destroy(M); M = nullptr; }
        const bool hold0 = ctx->pattern_hold;
        if (prm.prec_refresh) ctx->pattern_hold = true;
        rc = pb_build_prec(ctx, J, &prm, &M);
        ctx->pattern_hold = hold0;
      }
      age = 0;
      ++info->prec_builds;
    }
    if (rc != ISPH_SUCCESS) break;
    ++age;
    if (n > 0) {
      hipLaunchKernelGGL(k_scale_copy<double>, dim3(sg), dim3(kBlock), 0, st, n, (const double *)R->F.p, R->rhs.p, -1.0,
                         (const double *)nullptr, 0);
      rc = hipMemsetAsync(R->delta.p, 0, sizeof(double) * (size_t)n, st) == hipSuccess ? ISPH_SUCCESS
                                                                                        : fail("memset failed", __FILE__, __LINE__);
    }
    if (rc != ISPH_SUCCESS) break;
    LinOp op{ctx, J, M, nullptr, n};
    isph_solve_info li;
    memset(&li, 0, sizeof(li));
    rc = gmres(op, R->rhs.p, R->delta.p, &prm.linear, &li);
    if (rc != ISPH_SUCCESS) break;
    info->linear_iters += li.iters;
    hipLaunchKernelGGL(k_pb_update, dim3(sg), dim3(kBlock), 0, st, n, (const double *)R->delta.p, R->psi.p, ctx->partial.p);
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kBlock), 0, st, 1, sg, (const double *)ctx->partial.p, ctx->dscal.p + SC_PB + 2);
    rc = allreduce_inplace(ctx, ctx->dscal.p + SC_PB + 2, 1);
    if (rc != ISPH_SUCCESS) break;
    info->newton_iters = it + 1;
  }
  if (M) isph_prec_destroy(M);
  ISPH_CHECK(rc);
  ISPH_CHECK(pb_out(ctx, J, R->psi.p, psi, on_device));
  ISPH_CHECK_HIP(hipEventRecord(ctx->ev1, st));
  ISPH_CHECK_HIP(hipEventSynchronize(ctx->ev1));
  float ms = 0.f;
  ISPH_CHECK_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  info->status = status;
  info->norm_f = norm_f;
  info->norm_update = norm_u;
  info->ms = ms;
  return ISPH_SUCCESS;
}

}  // extern "C"
