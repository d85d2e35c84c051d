// body_force.hpp -- the two remaining producers of the body force `force`: the electrostatic force of the electrokinetic
// step and the random stress of the fluctuating step.  Included at the end of isph_capi.hip.
//
// Replaces
//   FunctorOuterSmoothField, scalar form                                 (ref: functor_smooth_field.h:43-106)
//   PairISPH_Corrected::computePsiGradient                               (ref: pair_isph_corrected.cpp:540-565)
//     Corrected::FunctorOuterGradient / FunctorOuterGradient_MorrisHolmes (ref: functor_gradient.h:80-169,
//                                                                              functor_boundary_morris_holmes.h:99-102)
//   PairISPH_Corrected::computePhiGradient                               (ref: pair_isph_corrected.cpp:621-651)
//   PairISPH::computeElectrostaticForce                                  (ref: pair_isph.cpp:679-687)
//     FunctorOuterElectrostaticForce                                     (ref: functor_electrostatic_force.h:39-56)
//   PairISPH::computeRandomStressTensor                                  (ref: pair_isph.cpp:710-758)
//   PairISPH_Corrected::computeForceFromRandomStress                     (ref: pair_isph_corrected.cpp:130-132, 812-826)
//     FunctorOuterRandomStress<FunctorOuterDivergenceAntiSymmetric>      (ref: functor_random_stress.h:54-74)
//
// The electrokinetic chain is three loops over the particles in the reference (two gradient functors, one pointwise
// force functor) with two [nmax][3] arrays between them.  Both gradients walk the same neighbour list with the same
// positions, kernel derivative and G_i^T r_ij and differ in the field, the filter of j and the mirror weight, so they are
// ONE sweep here; the buffer-row override and the force are pointwise on the lane that summed the gradients and are its
// epilogue.  The random stress is three divergence functors per particle in the reference, one per column of the
// tensor; one sweep here gathers the neighbour's packed tensor (48 bytes) once and accumulates the dim columns.
// Like the gradient / divergence operators these sweeps work in the caller's particle numbering; one lane per particle,
// the lane-interleaved neighbour list, pair_rsq for every cut test.
#pragma once
#include "philox.hpp"
#include "surface_tension.hpp"

namespace isph {

// sf_i = f_i W(0, h_ii) V_i + sum_j f_j W(r_ij) V_j; a row whose kind fails the filter is not written
__global__ __launch_bounds__(kBlock) void k_smooth_field(AsmTables T, OpArgs a, const double *__restrict__ f,
                                                         double *__restrict__ sf) {
  const int i = xcd_block() * blockDim.x + threadIdx.x;
  if (i >= a.nlocal) return;
  const int dim = T.dim, nt1 = T.ntypes + 1, it = a.type[i], ikind = T.kind[it];
  if (a.use_filter && !(ikind & a.filt_i)) return;
  double s = f[i] * (kernel_val(T.kernel, 0.0, T.hinv[it * nt1 + it], T.knorm[it * nt1 + it]) * a.vfrac[i]);
  for (int jj = 0, je = T.nlen[i]; jj < je; ++jj) {
    const int j = neigh_at(T, i, jj);
    const int jt = a.type[j];
    if (a.use_filter && !(T.kind[jt] & a.filt_j)) continue;
    double rij[3];
    const double rsq = pair_rsq(dim, a.x, i, j, rij);
    if (!(rsq < T.cutsq[it * nt1 + jt])) continue;
    const double r = sqrt(rsq) + kEps;
    const double w = kernel_val(T.kernel, r, T.hinv[it * nt1 + jt], T.knorm[it * nt1 + jt]);
    s += f[j] * (w * a.vfrac[j]);
  }
  sf[i] = s;
}

struct EkArgs {
  double ezcb, psiref, gamma;
  double pb_e[3], ae_e[3];
  int morris;                 // MirrorMorrisHolmes on the psi gradient
  double safe;
  const double *pnd;          // [nall], read for Solid neighbours (and the row) when morris
  const double *psi, *phi;    // [nall]; phi may be NULL
  double *psigrad, *phigrad;  // [nlocal][3] or NULL
  double *f;                  // [nlocal][3] or NULL
};

// grad psi with (Fluid, All) and the mirror, grad phi with (Fluid, Fluid) and the buffer-row override, then
// f_i -= ezcb 2 sinh(psi_i) / (1 + 2 gamma sinh^2(psi_i / 2)) (-psiref grad psi_i + e), e = -grad phi_i or pb_e
template <int DIM, int FAM>  // FAM 0 Symmetric (G = Gc[i]), 1 AntiSymmetric (G = I, V = sqrt(V_i V_j))
__global__ __launch_bounds__(kBlock) void k_ek_force(AsmTables T, OpArgs a, EkArgs e) {
  const int i = xcd_block() * blockDim.x + threadIdx.x;
  if (i >= a.nlocal) return;
  const int nt1 = T.ntypes + 1, it = a.type[i], ikind = T.kind[it];
  const double psii = e.psi[i];
  double gpsi[3] = {0, 0, 0}, gphi[3] = {0, 0, 0};
  if (ikind & KIND_FLUID) {
    double G[DIM * DIM];
    if (FAM == 0)
      for (int k = 0; k < DIM * DIM; ++k) G[k] = a.Gc[(size_t)i * DIM * DIM + k];
    const bool with_phi = e.phi != nullptr;
    const double vi = a.vfrac[i], phii = with_phi ? e.phi[i] : 0.0;
    const bool free_i = !(ikind & KIND_SOLID);
    for (int jj = 0, je = T.nlen[i]; jj < je; ++jj) {
      const int j = neigh_at(T, i, jj);
      const int jt = a.type[j], jkind = T.kind[jt];
      const bool in_psi = (jkind & KIND_ALL) != 0, in_phi = with_phi && (jkind & KIND_FLUID);
      if (!in_psi && !in_phi) continue;
      double rij[3];
      const double rsq = pair_rsq(DIM, a.x, i, j, rij);
      const double cutsq = T.cutsq[it * nt1 + jt];
      if (!(rsq < cutsq)) continue;
      const double r = sqrt(rsq) + kEps;
      const double dwdr = kernel_dval(T.kernel, r, T.hinv[it * nt1 + jt], T.kdnorm[it * nt1 + jt]);
      const double vj = a.vfrac[j];
      const double w = dwdr / r * (FAM ? sqrt(vi * vj) : vj);
      double gr[3];
      if (FAM) { gr[0] = rij[0]; gr[1] = rij[1]; gr[2] = rij[2]; }
      else gt_times_r<DIM>(G, rij, gr);
      if (in_psi) {
        double coeff = 1.0;
        if (e.morris && free_i && (jkind & KIND_SOLID))
          coeff = mirror_coeff(e.pnd, a.vfrac, e.safe, T.h[it * nt1 + jt], i, j, sqrt(cutsq));
        const double vjtmp = w * coeff;
        const double d = FAM ? (psii + e.psi[j]) : (e.psi[j] - psii);
        for (int k = 0; k < DIM; ++k) gpsi[k] += gr[k] * vjtmp * d;
      }
      if (in_phi) {
        const double d = FAM ? (phii + e.phi[j]) : (e.phi[j] - phii);
        for (int k = 0; k < DIM; ++k) gphi[k] += gr[k] * w * d;
      }
    }
  }
  // the buffer area holds the constant gradient of the applied field (pair_isph_corrected.cpp:643-650)
  if (e.phi && (ikind == KIND_BUFFER_DIRICHLET || ikind == KIND_BUFFER_NEUMANN))
    for (int k = 0; k < 3; ++k) gphi[k] = -e.ae_e[k];
  if (e.psigrad)
    for (int k = 0; k < 3; ++k) e.psigrad[3 * (size_t)i + k] = gpsi[k];
  if (e.phigrad && e.phi)
    for (int k = 0; k < 3; ++k) e.phigrad[3 * (size_t)i + k] = gphi[k];
  if (e.f) {
    const double sh = sinh(psii), sh2 = sinh(psii / 2.0);
    const double c = e.ezcb * 2.0 * sh / (1.0 + 2.0 * e.gamma * (sh2 * sh2));
    for (int k = 0; k < DIM; ++k) {
      const double ek = e.phi ? -gphi[k] : e.pb_e[k];
      e.f[3 * (size_t)i + k] -= c * (-e.psiref * gpsi[k] + ek);
    }
  }
}

// the packed slot of T[a][b], a <= b: (0,0), (0,1), (1,1), (0,2), (1,2), (2,2) -- the order of Lc
__host__ __device__ constexpr int sym6(int a, int b) { return a <= b ? b * (b + 1) / 2 + a : a * (a + 1) / 2 + b; }

// computeRandomStressTensor on the rows with kind & Fluid, zeros elsewhere.  DEPARTURE from the reference: the dim^2
// normals are a function of (seed, step, tag) -- key = seed, counter = (tag, block, step) -- not the next numbers of the
// rank's RanMars stream in ilist order.
template <int DIM>
__global__ __launch_bounds__(kBlock) void k_random_stress_tensor(int nlocal, const int *__restrict__ type,
                                                                 const int *__restrict__ kind, const int *__restrict__ tag,
                                                                 unsigned long long seed, unsigned long long step,
                                                                 double *__restrict__ rs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nlocal) return;
  double t6[6] = {0, 0, 0, 0, 0, 0};
  if (kind[type[i]] & KIND_FLUID) {
    constexpr int nblock = (DIM * DIM + 1) / 2;
    double g[2 * nblock];
#pragma unroll
    for (int b = 0; b < nblock; ++b) {
      unsigned o[4];
      philox4x32_10((unsigned)tag[i], (unsigned)b, (unsigned)step, (unsigned)(step >> 32), (unsigned)seed,
                    (unsigned)(seed >> 32), o);
      const double u1 = philox_uniform(o[0], o[1]), u2 = philox_uniform(o[2], o[3]);
      const double rad = sqrt(-2.0 * log(u1)), ang = 6.283185307179586 * u2;
      g[2 * b] = rad * cos(ang);
      g[2 * b + 1] = rad * sin(ang);
    }
    double Tm[DIM][DIM], trace = 0.0;
#pragma unroll
    for (int k2 = 0; k2 < DIM; ++k2)
#pragma unroll
      for (int k1 = 0; k1 < DIM; ++k1) Tm[k2][k1] = 0.5 * (g[k2 * DIM + k1] + g[k1 * DIM + k2]);
    for (int k = 0; k < DIM; ++k) trace += Tm[k][k];
    for (int k = 0; k < DIM; ++k) Tm[k][k] -= trace / DIM;
#pragma unroll
    for (int b = 0; b < DIM; ++b)
#pragma unroll
      for (int c = 0; c <= b; ++c) t6[sym6(c, b)] = Tm[c][b];
  }
  double2 *out = reinterpret_cast<double2 *>(rs + 6 * (size_t)i);
  out[0] = make_double2(t6[0], t6[1]);
  out[1] = make_double2(t6[2], t6[3]);
  out[2] = make_double2(t6[4], t6[5]);
}

// the tensor of list entry j: its own slot when the caller filled the ghosts, else through the column map
__device__ __forceinline__ void rs_record(const double *__restrict__ rs, const int *__restrict__ colmap,
                                          const double *__restrict__ ghosts, int nlocal, int nghost, int j, double t[6]) {
  const double *src = rs + 6 * (size_t)j;
  if (colmap && j >= nlocal) {
    const int col = colmap[j];
    if (col < 0) src = nullptr;
    else if (col < nlocal) src = rs + 6 * (size_t)col;
    else if (ghosts && col - nlocal < nghost) src = ghosts + 6 * (size_t)(col - nlocal);
    else src = nullptr;
  }
  if (!src) { t[0] = t[1] = t[2] = t[3] = t[4] = t[5] = 0.0; return; }
  const double2 *s2 = reinterpret_cast<const double2 *>(src);
  const double2 a = s2[0], b = s2[1], c = s2[2];
  t[0] = a.x; t[1] = a.y; t[2] = b.x; t[3] = b.y; t[4] = c.x; t[5] = c.y;
}

// d_c = -sum_j r_ij . (T_i[:, c] + T_j[:, c]) W'/r sqrt(V_i V_j), f_i[c] += d_c sqrt(2 kBT nu_i rho_i / dt / V_i):
// FunctorOuterDivergenceAntiSymmetric with alpha = -1 on every column of the tensor in one sweep, (Fluid, Fluid)
template <int DIM>
__global__ __launch_bounds__(kBlock) void k_random_stress_force(AsmTables T, OpArgs a, double dt, double kBT,
                                                                const double *__restrict__ nu, const double *__restrict__ rho,
                                                                const double *__restrict__ rs, const int *__restrict__ colmap,
                                                                const double *__restrict__ ghosts, int nghost,
                                                                double *__restrict__ f) {
  const int i = xcd_block() * blockDim.x + threadIdx.x;
  if (i >= a.nlocal) return;
  const int nt1 = T.ntypes + 1, it = a.type[i];
  if (!(T.kind[it] & KIND_FLUID)) return;
  double ti[6], d[3] = {0, 0, 0};
  rs_record(rs, nullptr, nullptr, a.nlocal, 0, i, ti);
  const double vi = a.vfrac[i];
  for (int jj = 0, je = T.nlen[i]; jj < je; ++jj) {
    const int j = neigh_at(T, i, jj);
    const int jt = a.type[j];
    if (!(T.kind[jt] & KIND_FLUID)) continue;
    double rij[3];
    const double rsq = pair_rsq(DIM, a.x, i, j, rij);
    if (!(rsq < T.cutsq[it * nt1 + jt])) continue;
    const double r = sqrt(rsq) + kEps;
    const double dwdr = kernel_dval(T.kernel, r, T.hinv[it * nt1 + jt], T.kdnorm[it * nt1 + jt]);
    const double vjtmp = dwdr / r * sqrt(vi * a.vfrac[j]);
    double tj[6];
    rs_record(rs, colmap, ghosts, a.nlocal, nghost, j, tj);
#pragma unroll
    for (int c = 0; c < DIM; ++c)
#pragma unroll
      for (int k = 0; k < DIM; ++k) d[c] += rij[k] * (ti[sym6(k, c)] + tj[sym6(k, c)]) * vjtmp;
  }
  const double sq_variance = sqrt(2.0 * kBT * nu[i] * rho[i] / dt / vi);
  for (int c = 0; c < DIM; ++c) f[3 * (size_t)i + c] += d[c] * -1.0 * sq_variance;
}

inline bool rs_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int smooth_field(isph_ctx *ctx, const isph_particles *P, const double *f, int use_filter, int filt_i, int filt_j,
                        double *sf_out, int on_device) {
  // no correction tensor enters: staged as the AntiSymmetric family is
  OpStage st;
  int rc = op_stage(ctx, P, /*antisym=*/1, on_device, st);
  const int n = P->nlocal;
  DevTmp<double> tf;
  InOut out;  // rows that fail the filter keep the caller's values
  const double *df = nullptr;
  if (rc == ISPH_SUCCESS) rc = stage(ctx, f, (size_t)P->nall, on_device, tf, &df);
  if (rc == ISPH_SUCCESS) rc = out.open(ctx, sf_out, (size_t)n, on_device);
  if (rc == ISPH_SUCCESS && n > 0) {
    st.a.use_filter = use_filter; st.a.filt_i = filt_i; st.a.filt_j = filt_j;
    hipLaunchKernelGGL(k_smooth_field, dim3(xcd_grid((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, st.T, st.a, df,
                       out.dev);
    if (out.close(ctx) != ISPH_SUCCESS) rc = ISPH_FAILURE;
    rc = st_sync(ctx, rc, "smooth-field kernel failed");
  }
  out.buf.release();
  st.release();
  return rc;
}

inline void launch_ek_force(isph_ctx *ctx, const OpStage &st, const EkArgs &e) {
  const dim3 grid(xcd_grid((st.a.nlocal + kBlock - 1) / kBlock));
  if (st.T.dim == 3 && st.a.antisym) hipLaunchKernelGGL((k_ek_force<3, 1>), grid, dim3(kBlock), 0, ctx->stream, st.T, st.a, e);
  else if (st.T.dim == 3) hipLaunchKernelGGL((k_ek_force<3, 0>), grid, dim3(kBlock), 0, ctx->stream, st.T, st.a, e);
  else if (st.a.antisym) hipLaunchKernelGGL((k_ek_force<2, 1>), grid, dim3(kBlock), 0, ctx->stream, st.T, st.a, e);
  else hipLaunchKernelGGL((k_ek_force<2, 0>), grid, dim3(kBlock), 0, ctx->stream, st.T, st.a, e);
}

inline int electrostatic_force(isph_ctx *ctx, const isph_particles *P, int antisym, const isph_ek_params *prm,
                               const double *psi, const double *phi, double *psigrad_out, double *phigrad_out,
                               double *f_inout, int on_device) {
  OpStage st;
  int rc = op_stage(ctx, P, antisym, on_device, st);
  const int n = P->nlocal, n1 = n > 0 ? n : 1;
  EkArgs e;
  memset(&e, 0, sizeof(e));
  e.ezcb = prm->ezcb; e.psiref = prm->psiref; e.gamma = prm->gamma;
  for (int k = 0; k < 3; ++k) { e.pb_e[k] = prm->pb_e[k]; e.ae_e[k] = prm->ae_e[k]; }
  e.morris = P->morris_holmes ? 1 : 0; e.safe = P->morris_safe_coeff;
  DevTmp<double> tpsi, tphi, tgpsi, tgphi;
  InOut fio;
  if (rc == ISPH_SUCCESS && e.morris) rc = stage(ctx, P->pnd, (size_t)P->nall, on_device, st.S.pnd, &e.pnd);
  if (rc == ISPH_SUCCESS) rc = stage(ctx, psi, (size_t)P->nall, on_device, tpsi, &e.psi);
  if (rc == ISPH_SUCCESS) rc = stage(ctx, phi, (size_t)P->nall, on_device, tphi, &e.phi);
  const bool want_phigrad = phigrad_out && phi;
  e.psigrad = psigrad_out; e.phigrad = want_phigrad ? phigrad_out : nullptr;
  if (rc == ISPH_SUCCESS && !on_device) {
    if (psigrad_out) { rc = tgpsi.reserve((size_t)n1 * 3); e.psigrad = tgpsi.p; }
    if (rc == ISPH_SUCCESS && want_phigrad) { rc = tgphi.reserve((size_t)n1 * 3); e.phigrad = tgphi.p; }
  }
  if (rc == ISPH_SUCCESS && f_inout) { rc = fio.open(ctx, f_inout, (size_t)n * 3, on_device); e.f = fio.dev; }
  if (rc == ISPH_SUCCESS && n > 0) {
    launch_ek_force(ctx, st, e);
    if (f_inout && fio.close(ctx) != ISPH_SUCCESS) rc = ISPH_FAILURE;
    if (!on_device &&
        ((psigrad_out && hipMemcpyAsync(psigrad_out, e.psigrad, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) ||
         (want_phigrad && hipMemcpyAsync(phigrad_out, e.phigrad, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)))
      rc = fail("copy failed", __FILE__, __LINE__);
    rc = st_sync(ctx, rc, "electrostatic-force kernel failed");
  }
  fio.buf.release();
  st.release();
  return rc;
}

inline void launch_random_stress_tensor(isph_ctx *ctx, int dim, int n, const int *type, const int *kind, const int *tag,
                                        unsigned long long seed, unsigned long long step, double *rs) {
  const dim3 grid((n + kBlock - 1) / kBlock);
  if (dim == 3) hipLaunchKernelGGL(k_random_stress_tensor<3>, grid, dim3(kBlock), 0, ctx->stream, n, type, kind, tag, seed, step, rs);
  else hipLaunchKernelGGL(k_random_stress_tensor<2>, grid, dim3(kBlock), 0, ctx->stream, n, type, kind, tag, seed, step, rs);
}

inline void launch_random_stress_force(isph_ctx *ctx, const OpStage &st, double dt, double kBT, const double *nu,
                                       const double *rho, const double *rs, const int *colmap, const double *ghosts,
                                       int nghost, double *f) {
  const dim3 grid(xcd_grid((st.a.nlocal + kBlock - 1) / kBlock));
  if (st.T.dim == 3)
    hipLaunchKernelGGL(k_random_stress_force<3>, grid, dim3(kBlock), 0, ctx->stream, st.T, st.a, dt, kBT, nu, rho, rs, colmap,
                       ghosts, nghost, f);
  else
    hipLaunchKernelGGL(k_random_stress_force<2>, grid, dim3(kBlock), 0, ctx->stream, st.T, st.a, dt, kBT, nu, rho, rs, colmap,
                       ghosts, nghost, f);
}

// the tensor kernel reads the types and the kind table only: no neighbour list is staged for it
struct RsTensorStage {
  DevTmp<int> type, kind, tag;
  const int *dtype = nullptr, *dkind = nullptr, *dtag = nullptr;
};

inline int rs_tensor_stage(isph_ctx *ctx, const isph_particles *P, const int *tag, int on_device, RsTensorStage &ts) {
  ISPH_REQUIRE(P->dim == 2 || P->dim == 3, "dim must be 2 or 3");
  ISPH_REQUIRE(P->type && P->kind, "particle arrays missing");
  ISPH_CHECK(stage(ctx, P->type, (size_t)P->nlocal, on_device, ts.type, &ts.dtype));
  ISPH_CHECK(stage(ctx, P->kind, (size_t)P->ntypes + 1, 0, ts.kind, &ts.dkind));
  ISPH_CHECK(stage(ctx, tag, (size_t)P->nlocal, on_device, ts.tag, &ts.dtag));
  return ISPH_SUCCESS;
}

inline int random_stress_tensor(isph_ctx *ctx, const isph_particles *P, const int *tag, unsigned long long seed,
                                unsigned long long step, double *rs_out, int on_device) {
  ISPH_REQUIRE(!on_device || rs_aligned(rs_out), "rs_out must be 16-byte aligned device memory");
  RsTensorStage ts;
  int rc = rs_tensor_stage(ctx, P, tag, on_device, ts);
  const int n = P->nlocal;
  DevTmp<double> tr;
  double *dr = rs_out;
  if (rc == ISPH_SUCCESS && !on_device) { rc = tr.reserve((size_t)(n > 0 ? n : 1) * 6); dr = tr.p; }
  if (rc == ISPH_SUCCESS && n > 0) {
    launch_random_stress_tensor(ctx, P->dim, n, ts.dtype, ts.dkind, ts.dtag, seed, step, dr);
    if (!on_device && hipMemcpyAsync(rs_out, dr, sizeof(double) * 6 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
      rc = fail("copy failed", __FILE__, __LINE__);
    rc = st_sync(ctx, rc, "random-stress tensor kernel failed");
  }
  return rc;
}

inline int random_stress_force(isph_ctx *ctx, const isph_particles *P, double dt, double kBT, const double *nu,
                               const double *rho, const double *rs, double *f_inout, int on_device) {
  ISPH_REQUIRE(!on_device || rs_aligned(rs), "rs must be 16-byte aligned device memory");
  OpStage st;
  int rc = op_stage(ctx, P, /*antisym=*/1, on_device, st);
  const int n = P->nlocal;
  DevTmp<double> tnu, trho, trs;
  InOut fio;
  const double *dnu = nullptr, *drho = nullptr, *drs = nullptr;
  if (rc == ISPH_SUCCESS) rc = stage(ctx, nu, (size_t)n, on_device, tnu, &dnu);
  if (rc == ISPH_SUCCESS) rc = stage(ctx, rho, (size_t)n, on_device, trho, &drho);
  if (rc == ISPH_SUCCESS) rc = stage(ctx, rs, (size_t)P->nall * 6, on_device, trs, &drs);
  if (rc == ISPH_SUCCESS) rc = fio.open(ctx, f_inout, (size_t)n * 3, on_device);
  if (rc == ISPH_SUCCESS && n > 0) {
    launch_random_stress_force(ctx, st, dt, kBT, dnu, drho, drs, nullptr, nullptr, 0, fio.dev);
    if (fio.close(ctx) != ISPH_SUCCESS) rc = ISPH_FAILURE;
    rc = st_sync(ctx, rc, "random-stress force kernel failed");
  }
  fio.buf.release();
  st.release();
  return rc;
}

}  // namespace isph

extern "C" {

void isph_ek_params_default(isph_ek_params *p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->ezcb = 0.0; p->psiref = 1.0; p->gamma = 0.0;  // pair_isph.cpp:1684-1698
}

int isph_smooth_field(isph_ctx *ctx, const isph_particles *P, const double *f, int use_filter, int filt_i, int filt_j,
                      double *sf_out, int on_device) {
  ISPH_REQUIRE(ctx && P && f && sf_out, "NULL argument");
  return isph::smooth_field(ctx, P, f, use_filter, filt_i, filt_j, sf_out, on_device);
}

int isph_electrostatic_force(isph_ctx *ctx, const isph_particles *P, int antisym, const isph_ek_params *prm, const double *psi,
                             const double *phi, double *psigrad_out, double *phigrad_out, double *f_inout, int on_device) {
  ISPH_REQUIRE(ctx && P && prm && psi, "NULL argument");
  ISPH_REQUIRE(antisym || P->Gc, "the Symmetric gradient needs Gc (isph_compute_corrections)");
  ISPH_REQUIRE(!P->morris_holmes || P->pnd, "the MorrisHolmes mirror needs pnd (isph_compute_pnd + forward comm)");
  return isph::electrostatic_force(ctx, P, antisym, prm, psi, phi, psigrad_out, phigrad_out, f_inout, on_device);
}

int isph_random_stress_tensor(isph_ctx *ctx, const isph_particles *P, const int *tag, unsigned long long seed,
                              unsigned long long step, double *rs_out, int on_device) {
  ISPH_REQUIRE(ctx && P && tag && rs_out, "NULL argument");
  return isph::random_stress_tensor(ctx, P, tag, seed, step, rs_out, on_device);
}

int isph_random_stress_force(isph_ctx *ctx, const isph_particles *P, double dt, double kBT, const double *nu, const double *rho,
                             const double *rs, double *f_inout, int on_device) {
  ISPH_REQUIRE(ctx && P && nu && rho && rs && f_inout, "NULL argument");
  ISPH_REQUIRE(dt > 0.0, "dt must be positive");
  return isph::random_stress_force(ctx, P, dt, kBT, nu, rho, rs, f_inout, on_device);
}

int isph_force_from_random_stress(isph_ctx *ctx, const isph_particles *P, const isph_halo_plan *plan, const int *tag,
                                  unsigned long long seed, unsigned long long step, double dt, double kBT, const double *nu,
                                  const double *rho, double *f_inout, double *rs_out, int on_device) {
  using namespace isph;
  ISPH_REQUIRE(ctx && P && tag && nu && rho && f_inout, "NULL argument");
  ISPH_REQUIRE(dt > 0.0, "dt must be positive");
  ISPH_REQUIRE(P->colmap, "colmap is required (ghost tensors are read through it)");
  ISPH_REQUIRE(!plan || plan->nlocal == P->nlocal, "halo plan was made for another nlocal");
  ISPH_REQUIRE(!on_device || !rs_out || rs_aligned(rs_out), "rs_out must be 16-byte aligned device memory");
  const int n = P->nlocal, n1 = n > 0 ? n : 1;
  const int nghost = plan ? plan->H.nrecv : 0;
  if (!on_device)
    for (int j = 0; j < P->nall; ++j)
      ISPH_REQUIRE(P->colmap[j] >= 0 && P->colmap[j] < n + nghost, "colmap entry outside the owned particles and the plan's ghosts");
  OpStage st;
  DevTmp<int> ttag;
  DevTmp<double> tnu, trho, tr, tgh;
  InOut fio;
  const int *dtag = nullptr, *dcol = nullptr;
  const double *dnu = nullptr, *drho = nullptr;
  int rc = op_stage(ctx, P, /*antisym=*/1, on_device, st);
  if (rc == ISPH_SUCCESS) rc = stage(ctx, P->colmap, (size_t)P->nall, on_device, st.S.colmap, &dcol);
  if (rc == ISPH_SUCCESS) rc = stage(ctx, tag, (size_t)n, on_device, ttag, &dtag);
  if (rc == ISPH_SUCCESS) rc = stage(ctx, nu, (size_t)n, on_device, tnu, &dnu);
  if (rc == ISPH_SUCCESS) rc = stage(ctx, rho, (size_t)n, on_device, trho, &drho);
  double *dr = (on_device && rs_out) ? rs_out : nullptr;
  if (rc == ISPH_SUCCESS && !dr) { rc = tr.reserve((size_t)n1 * 6); dr = tr.p; }
  if (rc == ISPH_SUCCESS && nghost > 0) rc = tgh.reserve((size_t)nghost * 6);
  if (rc == ISPH_SUCCESS) rc = fio.open(ctx, f_inout, (size_t)n * 3, on_device);
  if (rc == ISPH_SUCCESS && n > 0) launch_random_stress_tensor(ctx, P->dim, n, st.a.type, st.T.kind, dtag, seed, step, dr);
  // every rank takes part in the exchange, also one without particles
  if (rc == ISPH_SUCCESS && plan) rc = isph_halo_forward(ctx, plan, dr, tgh.p, 6, /*on_device=*/1);
  if (rc == ISPH_SUCCESS && n > 0) {
    launch_random_stress_force(ctx, st, dt, kBT, dnu, drho, dr, dcol, nghost > 0 ? tgh.p : nullptr, nghost, fio.dev);
    if (fio.close(ctx) != ISPH_SUCCESS) rc = ISPH_FAILURE;
    if (!on_device && rs_out &&
        hipMemcpyAsync(rs_out, dr, sizeof(double) * 6 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
      rc = fail("copy failed", __FILE__, __LINE__);
  }
  rc = st_sync(ctx, rc, "random-stress kernels failed");
  fio.buf.release();
  st.release();
  return rc;
}

}  // extern "C"
