// surface_tension.hpp -- the producers of the body force `force` for two-phase flow, and the wall normals the
// contact-angle correction reads.  Included at the end of isph_capi.hip.
//
// Replaces
//   PairISPH_Corrected::computeNormals (Solid walls, no use_part)        (ref: pair_isph_corrected.cpp:374-425)
//     Corrected::FunctorOuterNormal                                      (ref: functor_normal.h:57-133)   -> k_normals, assemble.hpp
//   PairISPH_Corrected::computeSurfaceTension_ContinuumSurfaceForce      (ref: pair_isph_corrected.cpp:684-758)
//     Corrected::FunctorOuterPhaseGradient                               (ref: functor_phase_gradient.h:49-141)
//     ColorFunctionCorrected / ColorFunctionAdami                        (ref: color.h:28-66)
//     FunctorOuterNormalizeVector                                        (ref: functor_normalize_vector.h:29-41)
//     Corrected::FunctorOuterCorrectPhaseNormal                          (ref: functor_correct_phase_normal.h:43-95)
//     Corrected::FunctorOuterPhaseDivergence                             (ref: functor_phase_divergence.h:41-98)
//     FunctorOuterContinuumSurfaceForce                                  (ref: functor_continuum_surface_force.h:52-64)
//   PairISPH_Corrected::computeSurfaceTension_PairwiseForce              (ref: pair_isph_corrected.cpp:760-784)
//     FunctorOuterPairwiseForce                                          (ref: functor_pairwise_force.h:31-83)
//     PairwiseForceFunction_*                                            (ref: pairwise_force.h:38-118)
//
// The continuum surface force is five functors and three forward comms in the reference.  Normalising the phase
// gradient and bending it to the contact angle are pointwise on owned particles, so they are the epilogue of the lane
// that summed the gradient, and the chain is TWO neighbour sweeps with ONE ghost fill between them.  Sweep 1 leaves
// {n_x, n_y, n_z, |grad c|} as one 32-byte record per particle: sweep 2 gathers the neighbour's normal and magnitude
// with one access (the magnitude decides whether the neighbour takes part at all, so it comes first in time but
// lives in the same sector).  Like the gradient / divergence operators these sweeps work in the caller's particle
// numbering; one lane per particle, the lane-interleaved neighbour list, pair_rsq for every cut test.
#pragma once
#include "operators.hpp"

namespace isph {

struct CsfArgs {
  int color;                      // 0 Corrected, 1 Adami
  double alpha, eps, kappa;
  double sin1, cos1, sin2, cos2;  // contact angle theta for phase 1, pi - theta for the others
  const int *phase;               // [ntypes+1]
  const double *rho, *wall, *pnd; // [nall] or NULL; pair->normal [.][3] or NULL; pair->pnd
};

template <int DIM>
__device__ __forceinline__ void gt_times_r(const double *G, const double rij[3], double gr[3]) {
  gr[0] = gr[1] = gr[2] = 0.0;
  for (int k2 = 0; k2 < DIM; ++k2) {
    double gitmp = 0.0;
    for (int k1 = 0; k1 < DIM; ++k1) gitmp += G[k2 * DIM + k1] * rij[k1];
    gr[k2] = gitmp;
  }
}

// sweep 1: phase gradient, its length, the unit phase normal, the contact-angle correction
template <int DIM>
__global__ __launch_bounds__(kBlock) void k_csf_phase_normal(AsmTables T, OpArgs a, CsfArgs c, double *__restrict__ grad,
                                                             double4 *__restrict__ nmag) {
  const int i = xcd_block() * blockDim.x + threadIdx.x;
  if (i >= a.nlocal) return;
  const int nt1 = T.ntypes + 1, it = a.type[i], ikind = T.kind[it], iphase = c.phase[it];
  double g[3] = {0, 0, 0}, n[3] = {0, 0, 0}, mag = 0.0;
  if (ikind & KIND_FLUID) {
    double G[DIM * DIM];
    for (int k = 0; k < DIM * DIM; ++k) G[k] = a.Gc[(size_t)i * DIM * DIM + k];
    const double vi = a.vfrac[i], irho = c.rho ? c.rho[i] : 1.0;
    double vol_in = vi, vol_out = 0.0;
    for (int jj = 0, je = T.nlen[i]; jj < je; ++jj) {
      const int j = neigh_at(T, i, jj);
      const int jt = a.type[j];
      const double vj = a.vfrac[j];
      bool in_phase = true;
      if ((T.kind[jt] & KIND_FLUID) && c.phase[jt] != iphase) {
        double rij[3];
        const double rsq = pair_rsq(DIM, a.x, i, j, rij);
        if (rsq < T.cutsq[it * nt1 + jt]) {
          const double r = sqrt(rsq) + kEps;
          const double dwdr = kernel_dval(T.kernel, r, T.hinv[it * nt1 + jt], T.kdnorm[it * nt1 + jt]);
          in_phase = false;
          vol_out += vj;
          if (c.color == 0) {  // 1st order consistent corrected gradient, c_ij = 1
            double gr[3];
            gt_times_r<DIM>(G, rij, gr);
            const double vjtmp = dwdr / r * vj;
            for (int k = 0; k < DIM; ++k) g[k] += gr[k] * vjtmp;
          } else {             // Adami: c_ij = rho_i / (rho_i + rho_j), volume-averaged gradient
            const double jrho = c.rho ? c.rho[j] : 1.0;
            const double cij = irho / (irho + jrho);
            const double t = (vi * vi + vj * vj) * cij * dwdr;
            for (int k = 0; k < DIM; ++k) g[k] += t * (rij[k] / r) / vi;
          }
        }
      }
      if (in_phase) vol_in += vj;  // every listed neighbour that is not an out-of-phase one inside the cut (:82-124)
    }
    const double ratio = vol_in / (vol_in + vol_out);
    if (ratio < c.eps || ratio > 1.0 - c.eps) g[0] = g[1] = g[2] = 0.0;
    double s = 0.0;
    for (int k = 0; k < DIM; ++k) s += g[k] * g[k];
    mag = sqrt(s);
    for (int k = 0; k < DIM; ++k) n[k] = mag != 0.0 ? g[k] / mag : g[k];
    if (c.wall) {  // FunctorOuterCorrectPhaseNormal
      double nw[3] = {0, 0, 0}, kk = 0.0, pp = 0.0;
      for (int k = 0; k < DIM; ++k) { nw[k] = c.wall[3 * (size_t)i + k]; kk += nw[k] * nw[k]; pp += n[k] * n[k]; }
      if (kk > 0.5 && pp > 0.5) {
        const double st = iphase == 1 ? c.sin1 : c.sin2, ct = iphase == 1 ? c.cos1 : c.cos2;
        double dot = 0.0, nt[3] = {0, 0, 0}, m2 = 0.0;
        for (int k = 0; k < DIM; ++k) dot += n[k] * nw[k];
        for (int k = 0; k < DIM; ++k) { nt[k] = n[k] - dot * nw[k]; m2 += nt[k] * nt[k]; }
        const double mt = sqrt(m2);
        if (mt != 0.0)
          for (int k = 0; k < DIM; ++k) nt[k] /= mt;
        const double d = 2.0 * (c.pnd[i] * vi - 0.5) - 0.5;
        const double fw = d < 0.0 ? 0.0 : 2.0 * d;
        double m3 = 0.0;
        for (int k = 0; k < DIM; ++k) {
          const double ntl = nt[k] * st + nw[k] * ct;
          n[k] = fw * n[k] + (1.0 - fw) * ntl;
          m3 += n[k] * n[k];
        }
        const double mn = sqrt(m3);
        if (mn != 0.0)
          for (int k = 0; k < DIM; ++k) n[k] /= mn;
      }
    }
  }
  if (grad)
    for (int k = 0; k < 3; ++k) grad[3 * (size_t)i + k] = g[k];
  nmag[i] = make_double4(n[0], n[1], n[2], mag);
}

// the record of list entry j: its own slot when the caller filled the ghosts, else through the column map (an image of
// an owned particle reads the owner's record, an off-rank ghost the halo buffer)
__device__ __forceinline__ double4 csf_record(const double4 *__restrict__ nmag, const int *__restrict__ colmap,
                                              const double4 *__restrict__ ghosts, int nlocal, int nghost, int j) {
  if (!colmap || j < nlocal) return nmag[j];
  const int col = colmap[j];
  if (col < nlocal) return nmag[col];
  if (ghosts && col - nlocal < nghost) return ghosts[col - nlocal];
  return make_double4(0.0, 0.0, 0.0, 0.0);
}

// sweep 2: curvature kappa_i = div n over the active neighbours, f_i -= alpha (1 - exp(-kappa_csf/|kappa_i|)) kappa_i n_i mag_i.
// DEPARTURE from the reference: kappa_i == 0 on an active particle adds nothing (the reference forms
// alpha (1 - exp(+inf)) 0 = NaN there, functor_continuum_surface_force.h:58-62).
template <int DIM>
__global__ __launch_bounds__(kBlock) void k_csf_force(AsmTables T, OpArgs a, CsfArgs c, const double4 *__restrict__ nmag,
                                                      const int *__restrict__ colmap, const double4 *__restrict__ ghosts,
                                                      int nghost, double *__restrict__ f, double *__restrict__ kappa_out) {
  const int i = xcd_block() * blockDim.x + threadIdx.x;
  if (i >= a.nlocal) return;
  const int nt1 = T.ntypes + 1, it = a.type[i], ikind = T.kind[it], iphase = c.phase[it];
  const double4 ri = nmag[i];
  double div = 0.0;
  const bool active = (ikind & KIND_FLUID) && ri.w > kEps;
  if (active) {
    double G[DIM * DIM];
    for (int k = 0; k < DIM * DIM; ++k) G[k] = a.Gc[(size_t)i * DIM * DIM + k];
    const double ni[3] = {ri.x, ri.y, ri.z};
    for (int jj = 0, je = T.nlen[i]; jj < je; ++jj) {
      const int j = neigh_at(T, i, jj);
      const int jt = a.type[j];
      if (!(T.kind[jt] & KIND_FLUID)) continue;
      const double4 rj = csf_record(nmag, colmap, ghosts, a.nlocal, nghost, j);
      if (!(rj.w > kEps)) continue;
      double rij[3];
      const double rsq = pair_rsq(DIM, a.x, i, j, rij);
      if (!(rsq < T.cutsq[it * nt1 + jt])) continue;
      const double r = sqrt(rsq) + kEps;
      const double dwdr = kernel_dval(T.kernel, r, T.hinv[it * nt1 + jt], T.kdnorm[it * nt1 + jt]);
      const double sign = c.phase[jt] == iphase ? 1.0 : -1.0;
      const double nj[3] = {rj.x, rj.y, rj.z};
      const double vjtmp = dwdr / r * a.vfrac[j];
      double gr[3];
      gt_times_r<DIM>(G, rij, gr);
      for (int k = 0; k < DIM; ++k) div += gr[k] * (sign * nj[k] - ni[k]) * vjtmp;
    }
    if (div != 0.0) {
      const double al = c.alpha * (1.0 - exp(-c.kappa / fabs(div)));
      for (int k = 0; k < DIM; ++k) f[3 * (size_t)i + k] -= al * div * ni[k] * ri.w;
    }
  }
  if (kappa_out) kappa_out[i] = div;
}

// PairwiseForceFunction::val(s, r, c) (pairwise_force.h:51-54, 83-86, 114-117); A by dimension (:68-72, :100-104)
template <int DIM>
__device__ __forceinline__ double pairwise_f(int model, double s, double r, double cut) {
  if (model == 0) return r <= cut ? -s * cos(4.71238898038469 / cut * r) : 0.0;
  const double eps = cut / 3.5, eps0 = eps / 2.0;
  const double A = (model == 1 ? 4.0 : 8.0) * (DIM == 3 ? 2.0 : 1.0);
  const double v = s * (-A * exp(-(r * r) / (eps0 * eps0) / 2.0) + exp(-(r * r) / (eps * eps) / 2.0));
  return model == 1 ? v : r * v;
}

// f_i += sum_j -F(s[phase_i][phase_j], r, cut_ij) r_ij / r over (Fluid, Fluid) pairs; the per-particle sums are added
// over the workgroup (wave DPP sum, four waves through LDS) into partial[block][3] for the functor's _f_sum
template <int DIM>
__global__ __launch_bounds__(kBlock) void k_pairwise_force(AsmTables T, OpArgs a, int model, const int *__restrict__ phase,
                                                           const double *__restrict__ s, int nphase, double *__restrict__ f,
                                                           double *__restrict__ partial) {
  __shared__ double red[kBlock / 64][3];
  const int blk = xcd_block();
  const int i = blk * blockDim.x + threadIdx.x;
  double fi[3] = {0, 0, 0};
  if (i < a.nlocal) {
    const int nt1 = T.ntypes + 1, it = a.type[i], ikind = T.kind[it];
    if (ikind & KIND_FLUID) {
      const int iphase = phase[it];
      for (int jj = 0, je = T.nlen[i]; jj < je; ++jj) {
        const int j = neigh_at(T, i, jj);
        const int jt = a.type[j];
        if (!(T.kind[jt] & KIND_FLUID)) continue;
        double rij[3];
        const double rsq = pair_rsq(DIM, a.x, i, j, rij);
        const double cutsq = T.cutsq[it * nt1 + jt];
        if (!(rsq < cutsq)) continue;
        const double r = sqrt(rsq) + kEps;
        const double fv = pairwise_f<DIM>(model, s[iphase * nphase + phase[jt]], r, sqrt(cutsq));
        for (int k = 0; k < DIM; ++k) fi[k] += -fv * rij[k] / r;
      }
      for (int k = 0; k < DIM; ++k) f[3 * (size_t)i + k] += fi[k];
    }
  }
  // every lane of the workgroup arrives here (no early return above)
  const int wave = threadIdx.x >> 6;
  for (int k = 0; k < 3; ++k) {
    const double w = wave_sum(fi[k]);
    if ((threadIdx.x & 63) == 0) red[wave][k] = w;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double t = 0.0;
    for (int w = 0; w < kBlock / 64; ++w) t += red[w][threadIdx.x];
    partial[3 * (size_t)blk + threadIdx.x] = t;
  }
}

// out[k] = sum over blocks of partial[block][k], one wave, fixed order
__global__ __launch_bounds__(64) void k_sum_partials3(int nblocks, const double *__restrict__ partial, double *__restrict__ out) {
  double t[3] = {0, 0, 0};
  for (int b = threadIdx.x; b < nblocks; b += 64)
    for (int k = 0; k < 3; ++k) t[k] += partial[3 * (size_t)b + k];
  for (int k = 0; k < 3; ++k) {
    const double w = wave_sum(t[k]);
    if (threadIdx.x == 0) out[k] = w;
  }
}

inline int st_sync(isph_ctx *ctx, int rc, const char *what) {
  if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipGetLastError() != hipSuccess)
    return rc == ISPH_SUCCESS ? fail(what, __FILE__, __LINE__) : rc;
  return rc;
}

inline int compute_normals(isph_ctx *ctx, const isph_particles *P, double *normal_out, double *pnd_out, int on_device) {
  OpStage st;
  int rc = op_stage(ctx, P, /*antisym=*/0, on_device, st);
  const int n = P->nlocal, n1 = n > 0 ? n : 1;
  DevTmp<double> tn, tp;
  double *dn = normal_out, *dp = pnd_out;
  if (rc == ISPH_SUCCESS && !on_device) {
    rc = tn.reserve((size_t)n1 * 3);
    dn = tn.p;
    if (rc == ISPH_SUCCESS && pnd_out) { rc = tp.reserve((size_t)n1); dp = tp.p; }
  }
  if (rc == ISPH_SUCCESS && n > 0) {
    const dim3 grid(xcd_grid((n + kBlock - 1) / kBlock));
    if (P->dim == 3)
      hipLaunchKernelGGL(k_normals<3>, grid, dim3(kBlock), 0, ctx->stream, st.T, n, st.a.x, st.a.type, st.a.vfrac, st.a.Gc, dn, dp);
    else
      hipLaunchKernelGGL(k_normals<2>, grid, dim3(kBlock), 0, ctx->stream, st.T, n, st.a.x, st.a.type, st.a.vfrac, st.a.Gc, dn, dp);
    if (!on_device) {
      if (hipMemcpyAsync(normal_out, dn, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
          (pnd_out && hipMemcpyAsync(pnd_out, dp, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess))
        rc = fail("copy failed", __FILE__, __LINE__);
    }
    rc = st_sync(ctx, rc, "normals kernel failed");
  }
  st.release();
  return rc;
}

// parameters and the small host tables of the continuum surface force, staged
struct CsfStage {
  CsfArgs c;
  DevTmp<int> phase;
  DevTmp<double> rho, wall, pnd;
};

inline int csf_stage(isph_ctx *ctx, const isph_particles *P, const isph_csf_params *prm, const double *rho,
                     const double *wall_normal, int on_device, CsfStage &cs) {
  ISPH_REQUIRE(prm->color == 0 || prm->color == 1, "csf color must be 0 (Corrected) or 1 (Adami)");
  ISPH_REQUIRE(prm->phase, "csf phase table missing");
  ISPH_REQUIRE(!wall_normal || P->pnd, "the contact-angle correction needs pnd (isph_compute_normals / isph_compute_pnd + forward comm)");
  memset(&cs.c, 0, sizeof(cs.c));
  cs.c.color = prm->color;
  cs.c.alpha = prm->alpha; cs.c.eps = prm->epsilon; cs.c.kappa = prm->kappa;
  const double pi = 3.14159265358979323846;
  cs.c.sin1 = sin(prm->theta); cs.c.cos1 = cos(prm->theta);
  cs.c.sin2 = sin(pi - prm->theta); cs.c.cos2 = cos(pi - prm->theta);
  ISPH_CHECK(stage(ctx, prm->phase, (size_t)P->ntypes + 1, 0, cs.phase, &cs.c.phase));
  ISPH_CHECK(stage(ctx, rho, (size_t)P->nall, on_device, cs.rho, &cs.c.rho));
  ISPH_CHECK(stage(ctx, wall_normal, (size_t)P->nlocal * 3, on_device, cs.wall, &cs.c.wall));
  if (wall_normal) ISPH_CHECK(stage(ctx, P->pnd, (size_t)P->nlocal, on_device, cs.pnd, &cs.c.pnd));
  return ISPH_SUCCESS;
}

inline void launch_csf_phase_normal(isph_ctx *ctx, const OpStage &st, const CsfArgs &c, double *grad, double *nmag) {
  const dim3 grid(xcd_grid((st.a.nlocal + kBlock - 1) / kBlock));
  if (st.T.dim == 3)
    hipLaunchKernelGGL(k_csf_phase_normal<3>, grid, dim3(kBlock), 0, ctx->stream, st.T, st.a, c, grad, reinterpret_cast<double4 *>(nmag));
  else
    hipLaunchKernelGGL(k_csf_phase_normal<2>, grid, dim3(kBlock), 0, ctx->stream, st.T, st.a, c, grad, reinterpret_cast<double4 *>(nmag));
}

inline void launch_csf_force(isph_ctx *ctx, const OpStage &st, const CsfArgs &c, const double *nmag, const int *colmap,
                             const double *ghosts, int nghost, double *f, double *kappa) {
  const dim3 grid(xcd_grid((st.a.nlocal + kBlock - 1) / kBlock));
  if (st.T.dim == 3)
    hipLaunchKernelGGL(k_csf_force<3>, grid, dim3(kBlock), 0, ctx->stream, st.T, st.a, c, reinterpret_cast<const double4 *>(nmag),
                       colmap, reinterpret_cast<const double4 *>(ghosts), nghost, f, kappa);
  else
    hipLaunchKernelGGL(k_csf_force<2>, grid, dim3(kBlock), 0, ctx->stream, st.T, st.a, c, reinterpret_cast<const double4 *>(nmag),
                       colmap, reinterpret_cast<const double4 *>(ghosts), nghost, f, kappa);
}

// the records are read and written as 32-byte vectors
inline bool csf_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 31u) == 0; }

inline int csf_phase_normal(isph_ctx *ctx, const isph_particles *P, const isph_csf_params *prm, const double *rho,
                            const double *wall_normal, double *grad_out, double *nmag_out, int on_device) {
  ISPH_REQUIRE(!on_device || csf_aligned(nmag_out), "nmag_out must be 32-byte aligned device memory");
  OpStage st;
  CsfStage cs;
  int rc = op_stage(ctx, P, /*antisym=*/0, on_device, st);
  if (rc == ISPH_SUCCESS) rc = csf_stage(ctx, P, prm, rho, wall_normal, on_device, cs);
  const int n = P->nlocal, n1 = n > 0 ? n : 1;
  DevTmp<double> tg, tm;
  double *dg = grad_out, *dm = nmag_out;
  if (rc == ISPH_SUCCESS && !on_device) {
    rc = tm.reserve((size_t)n1 * 4);
    dm = tm.p;
    if (rc == ISPH_SUCCESS && grad_out) { rc = tg.reserve((size_t)n1 * 3); dg = tg.p; }
  }
  if (rc == ISPH_SUCCESS && n > 0) {
    launch_csf_phase_normal(ctx, st, cs.c, dg, dm);
    if (!on_device) {
      if (hipMemcpyAsync(nmag_out, dm, sizeof(double) * 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
          (grad_out && hipMemcpyAsync(grad_out, dg, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess))
        rc = fail("copy failed", __FILE__, __LINE__);
    }
    rc = st_sync(ctx, rc, "phase-normal kernel failed");
  }
  st.release();
  return rc;
}

inline int csf_force(isph_ctx *ctx, const isph_particles *P, const isph_csf_params *prm, const double *nmag, double *f_inout,
                     double *kappa_out, int on_device) {
  ISPH_REQUIRE(!on_device || csf_aligned(nmag), "nmag must be 32-byte aligned device memory");
  OpStage st;
  CsfStage cs;
  int rc = op_stage(ctx, P, /*antisym=*/0, on_device, st);
  if (rc == ISPH_SUCCESS) rc = csf_stage(ctx, P, prm, nullptr, nullptr, on_device, cs);
  const int n = P->nlocal, n1 = n > 0 ? n : 1;
  DevTmp<double> tm, tk;
  InOut fio;
  const double *dm = nullptr;
  double *dk = kappa_out;
  if (rc == ISPH_SUCCESS) rc = stage(ctx, nmag, (size_t)P->nall * 4, on_device, tm, &dm);
  if (rc == ISPH_SUCCESS) rc = fio.open(ctx, f_inout, (size_t)n * 3, on_device);
  if (rc == ISPH_SUCCESS && !on_device && kappa_out) { rc = tk.reserve((size_t)n1); dk = tk.p; }
  if (rc == ISPH_SUCCESS && n > 0) {
    launch_csf_force(ctx, st, cs.c, dm, nullptr, nullptr, 0, fio.dev, dk);
    if (fio.close(ctx) != ISPH_SUCCESS) rc = ISPH_FAILURE;
    if (!on_device && kappa_out &&
        hipMemcpyAsync(kappa_out, dk, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
      rc = fail("copy failed", __FILE__, __LINE__);
    rc = st_sync(ctx, rc, "surface-force kernel failed");
  }
  fio.buf.release();
  st.release();
  return rc;
}

}  // namespace isph

extern "C" {

void isph_csf_params_default(isph_csf_params *p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->color = 0;
  p->alpha = 1.0; p->theta = 0.0; p->epsilon = 0.01; p->kappa = 100.0;  // pair_isph.cpp:1583-1586
  p->phase = nullptr;
}

int isph_compute_normals(isph_ctx *ctx, const isph_particles *P, double *normal_out, double *pnd_out, int on_device) {
  ISPH_REQUIRE(ctx && P && normal_out, "NULL argument");
  ISPH_REQUIRE(P->Gc, "the wall normals need Gc (isph_compute_corrections)");
  return isph::compute_normals(ctx, P, normal_out, pnd_out, on_device);
}

int isph_csf_phase_normal(isph_ctx *ctx, const isph_particles *P, const isph_csf_params *prm, const double *rho,
                          const double *wall_normal, double *grad_out, double *nmag_out, int on_device) {
  ISPH_REQUIRE(ctx && P && prm && nmag_out, "NULL argument");
  ISPH_REQUIRE(P->Gc, "the continuum surface force needs Gc (isph_compute_corrections)");
  return isph::csf_phase_normal(ctx, P, prm, rho, wall_normal, grad_out, nmag_out, on_device);
}

int isph_csf_force(isph_ctx *ctx, const isph_particles *P, const isph_csf_params *prm, const double *nmag, double *f_inout,
                   double *kappa_out, int on_device) {
  ISPH_REQUIRE(ctx && P && prm && nmag && f_inout, "NULL argument");
  ISPH_REQUIRE(P->Gc, "the continuum surface force needs Gc (isph_compute_corrections)");
  return isph::csf_force(ctx, P, prm, nmag, f_inout, kappa_out, on_device);
}

int isph_surface_tension_csf(isph_ctx *ctx, const isph_particles *P, const isph_csf_params *prm, const isph_halo_plan *plan,
                             const double *rho, const double *wall_normal, double *f_inout, double *nmag_out, int on_device) {
  using namespace isph;
  ISPH_REQUIRE(ctx && P && prm && f_inout, "NULL argument");
  ISPH_REQUIRE(P->Gc, "the continuum surface force needs Gc (isph_compute_corrections)");
  ISPH_REQUIRE(P->colmap, "colmap is required (ghost records are read through it)");
  ISPH_REQUIRE(!plan || plan->nlocal == P->nlocal, "halo plan was made for another nlocal");
  ISPH_REQUIRE(!on_device || !nmag_out || csf_aligned(nmag_out), "nmag_out must be 32-byte aligned device memory");
  const int n = P->nlocal, n1 = n > 0 ? n : 1;
  const int nghost = plan ? plan->H.nrecv : 0;
  if (!on_device)
    for (int j = 0; j < P->nall; ++j)
      ISPH_REQUIRE(P->colmap[j] >= 0 && P->colmap[j] < n + nghost, "colmap entry outside the owned particles and the plan's ghosts");
  OpStage st;
  CsfStage cs;
  int rc = op_stage(ctx, P, /*antisym=*/0, on_device, st);
  if (rc == ISPH_SUCCESS) rc = csf_stage(ctx, P, prm, rho, wall_normal, on_device, cs);
  const int *dcol = nullptr;
  if (rc == ISPH_SUCCESS) rc = stage(ctx, P->colmap, (size_t)P->nall, on_device, st.S.colmap, &dcol);
  DevTmp<double> tm, tgh;
  InOut fio;
  double *dm = (on_device && nmag_out) ? nmag_out : nullptr;
  if (rc == ISPH_SUCCESS && !dm) { rc = tm.reserve((size_t)n1 * 4); dm = tm.p; }
  if (rc == ISPH_SUCCESS && nghost > 0) rc = tgh.reserve((size_t)nghost * 4);
  if (rc == ISPH_SUCCESS) rc = fio.open(ctx, f_inout, (size_t)n * 3, on_device);
  if (rc == ISPH_SUCCESS && n > 0) launch_csf_phase_normal(ctx, st, cs.c, nullptr, dm);
  // every rank takes part in the exchange, also one without particles
  if (rc == ISPH_SUCCESS && plan) rc = isph_halo_forward(ctx, plan, dm, tgh.p, 4, /*on_device=*/1);
  if (rc == ISPH_SUCCESS && n > 0) {
    launch_csf_force(ctx, st, cs.c, dm, dcol, nghost > 0 ? tgh.p : nullptr, nghost, fio.dev, nullptr);
    if (fio.close(ctx) != ISPH_SUCCESS) rc = ISPH_FAILURE;
    if (!on_device && nmag_out &&
        hipMemcpyAsync(nmag_out, dm, sizeof(double) * 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
      rc = fail("copy failed", __FILE__, __LINE__);
  }
  rc = st_sync(ctx, rc, "surface-tension kernels failed");
  fio.buf.release();
  st.release();
  return rc;
}

int isph_pairwise_force(isph_ctx *ctx, const isph_particles *P, int model, const int *phase, const double *s, int nphase,
                        double *f_inout, double f_sum[3], int on_device) {
  using namespace isph;
  ISPH_REQUIRE(ctx && P && phase && s && f_inout, "NULL argument");
  ISPH_REQUIRE(model >= 0 && model <= 2, "model must be 0 (TartakovskyMeakin), 1 or 2 (TartakovskyPanchenko Var1 / Var2)");
  ISPH_REQUIRE(nphase >= 1, "nphase must be positive");
  ISPH_REQUIRE(P->x && P->type && (P->neigh_ptr || P->neigh_ptr64) && P->neigh_idx, "particle arrays missing");
  for (int t = 1; t <= P->ntypes; ++t)
    ISPH_REQUIRE(phase[t] >= 0 && phase[t] < nphase, "phase of a type outside [0, nphase)");
  // no volumes and no correction tensor enter: stage as the AntiSymmetric family does, vfrac standing in with x if absent
  isph_particles Q = *P;
  if (!Q.vfrac) Q.vfrac = Q.x;
  OpStage st;
  int rc = op_stage(ctx, &Q, /*antisym=*/1, on_device, st);
  const int n = P->nlocal;
  const int blocks = xcd_grid(((n > 0 ? n : 1) + kBlock - 1) / kBlock);
  DevTmp<int> tph;
  DevTmp<double> ts, tpart, tsum;
  InOut fio;
  const int *dph = nullptr;
  const double *ds = nullptr;
  if (rc == ISPH_SUCCESS) rc = stage(ctx, phase, (size_t)P->ntypes + 1, 0, tph, &dph);
  if (rc == ISPH_SUCCESS) rc = stage(ctx, s, (size_t)nphase * nphase, 0, ts, &ds);
  if (rc == ISPH_SUCCESS) rc = tpart.reserve((size_t)blocks * 3);
  if (rc == ISPH_SUCCESS) rc = tsum.reserve(3);
  if (rc == ISPH_SUCCESS) rc = fio.open(ctx, f_inout, (size_t)n * 3, on_device);
  double hsum[3] = {0, 0, 0};
  if (rc == ISPH_SUCCESS && n > 0) {
    if (P->dim == 3)
      hipLaunchKernelGGL(k_pairwise_force<3>, dim3(blocks), dim3(kBlock), 0, ctx->stream, st.T, st.a, model, dph, ds, nphase, fio.dev, tpart.p);
    else
      hipLaunchKernelGGL(k_pairwise_force<2>, dim3(blocks), dim3(kBlock), 0, ctx->stream, st.T, st.a, model, dph, ds, nphase, fio.dev, tpart.p);
    if (f_sum) {
      hipLaunchKernelGGL(k_sum_partials3, dim3(1), dim3(64), 0, ctx->stream, blocks, (const double *)tpart.p, tsum.p);
      if (hipMemcpyAsync(hsum, tsum.p, sizeof(hsum), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail("copy failed", __FILE__, __LINE__);
    }
    if (fio.close(ctx) != ISPH_SUCCESS) rc = ISPH_FAILURE;
    rc = st_sync(ctx, rc, "pairwise-force kernel failed");
  }
  if (f_sum)
    for (int k = 0; k < 3; ++k) f_sum[k] = hsum[k];
  fio.buf.release();
  st.release();
  return rc;
}

}  // extern "C"
