// ins_step.hpp -- the device-resident time-step driver of incompressible Navier-Stokes (isph_ins_*): one rank's state on
// the device and the phases of PairISPH::compute, FixISPH::final_integrate and FixISPH_Shift::final_integrate chained
// with the entry points of the C ABI.  Nothing is restated here: every neighbour sweep, assembly and solve is the call
// a caller of the ABI would make, with device operands; the glue between them is step_ops.hpp plus the two transposes
// below.  Included by isph_capi.hip.
//
// Two forms.  isph_ins_create: one rank, ghosts are periodic images filled through the owner map.  isph_ins_create_dist:
// one rank's share of a brick of ranks (S->dist); the phases are the same calls, collective, with the list of
// nlist_dist.hpp behind them -- forwards through its plan for the ghost fills, its column map and ncol in the assemblers,
// its plan as the halo of H and A, the *_dist reductions of step_ops.hpp -- and isph_ins_rebuild migrates the state.  A rank
// that fails on its own carries its rc to the next ins_agree, where all ranks leave together.
#pragma once
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "neighbours.hpp"
#include "nlist_dist.hpp"
#include "step_ops.hpp"

struct isph_ins {
  isph_ctx *ctx = nullptr;
  isph_ins_params prm;
  std::vector<int> kind;
  std::vector<double> h, cutsq;
  std::string prec_h, prec_p;
  int nlocal = 0, nall = 0;
  bool has_state = false, has_list = false, pre_done = false, solid_present = false;
  bool moved = false;   // the particles have moved since the list was taken
  long long step = 0;   // steps completed by isph_ins_run
  // [nall][3]
  isph::DevBuf<double> x, v, vstar, f, normal;
  // [nall]
  isph::DevBuf<double> p, dp, rho, nu, vfrac, pnd, work;
  isph::DevBuf<int> type;
  // [nlocal][.]
  isph::DevBuf<double> Gc, Lc, bh, xh, bp, nullvec;
  isph::DevBuf<int> dkind;
  // the list: of the caller (copies) or of isph_ins_rebuild (the isph_nlist itself)
  isph::DevBuf<int> owner_c, nptr_c, nidx_c;
  isph::DevBuf<long long> nptr64_c;
  isph_nlist *nl = nullptr;
  const int *owner = nullptr, *nptr = nullptr, *nidx = nullptr;
  const long long *nptr64 = nullptr;
  long long nnz = 0;
  std::vector<int> null_mask;   // host: !(kind & Solid) of the owned rows, made once per isph_ins_set_state
  long long mask_count = 0;
  // the distributed form (isph_ins_create_dist): this rank's share of the particles; every phase is collective
  bool dist = false;
  isph_decomp dc;
  std::vector<double> faces[3];       // what dc.faces points to
  isph::DevBuf<int> tag;              // [nall] the caller's global id, carried with the particle
  std::vector<int> send_idx_h;        // host copy of the plan's send list (isph_mat_set_halo takes host arrays)
  long long nglobal = 0;              // particles over all ranks
  int last_sent = 0, last_recv = 0;   // of the last rebuild

  void release() {
    x.release(); v.release(); vstar.release(); f.release(); normal.release();
    p.release(); dp.release(); rho.release(); nu.release(); vfrac.release(); pnd.release(); work.release();
    type.release(); Gc.release(); Lc.release(); bh.release(); xh.release(); bp.release(); nullvec.release();
    dkind.release(); owner_c.release(); nptr_c.release(); nidx_c.release(); nptr64_c.release(); tag.release();
    if (nl) { nl->release(); delete nl; nl = nullptr; }
  }
};

namespace isph {

// xh [lda x dim] column-major <- the owned rows of v [.][3]: the initial guess of the Helmholtz solve (pair_isph.cpp:930-933)
__global__ __launch_bounds__(kBlock) void k_ins_rows_to_columns(int n, int dim, int lda, const double *__restrict__ v,
                                                                double *__restrict__ xh) {
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= (long long)n * dim) return;
  const int c = (int)(e / n);
  const long long i = e - (long long)c * n;
  xh[(long long)c * lda + i] = v[3 * i + c];
}

// vstar [nall][3] <- the solution columns, ghost rows from their owners (transpose + forward comm, pair_isph.cpp:974-978);
// components >= dim are 0
__global__ __launch_bounds__(kBlock) void k_ins_columns_to_rows(int nlocal, int nall, int dim, int lda,
                                                                const int *__restrict__ owner, const double *__restrict__ xh,
                                                                double *__restrict__ vstar) {
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= (long long)nall * 3) return;
  const long long i = e / 3;
  const int c = (int)(e - 3 * i);
  int o = (int)i;
  if (i >= nlocal) {
    o = owner[i];
    if (o < 0 || o >= nlocal) return;   // refused when the list was taken (ins_gather_ghosts)
  }
  vstar[e] = c < dim ? xh[(long long)c * lda + o] : 0.0;
}

__global__ __launch_bounds__(kBlock) void k_ins_add(long long n, const double *__restrict__ a, double *__restrict__ y) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) y[i] += a[i];
}

// integer rows of ghosts from their owners (atom->type of a periodic image)
__global__ __launch_bounds__(kBlock) void k_ins_ghost_fill_int(int nlocal, int nall, const int *__restrict__ owner,
                                                               int *__restrict__ a) {
  const long long i = (long long)nlocal + (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nall) return;
  const int o = owner[i];
  if (o < 0 || o >= nlocal) return;   // refused by the checked fill before this one
  a[i] = a[o];
}

// null vector of "sa-amg" on a NullSpace system: the normalised mask
__global__ __launch_bounds__(kBlock) void k_ins_null_vector(int n, int ntypes, const int *__restrict__ type,
                                                            const int *__restrict__ kind, double value, double *__restrict__ out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  out[i] = (kind_of(type, kind, ntypes, i) & kKindSolid) ? 0.0 : value;
}

// ---- the distributed form: kernels ---------------------------------------------------------------------------------------

// the owned rows of vstar [.][3] <- the solution columns; the ghosts follow with the forward comm of the list's plan
__global__ __launch_bounds__(kBlock) void k_ins_columns_to_owned_rows(int nlocal, int dim, int lda, const double *__restrict__ xh,
                                                                      double *__restrict__ vstar) {
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= (long long)nlocal * 3) return;
  const long long i = e / 3;
  const int c = (int)(e - 3 * i);
  vstar[e] = c < dim ? xh[(long long)c * lda + i] : 0.0;
}

// what travels with a particle through isph_migrate: fd [n][6] = v, p, rho, nu and fi [n][2] = type, tag.  One thread per
// double of fd, consecutive lanes on consecutive doubles; the first 2 n threads write fi as well
__global__ __launch_bounds__(kBlock) void k_ins_state_pack(int n, const double *__restrict__ v, const double *__restrict__ p,
                                                           const double *__restrict__ rho, const double *__restrict__ nu,
                                                           const int *__restrict__ type, const int *__restrict__ tag,
                                                           double *__restrict__ fd, int *__restrict__ fi) {
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= (long long)n * 6) return;
  const long long i = e / 6;
  const int c = (int)(e - 6 * i);
  fd[e] = c < 3 ? v[3 * i + c] : c == 3 ? p[i] : c == 4 ? rho[i] : nu[i];
  if (e < (long long)n * 2) fi[e] = (e & 1) ? tag[e >> 1] : type[e >> 1];
}

__global__ __launch_bounds__(kBlock) void k_ins_state_unpack(int n, const double *__restrict__ fd, const int *__restrict__ fi,
                                                             double *__restrict__ v, double *__restrict__ p,
                                                             double *__restrict__ rho, double *__restrict__ nu,
                                                             int *__restrict__ type, int *__restrict__ tag) {
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= (long long)n * 6) return;
  const long long i = e / 6;
  const int c = (int)(e - 6 * i);
  const double a = fd[e];
  if (c < 3) v[3 * i + c] = a;
  else if (c == 3) p[i] = a;
  else if (c == 4) rho[i] = a;
  else nu[i] = a;
  if (e < (long long)n * 2) {
    if (e & 1) tag[e >> 1] = fi[e];
    else type[e >> 1] = fi[e];
  }
}

// more than one rank behind the state: the phases talk to peers
inline bool ins_many(const isph_ins *S) { return S->dist && comm_active(S->ctx) && S->ctx->nranks > 1; }

// a rank that failed on its own carries its rc here; all ranks leave together (comm_consensus)
inline int ins_agree(isph_ins *S, const char *who, int rc) {
  (void)comm_consensus(S->ctx, ins_many(S), who, "isph_ins: the consensus all-reduce failed", nullptr, 0, rc);
  return rc;
}

inline int ins_ncol(const isph_ins *S) { return (S->dist && S->nl) ? S->nl->ncol : S->nlocal; }
inline int ins_rank0(const isph_ins *S) { return !S->dist || step_rank(S->ctx) == 0; }

// the halo of a matrix the driver assembled: the list's plan (what the caller of isph_nlist_build_dist passes on)
inline int ins_set_halo(isph_ins *S, isph_mat *A) {
  if (!S->dist || !S->nl || S->nl->halo.npeers == 0) return ISPH_SUCCESS;
  const isph_halo &H = S->nl->halo;
  return isph_mat_set_halo(S->ctx, A, H.npeers, H.peer.data(), H.send_ptr.data(), S->send_idx_h.data(), H.recv_ptr.data());
}

// grows b to `count` elements and keeps its first `keep`
template <class T>
inline int ins_resize(isph_ctx *ctx, DevBuf<T> &b, size_t count, size_t keep) {
  if (count <= b.cap && b.p) return ISPH_SUCCESS;
  DevBuf<T> nb;
  ISPH_CHECK(nb.reserve(count > 0 ? count : 1));
  if (keep > b.cap) keep = b.cap;
  if (keep > 0 && b.p) {
    if (hipMemcpyAsync(nb.p, b.p, sizeof(T) * keep, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
      nb.release();
      return fail("copy failed", __FILE__, __LINE__);
    }
  }
  b.release();   // parked by the pool until the device has been synchronised: the copy above still reads it
  b = nb;
  return ISPH_SUCCESS;
}

template <class T>
inline int ins_copy_in(isph_ctx *ctx, T *dst, const T *src, size_t count, int on_device) {
  if (count == 0) return ISPH_SUCCESS;
  ISPH_REQUIRE(on_device || !is_device_pointer(src), "device pointer passed with on_device = 0");
  ISPH_CHECK_HIP(hipMemcpyAsync(dst, src, sizeof(T) * count, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  return ISPH_SUCCESS;
}

// the owner map was validated when the list was taken (ins_gather_ghosts): the fills of a step read nothing back
// the distributed form: the forward comm through the list's plan, one exchange
inline int ins_fill(isph_ins *S, int ncomp, double *a, bool check = false) {
  if (S->dist) return nlist_forward<double>(S->ctx, S->nl, ncomp, a, 1);
  return ghost_fill_device(S->ctx, S->nlocal, S->nall, S->owner, ncomp, a, check);
}

// every [nall] array sized for the current ghosts, owned rows kept
inline int ins_size_all(isph_ins *S, bool keep_owned) {
  isph_ctx *ctx = S->ctx;
  const size_t na = (size_t)S->nall, nl = keep_owned ? (size_t)S->nlocal : 0;
  ISPH_CHECK(ins_resize(ctx, S->x, 3 * na, 3 * nl));
  ISPH_CHECK(ins_resize(ctx, S->v, 3 * na, 3 * nl));
  ISPH_CHECK(ins_resize(ctx, S->vstar, 3 * na, 3 * nl));
  ISPH_CHECK(ins_resize(ctx, S->f, 3 * na, 0));
  ISPH_CHECK(ins_resize(ctx, S->normal, 3 * na, 0));
  ISPH_CHECK(ins_resize(ctx, S->p, na, nl));
  ISPH_CHECK(ins_resize(ctx, S->dp, na, nl));
  ISPH_CHECK(ins_resize(ctx, S->rho, na, nl));
  ISPH_CHECK(ins_resize(ctx, S->nu, na, nl));
  ISPH_CHECK(ins_resize(ctx, S->vfrac, na, 0));
  ISPH_CHECK(ins_resize(ctx, S->pnd, na, 0));
  ISPH_CHECK(ins_resize(ctx, S->work, na, 0));
  ISPH_CHECK(ins_resize(ctx, S->type, na, nl));
  if (S->dist) ISPH_CHECK(ins_resize(ctx, S->tag, na, nl));
  return ISPH_SUCCESS;
}

// v, p, rho, nu, type of the ghosts through the owner map (their positions come with the list)
inline int ins_gather_ghosts(isph_ins *S) {
  isph_ctx *ctx = S->ctx;
  if (S->nall == S->nlocal) return ISPH_SUCCESS;
  ISPH_CHECK(ins_fill(S, 3, S->v.p, /*check=*/true));
  ISPH_CHECK(ins_fill(S, 1, S->p.p));
  ISPH_CHECK(ins_fill(S, 1, S->rho.p));
  ISPH_CHECK(ins_fill(S, 1, S->nu.p));
  hipLaunchKernelGGL(k_ins_ghost_fill_int, dim3((S->nall - S->nlocal + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream,
                     S->nlocal, S->nall, S->owner, S->type.p);
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

inline void ins_drop_list(isph_ins *S) {
  (void)isph_ctx_hold_neighbours(S->ctx, 0);
  if (S->nl) { S->nl->release(); delete S->nl; S->nl = nullptr; }
  S->has_list = false;
  S->pre_done = false;
  S->owner = S->nptr = S->nidx = nullptr;
  S->nptr64 = nullptr;
}

// the isph_particles of the state; with_pre: the products of isph_ins_pre as well
inline void ins_view(const isph_ins *S, bool with_pre, isph_particles *P) {
  memset(P, 0, sizeof(*P));
  const isph_ins_params &q = S->prm;
  P->dim = q.dim; P->nlocal = S->nlocal; P->nall = S->nall; P->ntypes = q.ntypes; P->kernel = q.kernel;
  P->x = S->x.p; P->type = S->type.p;
  P->kind = S->kind.data(); P->h = S->h.data(); P->cutsq = S->cutsq.data();
  P->neigh_ptr = S->nptr; P->neigh_ptr64 = S->nptr ? nullptr : S->nptr64; P->neigh_idx = S->nidx;
  P->colmap = S->owner;   // one rank, periodic images: the matrix column of a ghost is its owner's row
  if (S->dist && S->nl) P->colmap = S->nl->colmap.p;   // a brick of ranks: the list's column map
  P->morris_safe_coeff = 0.43301;
  P->solid_normal_diag = 1.0;   // the scalar Helmholtz pass of the same step has run (isph_particles)
  if (with_pre) {
    P->vfrac = S->vfrac.p;
    if (!q.antisym) { P->Gc = S->Gc.p; P->Lc = S->Lc.p; }
    if (S->solid_present && !q.antisym) P->normal = S->normal.p;
  }
}

inline int ins_make_prec(isph_ins *S, const isph_mat *A, const std::string &type, int block, bool nullspace, isph_prec **M) {
  isph_ctx *ctx = S->ctx;
  const bool poly = isph_prec_type_kind(type.c_str()) == 7;   // "gmres-poly<d>"
  if ((type == "sa-amg" || poly) && nullspace) {
    isph_amg_params ap;
    isph_amg_params_default(&ap);
    const int n = S->nlocal;
    ISPH_CHECK(S->nullvec.reserve((size_t)(n > 0 ? n : 1)));
    const double val = S->mask_count > 0 ? 1.0 / std::sqrt((double)S->mask_count) : 0.0;
    if (n > 0)
      hipLaunchKernelGGL(k_ins_null_vector, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, n, S->prm.ntypes,
                         (const int *)S->type.p, (const int *)S->dkind.p, val, S->nullvec.p);
    if (poly) {   // the polynomial of the string's degree, its set-up projected with the driver's null vector
      isph_poly_params pp;
      isph_poly_params_default(&pp);
      pp.degree = atoi(type.c_str() + 10);
      return isph_prec_create_gmres_poly(ctx, A, &pp, S->nullvec.p, 1, M);
    }
    return isph_prec_create_amg(ctx, A, &ap, S->nullvec.p, 1, M);
  }
  return isph_prec_create(ctx, A, type.c_str(), block, M);
}

inline int ins_volumes(isph_ins *S) {
  isph_particles P;
  ins_view(S, false, &P);
  ISPH_CHECK(isph_compute_volumes(S->ctx, &P, S->vfrac.p, 1));
  return ins_fill(S, 1, S->vfrac.p);
}

inline int ins_corrections(isph_ins *S) {
  if (S->prm.antisym) return ISPH_SUCCESS;
  isph_particles P;
  ins_view(S, false, &P);
  P.vfrac = S->vfrac.p;
  const int d = S->prm.dim;
  ISPH_CHECK(S->Gc.reserve((size_t)std::max(S->nlocal, 1) * d * d));
  ISPH_CHECK(S->Lc.reserve((size_t)std::max(S->nlocal, 1) * (d * (d + 1) / 2)));
  return isph_compute_corrections(S->ctx, &P, S->Gc.p, S->Lc.p, 1);
}

}  // namespace isph

extern "C" {

void isph_ins_params_default(isph_ins_params *p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->dim = 3;
  p->kernel = 0;
  p->antisym = 1;              /* pair_isph.cpp:1779 */
  p->theta = 0.5;
  p->dt = 0.0;
  p->incremental_pressure = 1;
  p->singular_mode = 1;        /* NullSpace */
  p->prec_helmholtz = "bjacobi-ilu0";
  p->prec_poisson = "bjacobi-ilu0";
  p->helmholtz_block_size = 512;
  p->poisson_block_size = 512;
  isph_solver_params_default(&p->solver);
  p->shiftcut = 0.0;
  p->nonfluidweight = 0.1;
  p->tgv_umax = 0.1;
  p->status_type_mask = -1;
}

// the refusals and the copies isph_ins_create and isph_ins_create_dist share
static int ins_create_checked(isph_ctx *ctx, const isph_ins_params *prm, isph_ins **out) {
  using namespace isph;
  ISPH_REQUIRE(!prm->block_helmholtz, "isph_ins_create: block Helmholtz is not supported by the driver");
  ISPH_REQUIRE(!prm->morris_holmes, "isph_ins_create: the MorrisHolmes boundary is not supported by the driver");
  ISPH_REQUIRE(!prm->normals_bd_coord && !prm->normals_use_part,
               "isph_ins_create: bd_coord and use_part normals are not supported by the driver");
  ISPH_REQUIRE(!prm->recycle, "isph_ins_create: a recycle handle is not supported by the driver");
  ISPH_REQUIRE(!ctx->pattern_hold, "isph_ins_create: the hold-pattern mode of the context is not supported by the driver");
  ISPH_REQUIRE(prm->dim == 2 || prm->dim == 3, "isph_ins_create: dim must be 2 or 3");
  ISPH_REQUIRE(prm->kernel >= 0 && prm->kernel <= 2, "isph_ins_create: kernel must be 0, 1 or 2");
  ISPH_REQUIRE(prm->dt > 0.0, "isph_ins_create: dt must be positive");
  ISPH_REQUIRE(prm->singular_mode >= 0 && prm->singular_mode <= 3, "isph_ins_create: singular_mode must be 0..3");
  ISPH_REQUIRE(prm->ntypes >= 1 && prm->kind && prm->h && prm->cutsq, "isph_ins_create: the tables kind, h, cutsq are needed");
  ISPH_REQUIRE(prm->prec_helmholtz && prm->prec_poisson, "isph_ins_create: preconditioner names are needed");
  ISPH_REQUIRE(prm->shift >= 0.0 && (prm->shift == 0.0 || prm->shiftcut > 0.0), "isph_ins_create: shift needs shiftcut > 0");
  isph_ins *S = new isph_ins();
  S->ctx = ctx;
  S->prm = *prm;
  const size_t nt = (size_t)prm->ntypes + 1;
  S->kind.assign(prm->kind, prm->kind + nt);
  S->h.assign(prm->h, prm->h + nt * nt);
  S->cutsq.assign(prm->cutsq, prm->cutsq + nt * nt);
  S->prec_h = prm->prec_helmholtz;
  S->prec_p = prm->prec_poisson;
  S->prm.kind = nullptr; S->prm.h = nullptr; S->prm.cutsq = nullptr;
  S->prm.prec_helmholtz = nullptr; S->prm.prec_poisson = nullptr;
  int rc = S->dkind.reserve(nt);
  if (rc == ISPH_SUCCESS && hipMemcpyAsync(S->dkind.p, S->kind.data(), sizeof(int) * nt, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    rc = fail("copy failed", __FILE__, __LINE__);
  if (rc == ISPH_SUCCESS && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail("copy failed", __FILE__, __LINE__);
  if (rc != ISPH_SUCCESS) { S->release(); delete S; return rc; }
  *out = S;
  return ISPH_SUCCESS;
}

int isph_ins_create(isph_ctx *ctx, const isph_ins_params *prm, isph_ins **out) {
  using namespace isph;
  ISPH_REQUIRE(ctx && prm && out, "NULL argument");
  ISPH_CHECK(step_one_rank(ctx, "isph_ins_create: a context with a communicator is not supported (one rank only; "
                                "isph_ins_create_dist takes a brick of ranks)"));
  return ins_create_checked(ctx, prm, out);
}

int isph_ins_create_dist(isph_ctx *ctx, const isph_ins_params *prm, const isph_decomp *dc, isph_ins **out) {
  using namespace isph;
  ISPH_REQUIRE(ctx && prm && dc && out, "NULL argument");
  ISPH_REQUIRE(prm->cut > 0.0, "isph_ins_create_dist: cut of isph_ins_params must be positive (the radius of the neighbour list)");
  ISPH_REQUIRE(dc->dim == prm->dim, "isph_ins_create_dist: dim of the decomposition differs from dim of isph_ins_params");
  DdHost D;   // the checks of the decomposition: the grid against the rank count, the sub-boxes against the cut
  ISPH_CHECK(dd_setup(ctx, dc, prm->cut, true, D));
  bool box_set = false;
  for (int a = 0; a < prm->dim; ++a) box_set = box_set || prm->hi[a] != prm->lo[a] || prm->periodic[a] != 0;
  for (int a = 0; box_set && a < prm->dim; ++a)
    ISPH_REQUIRE(prm->lo[a] == dc->lo[a] && prm->hi[a] == dc->hi[a] && (prm->periodic[a] != 0) == (dc->periodic[a] != 0),
                 "isph_ins_create_dist: lo / hi / periodic of isph_ins_params contradict the decomposition");
  isph_ins *S = nullptr;
  ISPH_CHECK(ins_create_checked(ctx, prm, &S));
  S->dist = true;
  S->dc = *dc;
  for (int a = 0; a < 3; ++a) {
    S->dc.faces[a] = nullptr;
    if (a < dc->dim && dc->faces[a]) {
      S->faces[a].assign(dc->faces[a], dc->faces[a] + dc->pgrid[a] + 1);
      S->dc.faces[a] = S->faces[a].data();
    }
  }
  *out = S;
  return ISPH_SUCCESS;
}

void isph_ins_destroy(isph_ins *S) {
  if (!S) return;
  isph::ins_drop_list(S);
  S->release();
  delete S;
}

int isph_ins_set_state(isph_ins *S, int nlocal, const double *x, const double *v, const double *p, const int *type,
                       const double *rho, const double *nu, int on_device) {
  using namespace isph;
  ISPH_REQUIRE(S && x && v && p && type && rho && nu, "NULL argument");
  ISPH_REQUIRE(!S->dist, "isph_ins_set_state: a distributed state takes isph_ins_set_state_dist (the particles carry a tag)");
  ISPH_REQUIRE(nlocal >= 0 && nlocal <= INT_MAX / 8, "isph_ins_set_state: nlocal out of range");
  isph_ctx *ctx = S->ctx;
  ins_drop_list(S);
  S->has_state = false;
  S->nlocal = S->nall = nlocal;
  const size_t n = (size_t)nlocal;
  ISPH_CHECK(ins_size_all(S, false));
  ISPH_CHECK(ins_copy_in(ctx, S->x.p, x, 3 * n, on_device));
  ISPH_CHECK(ins_copy_in(ctx, S->v.p, v, 3 * n, on_device));
  ISPH_CHECK(ins_copy_in(ctx, S->p.p, p, n, on_device));
  ISPH_CHECK(ins_copy_in(ctx, S->type.p, type, n, on_device));
  ISPH_CHECK(ins_copy_in(ctx, S->rho.p, rho, n, on_device));
  ISPH_CHECK(ins_copy_in(ctx, S->nu.p, nu, n, on_device));
  ISPH_CHECK_HIP(hipMemsetAsync(S->vstar.p, 0, sizeof(double) * 3 * std::max<size_t>(n, 1), ctx->stream));
  ISPH_CHECK_HIP(hipMemsetAsync(S->dp.p, 0, sizeof(double) * std::max<size_t>(n, 1), ctx->stream));
  // the null mask of the Poisson solve is a host array of isph_solve: made here, once
  std::vector<int> htype(n);
  if (on_device) ISPH_CHECK_HIP(hipMemcpyAsync(htype.data(), S->type.p, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  const int *ht = on_device ? htype.data() : type;
  S->null_mask.resize(n);
  S->mask_count = 0;
  S->solid_present = false;
  for (size_t i = 0; i < n; ++i) {
    ISPH_REQUIRE(ht[i] >= 1 && ht[i] <= S->prm.ntypes, "isph_ins_set_state: a type outside [1, ntypes]");
    const int k = S->kind[(size_t)ht[i]];
    S->null_mask[i] = !(k & kKindSolid);
    S->mask_count += S->null_mask[i];
    S->solid_present = S->solid_present || k == kKindSolid;
  }
  ISPH_REQUIRE(!S->solid_present || !S->prm.antisym,
               "isph_ins_set_state: Solid particles need the corrected family (antisym = 0): the wall normals read Gc");
  S->has_state = true;
  S->step = 0;
  return ISPH_SUCCESS;
}

int isph_ins_set_state_dist(isph_ins *S, int nlocal, const double *x, const double *v, const double *p, const int *type,
                            const double *rho, const double *nu, const int *tag, int on_device) {
  using namespace isph;
  ISPH_REQUIRE(S, "NULL argument");
  ISPH_REQUIRE(S->dist, "isph_ins_set_state_dist: the state was not made by isph_ins_create_dist");
  isph_ctx *ctx = S->ctx;
  ins_drop_list(S);
  S->has_state = false;
  long long nmask = 0, nsolid = 0;
  auto local = [&]() -> int {
    ISPH_REQUIRE(nlocal >= 0 && nlocal <= INT_MAX / 32, "isph_ins_set_state_dist: nlocal out of range");
    ISPH_REQUIRE(nlocal == 0 || (x && v && p && type && rho && nu && tag), "NULL argument");
    S->nlocal = S->nall = nlocal;
    const size_t n = (size_t)nlocal;
    ISPH_CHECK(ins_size_all(S, false));
    ISPH_CHECK(ins_copy_in(ctx, S->x.p, x, 3 * n, on_device));
    ISPH_CHECK(ins_copy_in(ctx, S->v.p, v, 3 * n, on_device));
    ISPH_CHECK(ins_copy_in(ctx, S->p.p, p, n, on_device));
    ISPH_CHECK(ins_copy_in(ctx, S->type.p, type, n, on_device));
    ISPH_CHECK(ins_copy_in(ctx, S->rho.p, rho, n, on_device));
    ISPH_CHECK(ins_copy_in(ctx, S->nu.p, nu, n, on_device));
    ISPH_CHECK(ins_copy_in(ctx, S->tag.p, tag, n, on_device));
    ISPH_CHECK_HIP(hipMemsetAsync(S->vstar.p, 0, sizeof(double) * 3 * std::max<size_t>(n, 1), ctx->stream));
    ISPH_CHECK_HIP(hipMemsetAsync(S->dp.p, 0, sizeof(double) * std::max<size_t>(n, 1), ctx->stream));
    std::vector<int> htype(n);
    if (on_device && n > 0)
      ISPH_CHECK_HIP(hipMemcpyAsync(htype.data(), S->type.p, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
    ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    const int *ht = on_device ? htype.data() : type;
    S->null_mask.resize(n);
    for (size_t i = 0; i < n; ++i) {
      ISPH_REQUIRE(ht[i] >= 1 && ht[i] <= S->prm.ntypes, "isph_ins_set_state_dist: a type outside [1, ntypes]");
      const int k = S->kind[(size_t)ht[i]];
      S->null_mask[i] = !(k & kKindSolid);
      nmask += S->null_mask[i];
      nsolid += k == kKindSolid;
    }
    return ISPH_SUCCESS;
  };
  int rc = local();
  // ONE sum all-reduce: the non-Solid rows (the value of the SA-AMG null vector), the Solid rows (whether the normals are
  // computed and forwarded is a decision of all ranks), the particles, the failure flag
  double h[4] = {(double)nmask, (double)nsolid, (double)nlocal, rc == ISPH_SUCCESS ? 0.0 : 1.0};
  if (ins_many(S) && comm_host_allreduce(ctx, h, 4, /*sum*/ 0) != ISPH_SUCCESS)
    return fail("isph_ins_set_state_dist: the consensus all-reduce failed", __FILE__, __LINE__);
  if (h[3] != 0.0 && rc == ISPH_SUCCESS) rc = comm_failed_elsewhere("isph_ins_set_state_dist");
  ISPH_CHECK(rc);
  S->mask_count = (long long)h[0];
  S->solid_present = h[1] > 0.0;
  S->nglobal = (long long)h[2];
  ISPH_REQUIRE(!S->solid_present || !S->prm.antisym,
               "isph_ins_set_state_dist: Solid particles need the corrected family (antisym = 0): the wall normals read Gc");
  S->last_sent = S->last_recv = 0;
  S->has_state = true;
  S->step = 0;
  return ISPH_SUCCESS;
}

int isph_ins_set_list(isph_ins *S, int nall, const double *x_all, const int *owner, const int *neigh_ptr,
                      const long long *neigh_ptr64, const int *neigh_idx, int on_device) {
  using namespace isph;
  ISPH_REQUIRE(S && S->has_state, "isph_ins_set_list: no state (isph_ins_set_state comes first)");
  ISPH_REQUIRE(!S->dist, "isph_ins_set_list: a distributed state builds its own list (isph_ins_rebuild): a caller's list has no "
                         "column map and no halo plan");
  ISPH_REQUIRE(x_all && owner && (neigh_ptr || neigh_ptr64) && neigh_idx, "NULL argument");
  ISPH_REQUIRE(nall >= S->nlocal, "isph_ins_set_list: nall < nlocal");
  isph_ctx *ctx = S->ctx;
  ins_drop_list(S);
  const size_t n1 = (size_t)S->nlocal + 1;
  long long nnz = 0;
  if (neigh_ptr64) {
    ISPH_CHECK(S->nptr64_c.reserve(n1));
    ISPH_CHECK(ins_copy_in(ctx, S->nptr64_c.p, neigh_ptr64, n1, on_device));
    ISPH_CHECK_HIP(hipMemcpyAsync(&nnz, S->nptr64_c.p + S->nlocal, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  } else {
    int last = 0;
    ISPH_CHECK(S->nptr_c.reserve(n1));
    ISPH_CHECK(ins_copy_in(ctx, S->nptr_c.p, neigh_ptr, n1, on_device));
    ISPH_CHECK_HIP(hipMemcpyAsync(&last, S->nptr_c.p + S->nlocal, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    nnz = last;
  }
  ISPH_REQUIRE(nnz >= 0, "isph_ins_set_list: negative neighbour count");
  ISPH_CHECK(S->nidx_c.reserve((size_t)std::max<long long>(nnz, 1)));
  ISPH_CHECK(ins_copy_in(ctx, S->nidx_c.p, neigh_idx, (size_t)nnz, on_device));
  ISPH_CHECK(S->owner_c.reserve((size_t)std::max(nall, 1)));
  ISPH_CHECK(ins_copy_in(ctx, S->owner_c.p, owner, (size_t)nall, on_device));
  S->nall = nall;
  ISPH_CHECK(ins_size_all(S, true));
  // the ghosts' positions are the caller's; the owned rows stay those of the state
  ISPH_CHECK(ins_copy_in(ctx, S->x.p + 3 * (size_t)S->nlocal, x_all + 3 * (size_t)S->nlocal, 3 * (size_t)(nall - S->nlocal), on_device));
  S->owner = S->owner_c.p; S->nidx = S->nidx_c.p; S->nnz = nnz;
  S->nptr = neigh_ptr64 ? nullptr : S->nptr_c.p;
  S->nptr64 = neigh_ptr64 ? S->nptr64_c.p : nullptr;
  ISPH_CHECK(ins_gather_ghosts(S));
  S->has_list = true;
  S->moved = false;
  return ISPH_SUCCESS;
}

// LAMMPS between two compute() calls on a brick of ranks: Comm::exchange (isph_migrate with the state as its payload),
// Comm::borders + Neighbor::build (isph_nlist_build_dist, prune on), then the ghosts of the state in ONE forward
static int ins_rebuild_dist(isph_ins *S) {
  using namespace isph;
  isph_ctx *ctx = S->ctx;
  hipStream_t st = ctx->stream;
  const isph_ins_params &q = S->prm;
  const char *who = "isph_ins_rebuild";
  ins_drop_list(S);
  // 1. the payload: [n][6] doubles and [n][2] ints
  const int n0 = S->nlocal;
  DevTmp<double> fd;
  DevTmp<int> fi;
  int rc = fd.reserve((size_t)std::max(n0, 1) * 6);
  if (rc == ISPH_SUCCESS) rc = fi.reserve((size_t)std::max(n0, 1) * 2);
  if (rc == ISPH_SUCCESS && n0 > 0) {
    hipLaunchKernelGGL(k_ins_state_pack, dim3((unsigned)(((long long)n0 * 6 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, n0,
                       (const double *)S->v.p, (const double *)S->p.p, (const double *)S->rho.p, (const double *)S->nu.p,
                       (const int *)S->type.p, (const int *)S->tag.p, fd.p, fi.p);
    if (hipGetLastError() != hipSuccess) rc = fail("pack failed", __FILE__, __LINE__);
  }
  ISPH_CHECK(ins_agree(S, who, rc));
  // 2. migration
  isph_migrated M;
  rc = migrate(ctx, &S->dc, n0, S->x.p, 6, fd.p, 2, fi.p, 1, M);
  if (rc != ISPH_SUCCESS) { M.release(); return rc; }
  // 3. the new owned rows
  const int n = M.nlocal;
  const bool changed = M.nsent != 0 || M.nrecv != 0;
  S->last_sent = M.nsent; S->last_recv = M.nrecv;
  S->nlocal = S->nall = n;
  rc = ins_size_all(S, false);
  if (rc == ISPH_SUCCESS && n > 0) {
    hipLaunchKernelGGL(k_ins_state_unpack, dim3((unsigned)(((long long)n * 6 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, n,
                       (const double *)M.fd.p, (const int *)M.fi.p, S->v.p, S->p.p, S->rho.p, S->nu.p, S->type.p, S->tag.p);
    if (hipGetLastError() != hipSuccess) rc = fail("unpack failed", __FILE__, __LINE__);
  }
  if (rc == ISPH_SUCCESS && hipMemsetAsync(S->vstar.p, 0, sizeof(double) * 3 * (size_t)std::max(n, 1), st) != hipSuccess)
    rc = fail("memset failed", __FILE__, __LINE__);
  rc = ins_agree(S, who, rc);
  if (rc != ISPH_SUCCESS) { M.release(); return rc; }
  // 4. ghosts, list, column map, plan
  isph_nlist *nl = new isph_nlist();
  rc = nlist_build_dist(ctx, &S->dc, n, M.x.p, q.cut, /*prune=*/1, 1, *nl);
  M.release();
  if (rc != ISPH_SUCCESS) { nl->release(); delete nl; return rc; }
  S->nl = nl;
  S->nall = nl->nlocal + nl->nghost;
  S->nnz = nl->nnz;
  rc = ins_size_all(S, true);
  if (rc == ISPH_SUCCESS && S->nall > 0 &&
      hipMemcpyAsync(S->x.p, nl->x.p, sizeof(double) * 3 * (size_t)S->nall, hipMemcpyDeviceToDevice, st) != hipSuccess)
    rc = fail("copy failed", __FILE__, __LINE__);
  // the send list on the host, for isph_mat_set_halo
  S->send_idx_h.assign((size_t)nl->halo.nsend, 0);
  if (rc == ISPH_SUCCESS && nl->halo.nsend > 0 &&
      hipMemcpyAsync(S->send_idx_h.data(), nl->halo.send_idx.p, sizeof(int) * (size_t)nl->halo.nsend, hipMemcpyDeviceToHost, st) != hipSuccess)
    rc = fail("copy failed", __FILE__, __LINE__);
  // 6. the null mask of isph_solve is a host array: remade only when a particle arrived or left
  if (rc == ISPH_SUCCESS && (changed || S->null_mask.size() != (size_t)n)) {
    std::vector<int> ht((size_t)n);
    if (n > 0 && hipMemcpyAsync(ht.data(), S->type.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st) != hipSuccess)
      rc = fail("copy failed", __FILE__, __LINE__);
    if (rc == ISPH_SUCCESS && hipStreamSynchronize(st) != hipSuccess) rc = fail("copy failed", __FILE__, __LINE__);
    S->null_mask.assign((size_t)n, 0);
    for (size_t i = 0; rc == ISPH_SUCCESS && i < (size_t)n; ++i) {
      if (ht[i] < 1 || ht[i] > q.ntypes) { rc = fail("isph_ins_rebuild: a type outside [1, ntypes] arrived", __FILE__, __LINE__); break; }
      S->null_mask[i] = !(S->kind[(size_t)ht[i]] & kKindSolid);
    }
  }
  if (rc == ISPH_SUCCESS && hipStreamSynchronize(st) != hipSuccess) rc = fail("copy failed", __FILE__, __LINE__);
  rc = ins_agree(S, who, rc);
  if (rc != ISPH_SUCCESS) { ins_drop_list(S); return rc; }
  S->owner = nl->owner.p; S->nidx = nl->idx.p;
  S->nptr = nl->fits32 ? nl->ptr32.p : nullptr;
  S->nptr64 = nl->ptr64.p;
  // 5. v, p, rho, nu, type, tag of the ghosts: one exchange
  const isph_fwd_array arr[6] = {{S->v.p, 3, 0}, {S->p.p, 1, 0}, {S->rho.p, 1, 0}, {S->nu.p, 1, 0}, {S->type.p, 1, 1}, {S->tag.p, 1, 1}};
  rc = nlist_forward_multi(ctx, nl, 6, arr, 1, /*agree=*/false);
  if (rc != ISPH_SUCCESS) { ins_drop_list(S); return rc; }
  S->has_list = true;
  S->moved = false;
  return ISPH_SUCCESS;
}

int isph_ins_rebuild(isph_ins *S) {
  using namespace isph;
  ISPH_REQUIRE(S && S->has_state, "isph_ins_rebuild: no state (isph_ins_set_state comes first)");
  if (S->dist) return ins_rebuild_dist(S);
  isph_ctx *ctx = S->ctx;
  const isph_ins_params &q = S->prm;
  ISPH_REQUIRE(q.cut > 0.0, "isph_ins_rebuild: the box and the list cut of isph_ins_params are needed");
  ins_drop_list(S);
  isph_nlist *nl = nullptr;
  ISPH_CHECK(isph_nlist_build(ctx, q.dim, S->nlocal, S->x.p, q.lo, q.hi, q.periodic, q.cut, /*wrap=*/1, 1, &nl));
  S->nl = nl;
  S->nall = nl->nlocal + nl->nghost;
  S->nnz = nl->nnz;
  int rc = ins_size_all(S, true);
  // owned positions wrapped into the box, the images behind them: device to device
  if (rc == ISPH_SUCCESS && S->nall > 0 &&
      hipMemcpyAsync(S->x.p, nl->x.p, sizeof(double) * 3 * (size_t)S->nall, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
    rc = fail("copy failed", __FILE__, __LINE__);
  if (rc != ISPH_SUCCESS) { ins_drop_list(S); return rc; }
  S->owner = nl->owner.p; S->nidx = nl->idx.p;
  S->nptr = nl->fits32 ? nl->ptr32.p : nullptr;
  S->nptr64 = nl->ptr64.p;
  rc = ins_gather_ghosts(S);
  if (rc != ISPH_SUCCESS) { ins_drop_list(S); return rc; }
  S->has_list = true;
  S->moved = false;
  return ISPH_SUCCESS;
}

int isph_ins_sizes(const isph_ins *S, long long info[6]) {
  ISPH_REQUIRE(S && info, "NULL argument");
  info[0] = S->nlocal; info[1] = S->nall; info[2] = S->has_list ? S->nnz : -1; info[3] = S->step;
  info[4] = S->pre_done; info[5] = S->solid_present;
  return ISPH_SUCCESS;
}

int isph_ins_sizes_dist(const isph_ins *S, long long info[10]) {
  ISPH_REQUIRE(S && info, "NULL argument");
  ISPH_REQUIRE(S->dist, "isph_ins_sizes_dist: the state was not made by isph_ins_create_dist");
  const isph_nlist *nl = S->has_list ? S->nl : nullptr;
  info[0] = S->nlocal; info[1] = S->nall; info[2] = nl ? S->nnz : -1; info[3] = S->step;
  info[4] = nl ? nl->ncol : S->nlocal; info[5] = nl ? nl->halo.npeers : 0; info[6] = nl ? nl->noffrank : 0;
  info[7] = S->last_sent; info[8] = S->last_recv; info[9] = S->nglobal;
  return ISPH_SUCCESS;
}

int isph_ins_get(isph_ins *S, const char *name, int with_ghosts, void *out, int on_device) {
  using namespace isph;
  ISPH_REQUIRE(S && S->has_state && name && out, "isph_ins_get: NULL argument or no state");
  const std::string f = name;
  const int d = S->prm.dim;
  const void *src = nullptr;
  size_t per = 0, elem = sizeof(double);
  bool owned_only = false;
  if (f == "x") { src = S->x.p; per = 3; }
  else if (f == "v") { src = S->v.p; per = 3; }
  else if (f == "vstar") { src = S->vstar.p; per = 3; }
  else if (f == "f") { src = S->f.p; per = 3; }
  else if (f == "normal") { src = S->normal.p; per = 3; }
  else if (f == "p") { src = S->p.p; per = 1; }
  else if (f == "dp") { src = S->dp.p; per = 1; }
  else if (f == "rho") { src = S->rho.p; per = 1; }
  else if (f == "nu") { src = S->nu.p; per = 1; }
  else if (f == "vfrac") { src = S->vfrac.p; per = 1; }
  else if (f == "pnd") { src = S->pnd.p; per = 1; }
  else if (f == "Gc") { src = S->Gc.p; per = (size_t)d * d; owned_only = true; }
  else if (f == "Lc") { src = S->Lc.p; per = (size_t)d * (d + 1) / 2; owned_only = true; }
  else if (f == "type") { src = S->type.p; per = 1; elem = sizeof(int); }
  else if (f == "owner") { src = S->owner; per = 1; elem = sizeof(int); }
  else if (f == "tag" && S->dist) { src = S->tag.p; per = 1; elem = sizeof(int); }
  else if (f == "owner_rank" && S->dist) { src = S->nl ? S->nl->orank.p : nullptr; per = 1; elem = sizeof(int); }
  else if (f == "colmap" && S->dist) { src = S->nl ? S->nl->colmap.p : nullptr; per = 1; elem = sizeof(int); }
  else return fail("isph_ins_get: unknown field (x v vstar f normal p dp rho nu vfrac pnd Gc Lc type owner; a distributed state: "
                   "tag owner_rank colmap)", __FILE__, __LINE__);
  ISPH_REQUIRE(src, "isph_ins_get: the field has not been computed yet");
  ISPH_REQUIRE(!(owned_only && with_ghosts), "isph_ins_get: Gc and Lc hold the owned rows only");
  const size_t rows = with_ghosts ? (size_t)S->nall : (size_t)S->nlocal;
  ISPH_REQUIRE(on_device || !is_device_pointer(out), "on_device = 0 but the output is device memory");
  if (rows > 0)
    ISPH_CHECK_HIP(hipMemcpyAsync(out, src, elem * per * rows, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, S->ctx->stream));
  ISPH_CHECK_HIP(hipStreamSynchronize(S->ctx->stream));
  return ISPH_SUCCESS;
}

int isph_ins_pre(isph_ins *S) {
  using namespace isph;
  ISPH_REQUIRE(S && S->has_state, "isph_ins_pre: no state (isph_ins_set_state comes first)");
  ISPH_REQUIRE(S->has_list, "isph_ins_pre: no neighbour list (isph_ins_set_list or isph_ins_rebuild comes first)");
  isph_ctx *ctx = S->ctx;
  S->pre_done = false;
  ISPH_CHECK(isph_ctx_hold_neighbours(ctx, 1));
  ISPH_CHECK(ins_volumes(S));
  ISPH_CHECK(ins_corrections(S));
  if (S->solid_present) {
    isph_particles P;
    ins_view(S, false, &P);
    P.vfrac = S->vfrac.p; P.Gc = S->Gc.p; P.Lc = S->Lc.p;
    ISPH_CHECK(isph_compute_normals(ctx, &P, S->normal.p, S->pnd.p, 1));
    if (S->dist) {   // one message of 4 doubles per ghost, the reference's own (pair_isph_corrected.cpp:1352-1377)
      const isph_fwd_array arr[2] = {{S->normal.p, 3, 0}, {S->pnd.p, 1, 0}};
      ISPH_CHECK(nlist_forward_multi(ctx, S->nl, 2, arr, 1, /*agree=*/false));
    } else {
      ISPH_CHECK(ins_fill(S, 3, S->normal.p));
      ISPH_CHECK(ins_fill(S, 1, S->pnd.p));
    }
  }
  ISPH_CHECK_HIP(hipMemsetAsync(S->f.p, 0, sizeof(double) * 3 * (size_t)std::max(S->nall, 1), ctx->stream));
  S->pre_done = true;
  return ISPH_SUCCESS;
}

int isph_ins_view(const isph_ins *S, isph_particles *P) {
  ISPH_REQUIRE(S && P, "NULL argument");
  ISPH_REQUIRE(S->pre_done, "isph_ins_view: isph_ins_pre comes first");
  isph::ins_view(S, true, P);
  return ISPH_SUCCESS;
}

double *isph_ins_force(isph_ins *S) { return (S && S->pre_done) ? S->f.p : nullptr; }

int isph_ins_add_force(isph_ins *S, int rows, const double *f, int on_device) {
  using namespace isph;
  ISPH_REQUIRE(S && f, "NULL argument");
  ISPH_REQUIRE(S->pre_done, "isph_ins_add_force: isph_ins_pre comes first");
  ISPH_REQUIRE(rows == S->nlocal || rows == S->nall, "isph_ins_add_force: rows must be nlocal or nall");
  isph_ctx *ctx = S->ctx;
  DevTmp<double> sf;
  const double *df = nullptr;
  const size_t count = 3 * (size_t)rows;
  ISPH_CHECK(stage(ctx, f, count, on_device, sf, &df));
  if (count > 0)
    hipLaunchKernelGGL(k_ins_add, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, (long long)count, df,
                       S->f.p);
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

int isph_ins_solve(isph_ins *S, isph_ins_info *info) {
  using namespace isph;
  ISPH_REQUIRE(S, "NULL argument");
  ISPH_REQUIRE(S->pre_done, "isph_ins_solve: isph_ins_pre comes first");
  isph_ctx *ctx = S->ctx;
  const isph_ins_params &q = S->prm;
  const int n = S->nlocal, na = S->nall, d = q.dim, n1 = std::max(n, 1);
  isph_ins_info local;
  memset(&local, 0, sizeof(local));
  isph_particles P;
  ins_view(S, true, &P);
  // ---- Helmholtz (pair_isph.cpp:925-982)
  const double theta = q.theta > 0 ? q.theta : -q.theta;
  const bool rhs_only = theta < 1e-24;
  ISPH_CHECK(S->bh.reserve((size_t)n1 * d));
  ISPH_CHECK(S->xh.reserve((size_t)n1 * d));
  isph_mat *H = nullptr;
  const int ncol = ins_ncol(S);
  {
    int rc = isph_assemble_helmholtz(ctx, &P, q.antisym, q.dt, q.theta, S->nu.p, S->rho.p, S->p.p, S->f.p, q.g,
                                     q.incremental_pressure, S->v.p, ncol, rhs_only ? nullptr : &H, S->bh.p, n, 1);
    if (rc == ISPH_SUCCESS && H) rc = ins_set_halo(S, H);
    rc = ins_agree(S, "isph_ins_solve", rc);   // the assembly is this rank's own; the solve is collective
    if (rc != ISPH_SUCCESS) {
      if (H) isph_mat_destroy(H);
      return rc;
    }
  }
  if (rhs_only) {
    ISPH_CHECK_HIP(hipMemcpyAsync(S->xh.p, S->bh.p, sizeof(double) * (size_t)n * d, hipMemcpyDeviceToDevice, ctx->stream));
    local.helmholtz.converged = 1;
  } else {
    if (n > 0)
      hipLaunchKernelGGL(k_ins_rows_to_columns, dim3(((long long)n * d + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, n, d, n,
                         (const double *)S->v.p, S->xh.p);
    isph_prec *MH = nullptr;
    int rc = ins_make_prec(S, H, S->prec_h, q.helmholtz_block_size, false, &MH);
    if (rc == ISPH_SUCCESS) rc = isph_solve(ctx, H, MH, S->bh.p, S->xh.p, d, n, 0, nullptr, &q.solver, &local.helmholtz, 1);
    isph_prec_destroy(MH);
    isph_mat_destroy(H);
    ISPH_CHECK(rc);
  }
  if (S->dist) {   // owned rows, then the forward of vstar
    if (n > 0)
      hipLaunchKernelGGL(k_ins_columns_to_owned_rows, dim3(((long long)n * 3 + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, n,
                         d, n, (const double *)S->xh.p, S->vstar.p);
    ISPH_CHECK_HIP(hipGetLastError());
    ISPH_CHECK(ins_fill(S, 3, S->vstar.p));
  } else if (na > 0) {
    hipLaunchKernelGGL(k_ins_columns_to_rows, dim3(((long long)na * 3 + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, n, na, d,
                       n, S->owner, (const double *)S->xh.p, S->vstar.p);
  }
  ISPH_CHECK_HIP(hipGetLastError());
  // ---- Poisson (pair_isph.cpp:985-1027)
  ISPH_CHECK(S->bp.reserve((size_t)n1));
  isph_mat *A = nullptr;
  {
    int rc = isph_assemble_poisson(ctx, &P, q.antisym, q.dt, S->rho.p, S->vstar.p, q.singular_mode, ins_rank0(S), ncol, &A, S->bp.p, 1);
    if (rc == ISPH_SUCCESS) rc = ins_set_halo(S, A);
    rc = ins_agree(S, "isph_ins_solve", rc);
    if (rc != ISPH_SUCCESS) {
      if (A) isph_mat_destroy(A);
      return rc;
    }
  }
  {
    const bool nullspace = q.singular_mode == 1;
    isph_prec *M = nullptr;
    int rc = ins_make_prec(S, A, S->prec_p, q.poisson_block_size, nullspace, &M);
    if (rc == ISPH_SUCCESS && hipMemsetAsync(S->dp.p, 0, sizeof(double) * (size_t)n1, ctx->stream) != hipSuccess)
      rc = fail("memset failed", __FILE__, __LINE__);
    if (rc == ISPH_SUCCESS)
      rc = isph_solve(ctx, A, M, S->bp.p, S->dp.p, 1, n, nullspace ? 1 : 0, nullspace ? S->null_mask.data() : nullptr, &q.solver,
                      &local.poisson, 1);
    isph_prec_destroy(M);
    isph_mat_destroy(A);
    ISPH_CHECK(rc);
  }
  ISPH_CHECK(ins_fill(S, 1, S->dp.p));
  if (q.incremental_pressure)
    ISPH_CHECK(S->dist ? zero_mean_dist_device(ctx, n, na, S->type.p, S->dkind.p, q.ntypes, S->dp.p, 1, nullptr)
                       : zero_mean_device(ctx, n, na, S->type.p, S->dkind.p, q.ntypes, S->dp.p, 1, nullptr));
  // ---- corrections (pair_isph.cpp:1030-1031); the ghosts of the corrected velocity follow
  ISPH_CHECK(isph_correct_velocity_pressure(ctx, &P, q.antisym, q.dt, S->rho.p, S->dp.p, S->vstar.p, S->p.p, q.incremental_pressure, 1));
  ISPH_CHECK(ins_fill(S, 3, S->vstar.p));
  if (info) *info = local;
  return ISPH_SUCCESS;
}

int isph_ins_advance(isph_ins *S) {
  using namespace isph;
  ISPH_REQUIRE(S, "NULL argument");
  ISPH_REQUIRE(S->pre_done, "isph_ins_advance: isph_ins_pre comes first");
  isph_ctx *ctx = S->ctx;
  const isph_ins_params &q = S->prm;
  isph_particles P;
  ins_view(S, true, &P);
  ISPH_CHECK(isph_advance_begin(ctx, &P, q.antisym, q.dt, S->p.p, S->v.p, S->vstar.p, S->work.p, 1));
  ISPH_CHECK(ins_fill(S, 1, S->work.p));
  // over the owned particles and the ghosts, like FunctorOuterAdvanceTimeEnd (functor_advance_time_end.h:36-72): a ghost
  // takes its owner's increments, so it moves with its owner
  ISPH_CHECK(isph_advance_end(ctx, S->nall, q.dim, q.dt, S->work.p, S->vstar.p, S->p.p, S->x.p, S->v.p, 1));
  S->pre_done = false;   // the volumes and corrections belong to the positions before the move
  S->moved = true;
  return ISPH_SUCCESS;
}

int isph_ins_shift(isph_ins *S, double *vmax_out) {
  using namespace isph;
  ISPH_REQUIRE(S && S->has_state, "isph_ins_shift: no state");
  ISPH_REQUIRE(S->has_list, "isph_ins_shift: no neighbour list");
  const isph_ins_params &q = S->prm;
  ISPH_REQUIRE(q.shift > 0.0 && q.shiftcut > 0.0, "isph_ins_shift: shift and shiftcut of isph_ins_params must be positive");
  isph_ctx *ctx = S->ctx;
  // computePre on the moved particles with the list of the step (fix_isph_shift.cpp:146-163)
  ISPH_CHECK(ins_volumes(S));
  ISPH_CHECK(ins_corrections(S));
  isph_particles P;
  ins_view(S, true, &P);
  P.normal = nullptr;
  std::vector<int> fixed((size_t)q.ntypes + 1, 0);
  for (int t = 1; t <= q.ntypes; ++t) fixed[(size_t)t] = S->kind[(size_t)t] == kKindSolid;
  double vmax = 0.0;
  ISPH_CHECK(isph_shift_particles(ctx, &P, q.antisym, fixed.data(), q.shift, q.shiftcut, q.nonfluidweight, q.dt, S->x.p, S->v.p,
                                  S->p.p, &vmax, 1));
  if (vmax_out) *vmax_out = vmax;
  S->pre_done = false;
  S->moved = true;
  return ISPH_SUCCESS;
}

int isph_ins_diagnostics(isph_ins *S, double t, double out[12]) {
  using namespace isph;
  ISPH_REQUIRE(S && out, "NULL argument");
  ISPH_REQUIRE(S->pre_done, "isph_ins_diagnostics: isph_ins_pre comes first (the volumes are read)");
  const isph_ins_params &q = S->prm;
  if (S->dist) {
    ISPH_CHECK(tgv_error_dist_device(S->ctx, S->nlocal, S->x.p, S->vstar.p, S->p.p, S->rho.p, S->nu.p, t, q.tgv_umax, out));
    return status_dist_device(S->ctx, S->nlocal, q.status_type_mask, S->x.p, S->type.p, S->vfrac.p, S->vstar.p, S->rho.p,
                              q.status_centre, q.status_radius, out + 4);
  }
  ISPH_CHECK(tgv_error_device(S->ctx, S->nlocal, S->x.p, S->vstar.p, S->p.p, S->rho.p, S->nu.p, t, q.tgv_umax, out));
  return status_device(S->ctx, S->nlocal, q.status_type_mask, S->x.p, S->type.p, S->vfrac.p, S->vstar.p, S->rho.p, q.status_centre,
                       q.status_radius, out + 4);
}

int isph_ins_run(isph_ins *S, int nsteps, double *diag) {
  ISPH_REQUIRE(S && S->has_state && nsteps >= 0, "isph_ins_run: no state, or nsteps < 0");
  for (int k = 0; k < nsteps; ++k) {
    if (S->moved || !S->has_list) ISPH_CHECK(isph_ins_rebuild(S));
    ISPH_CHECK(isph_ins_pre(S));
    isph_ins_info info;
    ISPH_CHECK(isph_ins_solve(S, &info));
    const long long step = S->step + 1;
    if (diag) {
      double *row = diag + 16 * (size_t)k;
      ISPH_CHECK(isph_ins_diagnostics(S, (double)step * S->prm.dt, row));
      row[12] = info.helmholtz.iters; row[13] = info.poisson.iters;
      row[14] = info.helmholtz.converged; row[15] = info.poisson.converged;
    }
    ISPH_CHECK(isph_ins_advance(S));
    if (S->prm.shift > 0.0) ISPH_CHECK(isph_ins_shift(S, nullptr));
    S->step = step;
  }
  return ISPH_SUCCESS;
}

}  // extern "C"
