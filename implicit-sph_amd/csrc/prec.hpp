// prec.hpp -- the preconditioner object behind isph_prec_* (include/isph_hip.h): its kinds by name, the one way an object
// is created, the type strings of isph_prec_create, the application to one or several device vectors, the operand routes
// of the C entry points (host or device vectors, the caller's row numbering or the matrix' own) and the per-kind
// refactor.  isph_capi.hip checks the arguments of an entry point and calls into here; the kinds themselves live in
// ilu.hpp, amg.hpp, schwarz.hpp, chebyshev.hpp and gmres_poly.hpp, the overlap kind below.
#pragma once
#include <algorithm>
#include <vector>

#include "amg.hpp"
#include "chebyshev.hpp"
#include "comm.hpp"
#include "core.hpp"
#include "gmres_poly.hpp"
#include "ilu.hpp"
#include "schwarz.hpp"
#include "solver.hpp"

struct isph_overlap;  // below: overlap-1 Schwarz across ranks

namespace isph {

enum PrecKind : int {
  PREC_NONE = 0,
  PREC_JACOBI = 1,
  PREC_BJACOBI_ILU = 2,  // "bjacobi-ilu<k>": the block stream (ilu.hpp)
  PREC_AMG = 3,          // "sa-amg" (amg.hpp)
  PREC_SCHWARZ = 4,      // additive Schwarz ILU(k) (schwarz.hpp)
  PREC_OVERLAP = 5,      // ILU(k) of the rank's rows + one layer of the neighbours' rows (isph_prec_create_overlap)
  PREC_CHEBYSHEV = 6,    // Chebyshev polynomial in D^-1 A (chebyshev.hpp; applies the matrix it was built from: cheb_A must outlive it)
  PREC_GMRES_POLY = 7,   // GMRES polynomial in D^-1 A (gmres_poly.hpp; applies the matrix it was built from, like the Chebyshev kind)
  PREC_KINDS
};

inline int prec_multi_single_env() {
  const char *e = getenv("ISPH_PREC_MULTI_SINGLE");
  return e && e[0] == '1';
}
}  // namespace isph

struct isph_prec {
  isph::PrecKind type = isph::PREC_NONE;
  int n = 0;
  isph::DevBuf<double> invdiag;
  isph_ilu *ilu = nullptr;
  isph_amg *amg = nullptr;
  isph_schwarz *schwarz = nullptr;
  isph_overlap *ovl = nullptr;
  isph::Cheb *cheb = nullptr;
  const isph_mat *cheb_A = nullptr;  // ... and the matrix a GMRES polynomial applies
  isph::Poly *poly = nullptr;
  isph::RowOrderPtr order;  // the numbering of the matrix it was built from (isph_prec_apply takes the caller's)
  // ISPH_PREC_MULTI_SINGLE=1, read when the object is created: several vectors are applied one after the other whatever
  // one-sweep form the type has (prec_apply_multi_dev) -- the cross-check and the timing baseline of those forms
  int multi_single = isph::prec_multi_single_env();
};

// Ifpack_AdditiveSchwarz<ILU(k)> with "Overlap Level" 1 on more than one rank (precond_ifpack.h:43,60-74): the rank's
// subdomain is its own rows plus the rows of its ghost columns (Ifpack_OverlappingRowMatrix); the extended matrix is
// built by the caller (Epetra_Import of the rows; dist.extend_rows in the Python plumbing) and factored as one block by
// the level-scheduled path of schwarz.hpp.  An application gathers the ghost part of r with the matrix' halo plan,
// solves on the extended vector and -- combine mode Add, the wrapper's default -- sends the ghost part of the result
// back to its owners, who add it; Zero keeps the owned part only (restricted additive Schwarz).
struct isph_overlap {
  int n = 0, next = 0, combine = 0;
  isph_schwarz *inner = nullptr;
  isph_halo H;
  isph::DevBuf<double> rext, zext, sbuf, rbuf;
};

namespace isph {

// ---- the payload of a kind, or nullptr for an object of another kind --------------------------------------------------
inline isph_ilu *prec_ilu(const isph_prec *M) { return M && M->type == PREC_BJACOBI_ILU ? M->ilu : nullptr; }
inline isph_amg *prec_amg(const isph_prec *M) { return M && M->type == PREC_AMG ? M->amg : nullptr; }
// with_overlap: also the one subdomain inside an overlap object (prec_health reads its time-out word)
inline isph_schwarz *prec_schwarz(const isph_prec *M, bool with_overlap = false) {
  if (M && M->type == PREC_SCHWARZ) return M->schwarz;
  return M && with_overlap && M->type == PREC_OVERLAP && M->ovl ? M->ovl->inner : nullptr;
}
inline Cheb *prec_cheb(const isph_prec *M) { return M && M->type == PREC_CHEBYSHEV ? M->cheb : nullptr; }
inline Poly *prec_poly(const isph_prec *M) { return M && M->type == PREC_GMRES_POLY ? M->poly : nullptr; }

// ---- operands at the C ABI ----------------------------------------------------------------------------------------------
// upload helper: returns device pointer (either the caller's or a staged copy)
template <class T>
int stage_in(isph_ctx *ctx, const T *src, size_t n, int on_device, DevBuf<T> &tmp, const T **out) {
  if (on_device) { *out = src; return ISPH_SUCCESS; }
  ISPH_REQUIRE(!is_device_pointer(src), "device pointer passed with on_device = 0");
  ISPH_CHECK(tmp.reserve(n > 0 ? n : 1));
  ISPH_CHECK_HIP(hipMemcpyAsync(tmp.p, src, sizeof(T) * n, hipMemcpyHostToDevice, ctx->stream));
  *out = tmp.p;
  return ISPH_SUCCESS;
}

// K vectors of n rows from the caller's row numbering into the matrix' own (order.hpp): dst[k ld_dst + r] =
// src[k ld_src + perm[r]], one launch per vector.  nghost entries behind the n rows keep their place (the ghost values a
// caller hands to isph_spmv).
template <class T>
inline void order_gather(isph_ctx *ctx, const RowOrder &O, int n, int K, const T *src, size_t ld_src, T *dst, size_t ld_dst,
                         int nghost = 0) {
  const long long total = (long long)n + nghost;
  for (int k = 0; k < K; ++k)
    hipLaunchKernelGGL((k_perm_gather<T>), dim3(perm_grid(total)), dim3(kBlock), 0, ctx->stream, total, n, 1, (const int *)O.perm.p,
                       src + (size_t)k * ld_src, dst + (size_t)k * ld_dst);
}
// ... and back: dst[k ld_dst + perm[r]] = src[k ld_src + r]
template <class T>
inline void order_scatter(isph_ctx *ctx, const RowOrder &O, int n, int K, const T *src, size_t ld_src, T *dst, size_t ld_dst) {
  for (int k = 0; k < K; ++k)
    hipLaunchKernelGGL((k_perm_scatter<T>), dim3(perm_grid(n)), dim3(kBlock), 0, ctx->stream, n, (const int *)O.perm.p,
                       src + (size_t)k * ld_src, dst + (size_t)k * ld_dst);
}

// ---- the overlap kind -----------------------------------------------------------------------------------------------------
__global__ void k_scatter_add(int n, const int *__restrict__ idx, const double *__restrict__ v, double *__restrict__ z) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) z[idx[i]] += v[i];
}

inline void overlap_destroy(isph_overlap *O) {
  if (!O) return;
  if (O->inner) schwarz_destroy(O->inner);
  O->H.send_idx.release();
  O->rext.release(); O->zext.release(); O->sbuf.release(); O->rbuf.release();
  delete O;
}

// the halo lists are checked by the caller (isph_prec_create_overlap); *out is set at once: the owner destroys it on failure
inline int overlap_create(isph_ctx *ctx, const isph_mat *Aext, int nlocal, int level_of_fill, int combine, int npeers,
                          const int *peer_rank, const int *send_ptr, const int *send_idx, const int *recv_ptr, isph_overlap **out) {
  const int nrecv = npeers > 0 ? recv_ptr[npeers] : 0, nsend = npeers > 0 ? send_ptr[npeers] : 0;
  isph_overlap *O = new isph_overlap();
  *out = O;
  O->n = nlocal; O->next = nlocal + nrecv; O->combine = combine;
  isph_halo &H = O->H;
  H.npeers = npeers;
  H.peer.assign(peer_rank, peer_rank + npeers);
  H.send_ptr.assign(1, 0); H.recv_ptr.assign(1, 0);
  if (npeers > 0) { H.send_ptr.assign(send_ptr, send_ptr + npeers + 1); H.recv_ptr.assign(recv_ptr, recv_ptr + npeers + 1); }
  H.nsend = nsend; H.nrecv = nrecv;
  ISPH_CHECK(H.send_idx.reserve((size_t)(nsend > 0 ? nsend : 1)));
  if (nsend > 0 && hipMemcpyAsync(H.send_idx.p, send_idx, sizeof(int) * (size_t)nsend, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    return fail("copy of the send list failed", __FILE__, __LINE__);
  ISPH_CHECK(O->rext.reserve((size_t)(O->next > 0 ? O->next : 1)));
  ISPH_CHECK(O->zext.reserve((size_t)(O->next > 0 ? O->next : 1)));
  ISPH_CHECK(O->sbuf.reserve((size_t)(nsend > 0 ? nsend : 1)));
  ISPH_CHECK(O->rbuf.reserve((size_t)(nsend > 0 ? nsend : 1)));
  // one subdomain = the whole extended matrix, no further layers inside it
  ISPH_CHECK(schwarz_create(ctx, Aext, level_of_fill, /*block_size=*/0, /*overlap=*/0, /*combine=*/1, &O->inner));
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail("overlap set-up failed", __FILE__, __LINE__);
  return ISPH_SUCCESS;
}

inline int overlap_apply(isph_ctx *ctx, const isph_overlap *O, const double *r, double *z) {
  const isph_halo &H = O->H;
  const int n = O->n;
  // forward exchange: send[send range p] -> peer p, recv[recv range p] <- peer p; reverse: the two roles swapped
  ISPH_CHECK_HIP(hipMemcpyAsync(O->rext.p, r, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
  if (H.nsend > 0)
    hipLaunchKernelGGL(k_gather, dim3(stream_grid(H.nsend)), dim3(kBlock), 0, ctx->stream, H.nsend, (const int *)H.send_idx.p, r,
                       O->sbuf.p);
  ISPH_CHECK(comm_exchange(ctx, H, O->sbuf.p, O->rext.p + n, 1, /*reverse=*/false, ctx->stream));
  ISPH_CHECK(schwarz_apply(ctx, O->inner, O->rext.p, O->zext.p));
  ISPH_CHECK_HIP(hipMemcpyAsync(z, O->zext.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
  if (O->combine == 0 && H.npeers > 0) {  // Add: the neighbours' corrections of my rows come home (a rank may only send or only receive)
    ISPH_CHECK(comm_exchange(ctx, H, O->zext.p + n, O->rbuf.p, 1, /*reverse=*/true, ctx->stream));
    for (int p = 0; p < H.npeers; ++p) {  // one launch per peer: a row can be in several peers' lists, never twice in one
      const int s0 = H.send_ptr[(size_t)p], cnt = H.send_ptr[(size_t)p + 1] - s0;
      if (cnt > 0)
        hipLaunchKernelGGL(k_scatter_add, dim3(stream_grid(cnt)), dim3(kBlock), 0, ctx->stream, cnt, (const int *)H.send_idx.p + s0,
                           (const double *)O->rbuf.p + s0, z);
    }
  }
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

// ---- one way to create an object ----------------------------------------------------------------------------------------
inline void prec_destroy(isph_prec *M) {
  if (!M) return;
  M->invdiag.release();
  if (M->ilu) ilu_destroy(M->ilu);
  if (M->amg) amg_destroy(M->amg);
  if (M->schwarz) schwarz_destroy(M->schwarz);
  if (M->ovl) overlap_destroy(M->ovl);
  if (M->cheb) cheb_destroy(M->cheb);
  if (M->poly) poly_destroy(M->poly);
  delete M;
}

// An object under construction: n rows, its kind, and whatever the set-up has attached so far.  Leaving the scope before
// finish() -- an ISPH_CHECK of the set-up -- destroys it with its payload; finish() names the row numbering the object
// lives in (null: the caller's) and hands it out.
struct PrecNew {
  isph_prec *M;
  PrecNew(int n, PrecKind kind) : M(new isph_prec()) { M->n = n; M->type = kind; }
  PrecNew(const PrecNew &) = delete;
  ~PrecNew() { prec_destroy(M); }
  isph_prec *operator->() const { return M; }
  int finish(const RowOrderPtr &order, isph_prec **Mout) {
    M->order = order;
    *Mout = M;
    M = nullptr;
    return ISPH_SUCCESS;
  }
};

// the block capacity of the block stream for a table of subdomains: the widest one, rounded up to 64 rows
inline int ilu_block_cap(int nblocks, const int *block_ptr) {
  int cap = 64;
  for (int b = 0; b < nblocks; ++b) cap = std::max(cap, block_ptr[b + 1] - block_ptr[b]);
  return (cap + 63) / 64 * 64;
}

// the three routes of the block stream: the caller's table (nblocks > 0), the matrix' own subdomains (block_size <= 0), one
// block per block_size rows.  value_bits: 64 or 32 (checked by the caller)
inline int prec_ilu_init(isph_ctx *ctx, const isph_mat *A, int level_of_fill, int block_size, int nblocks, const int *block_ptr,
                         int value_bits, isph_prec *M) {
  if (nblocks > 0) {
    ISPH_REQUIRE(block_ptr, "NULL argument or no subdomains");
    ISPH_REQUIRE(level_of_fill >= 0 && level_of_fill <= 8, "level of fill must be in [0,8]");
    ISPH_REQUIRE(!is_device_pointer(block_ptr), "block_ptr must be a host array");
    ISPH_REQUIRE(!A->order, "the matrix was assembled in the library's own row numbering: its subdomains are the library's "
                            "bricks (isph_prec_create with block_size 0); a table over the caller's rows needs "
                            "isph_ctx_set_ordering(ctx, 0) before the assembly");
    const int cap = ilu_block_cap(nblocks, block_ptr);
    ISPH_REQUIRE(cap <= 1024, "a subdomain of the block stream holds at most 1024 rows (isph_prec_create_schwarz takes larger ones)");
    return ilu_create(ctx, A, cap, &M->ilu, /*sgs=*/false, level_of_fill, nblocks, block_ptr, value_bits);
  }
  if (block_size <= 0) {
    // the matrix' own subdomains: the bricks the assembly sorted the particles into (order.hpp)
    if (!A->order)
      return fail("block_size 0 selects the library's own subdomains: the matrix must come from an assembly entry point "
                  "with isph_ctx_set_ordering(ctx, 1)", __FILE__, __LINE__);
    const std::vector<int> &bp = A->order->block_ptr;
    return ilu_create(ctx, A, ilu_block_cap(A->order->nblocks(), bp.data()), &M->ilu, /*sgs=*/false, level_of_fill,
                      A->order->nblocks(), bp.data(), value_bits);
  }
  return ilu_create(ctx, A, block_size, &M->ilu, /*sgs=*/false, level_of_fill, 0, nullptr, value_bits);
}

inline int prec_jacobi_init(isph_ctx *ctx, const isph_mat *A, isph_prec *M) {
  ISPH_CHECK(M->invdiag.reserve((size_t)(M->n > 0 ? M->n : 1)));
  if (M->n > 0) {
    hipLaunchKernelGGL(k_sell_inv_diag, dim3((M->n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, M->n,
                       A->S.rowlen.p, A->S.slice_off.p, A->S.col.p, A->S.val.p, M->invdiag.p);
    if (hipGetLastError() != hipSuccess) return fail("jacobi setup failed", __FILE__, __LINE__);
  }
  return ISPH_SUCCESS;
}

inline int prec_chebyshev_init(isph_ctx *ctx, const isph_mat *A, const isph_cheb_params *prm, isph_prec *M) {
  ISPH_REQUIRE(prm->degree >= 1 && prm->degree <= kChebMaxDegree, "Chebyshev: degree must be in [1,16]");
  ISPH_REQUIRE(prm->ratio > 1.0, "Chebyshev: ratio (\"chebyshev: ratio eigenvalue\") must be > 1");
  ISPH_REQUIRE(prm->value_bits == 0 || prm->value_bits == 64 || prm->value_bits == 32,
               "Chebyshev: value_bits must be 64 (or 0: double values) or 32 (single-precision matrix values)");
  ISPH_REQUIRE(prm->eig_type == 0 || prm->eig_type == 1,
               "Chebyshev: eig_type must be 0 (the bound rho = ||D^-1 A||_inf) or 1 (the Arnoldi estimate)");
  ISPH_REQUIRE(prm->eig_iters >= 1 && prm->eig_iters <= kEigMaxIters, "Chebyshev: eig_iters must be in [1,50]");
  M->cheb_A = A;
  ISPH_CHECK(cheb_setup(ctx, A, prm->degree, prm->ratio, prm->lambda_max, prm->lambda_min, /*empty_ok=*/false,
                        /*collective=*/comm_active(ctx) && ctx->nranks > 1, /*prior_failure=*/false, &M->cheb,
                        prm->value_bits == 32 ? 32 : 64, prm->eig_type, prm->eig_iters, /*eig_level=*/0));
  M->cheb->held = ctx->pattern_hold;
  return ISPH_SUCCESS;
}

// the GMRES polynomial with the caller's null vector (host or device, the caller's numbering; may be NULL)
inline int prec_gmres_poly_init(isph_ctx *ctx, const isph_mat *A, const isph_poly_params *prm, const double *nullvec, int on_device,
                                isph_prec *M) {
  ISPH_REQUIRE(prm->degree >= 1 && prm->degree <= kPolyMaxDegree, "GMRES polynomial: degree must be in [1,25]");
  M->cheb_A = A;
  DevTmp<double> tn, tp;
  const double *dn = nullptr;
  if (nullvec) ISPH_CHECK(stage_in(ctx, nullvec, (size_t)M->n, on_device, tn, &dn));
  if (dn && A->order && M->n > 0) {  // the caller's null vector in the matrix' numbering
    ISPH_CHECK(tp.reserve((size_t)M->n));
    order_gather(ctx, *A->order, M->n, 1, dn, 0, tp.p, 0);
    dn = tp.p;
  }
  ISPH_CHECK(poly_create(ctx, A, prm->degree, dn, /*collective=*/comm_active(ctx) && ctx->nranks > 1, &M->poly));
  M->poly->held = ctx->pattern_hold;
  return ISPH_SUCCESS;
}

// the hierarchy with the caller's null vector (host or device, the caller's numbering; may be NULL)
inline int prec_amg_init(isph_ctx *ctx, const isph_mat *A, const isph_amg_params *prm, const double *nullvec, int on_device,
                         isph_prec *M) {
  DevTmp<double> tn, tp;
  const double *dn = nullptr;
  int rc = nullvec ? stage_in(ctx, nullvec, (size_t)M->n, on_device, tn, &dn) : ISPH_SUCCESS;
  if (rc == ISPH_SUCCESS && dn && A->order && M->n > 0) {  // the caller's null vector in the matrix' numbering
    rc = tp.reserve((size_t)M->n);
    if (rc == ISPH_SUCCESS) {
      order_gather(ctx, *A->order, M->n, 1, dn, 0, tp.p, 0);
      dn = tp.p;
    }
  }
  if (rc == ISPH_SUCCESS) rc = amg_create(ctx, A, prm, dn, &M->amg);
  tn.release(); tp.release();
  if (comm_active(ctx) && ctx->nranks > 1) {
    // Every level exchanges halos inside the cycle, and how often depends on the depth of the hierarchy and on the coarse
    // solver.  amg_create agrees on both between the ranks while it builds (amg.hpp); this is the last word on the outcome:
    // ranks that disagree would wait for each other forever -- fail on every rank together instead.
    double h[3] = {rc == ISPH_SUCCESS ? 1.0 : 0.0, (rc == ISPH_SUCCESS && M->amg->nlev > 1) ? 1.0 : 0.0,
                   (rc == ISPH_SUCCESS && M->amg->coarse_smooth) ? 1.0 : 0.0};
    const double nr = (double)ctx->nranks;
    if (comm_host_allreduce(ctx, h, 3, /*sum*/ 0) != ISPH_SUCCESS) rc = fail("AMG: set-up consensus between the ranks failed", __FILE__, __LINE__);
    else if (h[0] != nr) rc = rc != ISPH_SUCCESS ? rc : comm_failed_elsewhere("AMG");
    else if ((h[1] != 0.0 && h[1] != nr) || (h[1] == 0.0 && h[2] != 0.0 && h[2] != nr))
      rc = fail("AMG: the ranks built hierarchies of different depth; their fine-level halo exchanges would not match", __FILE__, __LINE__);
  }
  return rc;
}

// ---- the type strings of isph_prec_create -------------------------------------------------------------------------------
struct PrecSpec {
  PrecKind kind = PREC_NONE;
  int k = 0;            // "fact: level-of-fill" of the ILU kinds and of the AMG's ILU smoother; the degree of a polynomial
  int value_bits = 64;  // 32: the "-f32" forms
  int smoother = 0;     // isph_amg_params::smoother of the AMG forms
};

// a decimal number in [lo, hi] without sign or leading zero at s; s moves behind it
inline bool parse_prec_number(const char *&s, int lo, int hi, int *out) {
  if (*s < '0' || *s > '9' || (*s == '0' && s[1] >= '0' && s[1] <= '9')) return false;
  int v = 0;
  while (*s >= '0' && *s <= '9' && v <= hi) v = 10 * v + (*s++ - '0');
  if ((*s >= '0' && *s <= '9') || v < lo || v > hi) return false;
  *out = v;
  return true;
}

// none | jacobi | bjacobi-ilu<k>[-f32] | ilu<k> | sa-amg | sa-amg-ilu<k>, k = 0..8 | chebyshev<d>[-f32], d = 1..16 |
// gmres-poly<d>, d = 1..25
inline bool parse_prec_type(const char *type, PrecSpec *spec) {
  static const struct { const char *stem; PrecKind kind; int lo, hi; bool f32; int smoother; } forms[] = {  // lo > hi: no number
      {"none", PREC_NONE, 1, 0, false, 0},
      {"jacobi", PREC_JACOBI, 1, 0, false, 0},
      // "fact: level-of-fill" = k (precond_ifpack.h:35); "-f32": the same with value_bits = 32
      {"bjacobi-ilu", PREC_BJACOBI_ILU, 0, 8, true, 0},
      // ILU(k) of the whole local matrix -- what Ifpack factors on one MPI rank (the overlap is a no-op there)
      {"ilu", PREC_SCHWARZ, 0, 8, false, 0},
      // PrecondWrapper_ML defaults without a null vector (isph_prec_create_amg takes the full parameter set and the null
      // vector of a singular system); "-ilu<k>": ML's IFPACK smoother, block ILU(k) (smoother = 4, ilu_fill = k)
      {"sa-amg", PREC_AMG, 1, 0, false, 0},
      {"sa-amg-ilu", PREC_AMG, 0, 8, false, 4},
      // Ifpack's "Precond Type" = "Chebyshev" with "chebyshev: degree" = d and its other defaults; "-f32": value_bits = 32
      {"chebyshev", PREC_CHEBYSHEV, 1, kChebMaxDegree, true, 0},
      // Belos' GMRES polynomial of degree d in D^-1 A, without a null vector (isph_prec_create_gmres_poly takes one)
      {"gmres-poly", PREC_GMRES_POLY, 1, kPolyMaxDegree, false, 0}};
  for (const auto &f : forms) {
    const size_t len = strlen(f.stem);
    if (strncmp(type, f.stem, len) != 0) continue;
    const char *s = type + len;
    PrecSpec p;
    p.kind = f.kind; p.smoother = f.smoother;
    if (f.lo <= f.hi && !parse_prec_number(s, f.lo, f.hi, &p.k)) continue;
    if (f.f32 && !strcmp(s, "-f32")) { p.value_bits = 32; s += 4; }
    if (*s) continue;
    *spec = p;
    return true;
  }
  return false;
}

// isph_prec_create: block_size is the block of the block stream (0: the matrix' own subdomains) or the Gauss-Seidel block
// of the AMG's fine level
inline int prec_create_named(isph_ctx *ctx, const isph_mat *A, const char *type, int block_size, isph_prec **Mout) {
  PrecSpec s;
  if (!parse_prec_type(type, &s))
    return fail("unknown preconditioner type (none|jacobi|bjacobi-ilu<k>|ilu<k>|sa-amg-ilu<k>, k = 0..8|sa-amg|chebyshev<d>|chebyshev<d>-f32, d = 1..16|bjacobi-ilu<k>-f32)|gmres-poly<d>, d = 1..25", __FILE__, __LINE__);
  PrecNew M(A->S.nrow, s.kind);
  switch (s.kind) {
    case PREC_JACOBI: ISPH_CHECK(prec_jacobi_init(ctx, A, M.M)); break;
    case PREC_BJACOBI_ILU: ISPH_CHECK(prec_ilu_init(ctx, A, s.k, block_size, 0, nullptr, s.value_bits, M.M)); break;
    case PREC_SCHWARZ: ISPH_CHECK(schwarz_create(ctx, A, s.k, /*block_size=*/0, /*overlap=*/0, /*combine=*/0, &M->schwarz)); break;
    case PREC_AMG: {
      isph_amg_params prm;
      isph_amg_params_default(&prm);
      prm.block = block_size;
      if (s.smoother) { prm.smoother = s.smoother; prm.ilu_fill = s.k; }
      ISPH_CHECK(amg_create(ctx, A, &prm, nullptr, &M->amg));
      break;
    }
    case PREC_CHEBYSHEV: {
      isph_cheb_params prm;
      isph_cheb_params_default(&prm);
      prm.degree = s.k;
      prm.value_bits = s.value_bits;
      ISPH_CHECK(prec_chebyshev_init(ctx, A, &prm, M.M));
      break;
    }
    case PREC_GMRES_POLY: {
      isph_poly_params prm;
      isph_poly_params_default(&prm);
      prm.degree = s.k;
      ISPH_CHECK(prec_gmres_poly_init(ctx, A, &prm, nullptr, 0, M.M));
      break;
    }
    default: break;  // PREC_NONE: the identity
  }
  return M.finish(A->order, Mout);
}

// ---- application ----------------------------------------------------------------------------------------------------------
// The persistent triangular sweeps of the Schwarz path (schwarz.hpp k_gilu_solve_run) give up after a spin limit, store
// zeros and raise a word that the application copies to S->h_tmo.  Called with the stream DRAINED at the end of every
// solve / host-side application: a raised word fails the call -- on every rank together (one small max-reduction per
// solve; a rank that returned alone would leave the others waiting in their next collective) -- and is cleared, so one
// spurious time-out (a shared device, a debugger) does not poison the object.  A silently zeroed M^-1 r is never
// reported as a converged solve.
inline int prec_health(isph_ctx *ctx, const isph_prec *M) {
  if (!M || (M->type != PREC_SCHWARZ && M->type != PREC_OVERLAP)) return ISPH_SUCCESS;
  const isph_schwarz *S = prec_schwarz(M, /*with_overlap=*/true);
  double bad = 0.0;
  if (S && S->syncfree && S->h_tmo && *S->h_tmo != 0) {
    bad = 1.0;
    *S->h_tmo = 0;
    ISPH_CHECK_HIP(hipMemsetAsync(S->ctr.p + 3, 0, sizeof(int), ctx->stream));
  }
  if (comm_active(ctx) && ctx->nranks > 1) {
    ISPH_CHECK(ensure_scalars(ctx));
    double *d = ctx->dscal.p + SC_MISC + 30;
    ISPH_CHECK_HIP(hipMemcpyAsync(d, &bad, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ISPH_CHECK(comm_allreduce(ctx, d, 1, /*max*/ 1, ctx->stream));
    ISPH_CHECK_HIP(hipMemcpyAsync(&bad, d, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  }
  if (bad != 0.0)
    return fail("Schwarz ILU sweep: a row waited for a dependency beyond the spin limit; the result of this call is not valid", __FILE__, __LINE__);
  return ISPH_SUCCESS;
}

inline int prec_apply_dev(isph_ctx *ctx, const isph_prec *M, const double *r, double *z) {
  ISPH_REQUIRE(M != nullptr, "preconditioner is NULL");
  const int n = M->n;
  ProfScope prof(ctx, PROF_PREC_APPLY);
  switch (M->type) {
    case PREC_NONE:  // identity: callers pass distinct buffers
      if (r != z) ISPH_CHECK_HIP(hipMemcpyAsync(z, r, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
      return ISPH_SUCCESS;
    case PREC_JACOBI:
      hipLaunchKernelGGL(k_mul_elem, dim3(stream_grid(n)), dim3(kBlock), 0, ctx->stream, n, r, M->invdiag.p, z);
      return ISPH_SUCCESS;
    case PREC_AMG: return amg_apply(ctx, M->amg, r, z);
    case PREC_SCHWARZ: return schwarz_apply(ctx, M->schwarz, r, z);
    case PREC_OVERLAP: return overlap_apply(ctx, M->ovl, r, z);
    case PREC_CHEBYSHEV: return cheb_apply(ctx, M->cheb_A, M->cheb, r, z, /*zero_guess=*/true);
    case PREC_GMRES_POLY: return poly_apply(ctx, M->cheb_A, M->poly, r, z);
    default: return ilu_apply(ctx, M->ilu, r, z);
  }
}

// whether K vectors share the sweeps of M (isph_prec_multi_path).  Block ILU(k): 2..4 vectors in one sweep of the factor
// stream (ilu_multi_shared, the rule ilu_apply_multi acts on).  The Chebyshev polynomial and the fp64 V cycle of the
// Chebyshev-smoothed AMG: any K >= 2, in groups of up to kPrecMultiMax.
constexpr int kPrecMultiMax = 4;
inline bool prec_multi_shared(const isph_prec *M, int K) {
  if (!M || K < 2 || M->multi_single) return false;
  if (prec_ilu(M)) return ilu_multi_shared(M->ilu, K);
  if (M->type == PREC_CHEBYSHEV) return cheb_multi_ok(M->cheb_A, M->cheb);
  if (M->type == PREC_AMG) return amg_multi_ok(M->amg);
  return false;
}

// K applications of one preconditioner: block ILU(k) sweeps its factor stream once for all vectors, the Chebyshev
// polynomial and the Chebyshev-smoothed fp64 V cycle sweep every operator once per group of up to four vectors
// (cheb_apply_multi, amg_apply_multi).  Everything else -- and everything under ISPH_PREC_MULTI_SINGLE=1 -- applies the
// vectors one after the other; the bits are the same either way.
inline int prec_apply_multi_dev(isph_ctx *ctx, const isph_prec *M, int K, const double *const *rs, double *const *zs) {
  ISPH_REQUIRE(M != nullptr, "preconditioner is NULL");
  if (!M->multi_single && prec_ilu(M)) return ilu_apply_multi(ctx, M->ilu, K, rs, zs);
  const bool cheb = M->type == PREC_CHEBYSHEV;
  if ((cheb || M->type == PREC_AMG) && prec_multi_shared(M, K)) {
    ProfScope prof(ctx, PROF_PREC_APPLY);
    for (int k0 = 0; k0 < K; k0 += kPrecMultiMax) {
      const int g = std::min(kPrecMultiMax, K - k0);
      if (g == 1) ISPH_CHECK(cheb ? cheb_apply(ctx, M->cheb_A, M->cheb, rs[k0], zs[k0], /*zero_guess=*/true)
                                  : amg_apply(ctx, M->amg, rs[k0], zs[k0]));
      else if (cheb) ISPH_CHECK(cheb_apply_multi(ctx, M->cheb_A, M->cheb, g, rs + k0, zs + k0, /*zero_guess=*/true));
      else ISPH_CHECK(amg_apply_multi(ctx, M->amg, g, rs + k0, zs + k0));
    }
    return ISPH_SUCCESS;
  }
  for (int k = 0; k < K; ++k) ISPH_CHECK(prec_apply_dev(ctx, M, rs[k], zs[k]));
  return ISPH_SUCCESS;
}

// isph_prec_apply: r and z are the caller's -- host or device memory, the caller's row numbering.  Host operands are
// staged (beside the gathered copies in pool temporaries when the object lives in its matrix' numbering, in the context's
// own vectors otherwise); device operands in the caller's numbering go straight through, without a synchronisation.
inline int prec_apply_operands(isph_ctx *ctx, const isph_prec *M, const double *r, double *z, int on_device) {
  const size_t n = (size_t)M->n;
  const bool ordered = M->order && M->n > 0;
  if (!ordered && on_device) return prec_apply_dev(ctx, M, r, z);
  DevTmp<double> rc, ri, zi;
  if (!ordered) ISPH_CHECK(ctx->xdev.reserve(n > 0 ? n : 1));
  if (!ordered) ISPH_CHECK(ctx->bdev.reserve(n > 0 ? n : 1));
  const double *dr = nullptr;
  ISPH_CHECK(stage_in(ctx, r, n, on_device, ordered ? static_cast<DevBuf<double> &>(rc) : ctx->xdev, &dr));
  double *dz = on_device ? z : ordered ? rc.p : ctx->bdev.p;  // the result on the device, the caller's numbering
  if (ordered) {
    ISPH_CHECK(ri.reserve(n + 64));
    ISPH_CHECK(zi.reserve(n + 64));
    order_gather(ctx, *M->order, M->n, 1, dr, 0, ri.p, 0);
    ISPH_CHECK(prec_apply_dev(ctx, M, ri.p, zi.p));
    order_scatter(ctx, *M->order, M->n, 1, (const double *)zi.p, 0, dz, 0);
  } else {
    ISPH_CHECK(prec_apply_dev(ctx, M, dr, dz));
  }
  if (!on_device) ISPH_CHECK_HIP(hipMemcpyAsync(z, dz, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));  // the temporaries go back to the pool
  ISPH_CHECK_HIP(hipGetLastError());
  return prec_health(ctx, M);
}

// isph_prec_apply_multi: nvec vectors lda apart.  Host operands: one strided copy each way (the padding rows of z are not
// written); the matrix' own numbering: the vectors are gathered into it and the results scattered back, as
// prec_apply_operands does
inline int prec_apply_multi_operands(isph_ctx *ctx, const isph_prec *M, int nvec, const double *r, double *z, int lda, int on_device) {
  const int n = M->n;
  if (n == 0) return ISPH_SUCCESS;
  const size_t K = (size_t)nvec, ldd = ((size_t)n + 64 + 1) & ~(size_t)1, rowbytes = sizeof(double) * (size_t)n;
  const bool ordered = (bool)M->order;
  DevTmp<double> rin, ri, zi;
  const double *dr = r;
  double *dz = z;
  size_t ldr = (size_t)lda, ldz = (size_t)lda;
  if (!on_device) {
    ISPH_REQUIRE(!is_device_pointer(r) && !is_device_pointer(z), "device pointer passed with on_device = 0");
    ISPH_CHECK(rin.reserve(ldd * K));
    ISPH_CHECK_HIP(hipMemcpy2DAsync(rin.p, sizeof(double) * ldd, r, sizeof(double) * (size_t)lda, rowbytes, K, hipMemcpyHostToDevice, ctx->stream));
    dr = rin.p; ldr = ldd;
  }
  if (ordered) {
    ISPH_CHECK(ri.reserve(ldd * K));
    order_gather(ctx, *M->order, n, nvec, dr, ldr, ri.p, ldd);
    dr = ri.p; ldr = ldd;
  }
  if (ordered || !on_device) {
    ISPH_CHECK(zi.reserve(ldd * K));
    dz = zi.p; ldz = ldd;
  }
  std::vector<const double *> rs(K);
  std::vector<double *> zs(K);
  for (size_t k = 0; k < K; ++k) { rs[k] = dr + k * ldr; zs[k] = dz + k * ldz; }
  ISPH_CHECK(prec_apply_multi_dev(ctx, M, nvec, rs.data(), zs.data()));
  if (!ordered && on_device) return ISPH_SUCCESS;
  if (ordered) {   // back to the caller's numbering: into z itself on the device, into the staged r otherwise
    double *out = on_device ? z : rin.p;
    order_scatter(ctx, *M->order, n, nvec, (const double *)zi.p, ldd, out, on_device ? (size_t)lda : ldd);
    dz = out;
  }
  if (!on_device)
    ISPH_CHECK_HIP(hipMemcpy2DAsync(z, sizeof(double) * (size_t)lda, dz, sizeof(double) * ldd, rowbytes, K, hipMemcpyDeviceToHost, ctx->stream));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  ISPH_CHECK_HIP(hipGetLastError());
  return prec_health(ctx, M);
}

// a cycle_bits = 32 AMG is not a linear operator: only flexible GMRES keeps what it was applied to (Z); the other
// drivers form x += M^-1 (V y), the rounded cycle of a vector it never saw
inline int check_cycle_bits_solver(const isph_prec *M, const isph_solver_params *prm) {
  if (isph_prec_cycle_bits(M) != 32) return ISPH_SUCCESS;
  ISPH_REQUIRE(prm->solver_type == 0, "a preconditioner with cycle_bits = 32 needs flexible Block GMRES: solver_type 1 and 2 are not available with it");
  ISPH_REQUIRE(prm->flexible != 0, "a preconditioner with cycle_bits = 32 needs flexible = 1: the rounded cycle is not a linear operator");
  return ISPH_SUCCESS;
}

// ---- isph_prec_refactor, kind by kind ---------------------------------------------------------------------------------------
// "sa-amg" and "chebyshev<d>": the row count is checked here, everything else by the kind
inline int prec_refactor_rows(const isph_prec *M, const isph_mat *A) {
  if (A->S.nrow == M->n) return ISPH_SUCCESS;
  char msg[160];
  snprintf(msg, sizeof(msg), "refactor: the matrix has %d rows, the preconditioner was built for %d", A->S.nrow, M->n);
  return fail(msg, __FILE__, __LINE__);
}

// the hierarchy of the new values on the kept aggregates (amg.hpp amg_refactor)
inline int prec_refactor_amg(isph_ctx *ctx, isph_prec *M, const isph_mat *A) {
  ISPH_CHECK(prec_refactor_rows(M, A));
  ISPH_REQUIRE(M->order == A->order, "refactor: the matrix is not in the row numbering the AMG hierarchy was built in "
                                     "(the aggregates are sets of its rows): rebuild");
  return amg_refactor(ctx, M->amg, A);
}

// nothing of the pattern is kept: the set-up of the create call on the new values
inline int prec_refactor_chebyshev(isph_ctx *ctx, isph_prec *M, const isph_mat *A) {
  if (!M->cheb || !M->cheb->held)
    return fail("refactor of \"chebyshev<d>\": the polynomial was created while the pattern was not held (isph_ctx_hold_pattern "
                "was off): rebuild it", __FILE__, __LINE__);
  ISPH_CHECK(prec_refactor_rows(M, A));
  const Cheb *C0 = M->cheb;
  Cheb *C1 = nullptr;
  ISPH_CHECK(cheb_setup(ctx, A, C0->degree, C0->ratio_in, C0->lambda_max_in, C0->lambda_min_in, /*empty_ok=*/false,
                        /*collective=*/comm_active(ctx) && ctx->nranks > 1, /*prior_failure=*/false, &C1, C0->value_bits,
                        C0->eig_type_in, C0->eig_iters_in, /*eig_level=*/0));
  cheb_destroy(M->cheb);
  C1->held = true;
  M->cheb = C1;
  M->cheb_A = A;
  return ISPH_SUCCESS;
}

// ... and of "gmres-poly<d>": the Arnoldi steps, the roots and the steps again, with the null vector of the create call
inline int prec_refactor_gmres_poly(isph_ctx *ctx, isph_prec *M, const isph_mat *A) {
  if (!M->poly || !M->poly->held)
    return fail("refactor of \"gmres-poly<d>\": the polynomial was created while the pattern was not held (isph_ctx_hold_pattern "
                "was off): rebuild it", __FILE__, __LINE__);
  ISPH_CHECK(prec_refactor_rows(M, A));
  Poly *P0 = M->poly;
  ISPH_REQUIRE(!P0->has_null || M->order == A->order, "refactor: the matrix is not in the row numbering the null vector of the "
                                                      "GMRES polynomial was kept in: rebuild");
  Poly *P1 = new Poly();
  P1->degree_in = P0->degree_in; P1->unfused = P0->unfused; P1->has_null = P0->has_null; P1->held = true;
  std::swap(P1->nullv, P0->nullv);
  const int rc = poly_build(ctx, A, P1, /*collective=*/comm_active(ctx) && ctx->nranks > 1);
  if (rc != ISPH_SUCCESS) {   // the old polynomial stays whole
    std::swap(P1->nullv, P0->nullv);
    poly_destroy(P1);
    return rc;
  }
  poly_destroy(P0);
  M->poly = P1;
  M->cheb_A = A;
  return ISPH_SUCCESS;
}

// the numeric factorisation again.  The subdomains of the library's own numbering come with the matrix: they must be the
// ones the factor was laid out for
inline int prec_refactor_ilu(isph_ctx *ctx, isph_prec *M, const isph_mat *A) {
  const bool mo = (bool)M->order, ao = (bool)A->order;
  if (mo != ao || (mo && M->order != A->order && M->order->block_ptr != A->order->block_ptr)) {
    char msg[200];
    snprintf(msg, sizeof(msg), "refactor: the subdomain table differs (the preconditioner has %d subdomains %s the library's "
                               "numbering, the matrix %d)", M->ilu->nblocks, mo ? "in" : "outside",
             ao ? A->order->nblocks() : 0);
    return fail(msg, __FILE__, __LINE__);
  }
  return ilu_refactor(ctx, M->ilu, A->S);
}

inline int prec_refactor(isph_ctx *ctx, isph_prec *M, const isph_mat *A) {
  if (prec_amg(M)) ISPH_CHECK(prec_refactor_amg(ctx, M, A));
  else if (M->type == PREC_CHEBYSHEV) ISPH_CHECK(prec_refactor_chebyshev(ctx, M, A));
  else if (M->type == PREC_GMRES_POLY) ISPH_CHECK(prec_refactor_gmres_poly(ctx, M, A));
  else if (prec_ilu(M)) ISPH_CHECK(prec_refactor_ilu(ctx, M, A));
  else {
    static const char *const names[PREC_KINDS] = {"none", "jacobi", "bjacobi-ilu<k>", "sa-amg", "ilu<k> / additive Schwarz",
                                                  "overlap ILU(k)", "chebyshev<d>", "gmres-poly<d>"};
    char msg[200];
    snprintf(msg, sizeof(msg), "isph_prec_refactor applies to \"bjacobi-ilu<k>\", \"sa-amg\", \"chebyshev<d>\" and \"gmres-poly<d>\", not to a "
                               "preconditioner of type \"%s\": rebuild it", M->type >= 0 && M->type < PREC_KINDS ? names[M->type] : "?");
    return fail(msg, __FILE__, __LINE__);
  }
  M->order = A->order;
  return ISPH_SUCCESS;
}

}  // namespace isph
