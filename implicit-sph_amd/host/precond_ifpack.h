// precond_ifpack.h -- PrecondWrapper_Ifpack over the HIP block-Jacobi ILU(k)
// (ref: precond_ifpack.h:28-85: same parameter keys and defaults).
#pragma once
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "halo_lists.h"
#include "precond.h"

namespace LAMMPS_NS {

class PrecondWrapper_Ifpack : public PrecondWrapper {
 public:
  PrecondWrapper_Ifpack(MPI_Comm comm) : PrecondWrapper(comm) {}
  virtual ~PrecondWrapper_Ifpack() {}

  virtual Teuchos::ParameterList *setParameters(Teuchos::ParameterList *param = NULL) {
    if (param == NULL) {
      _param = Teuchos::rcp(new Teuchos::ParameterList);
      _param->set("fact: drop tolerance", 1e-9);   // ref: precond_ifpack.h:34 (unused by ILU)
      _param->set("fact: level-of-fill", 1);       // :35
      _param->set("schwarz: combine mode", "Add"); // :39
      _param->set("Precond Type", "ILU");          // :42
      _param->set("Overlap Level", 1);             // :43
      // device-side extension (not a reference key): rows per additive-Schwarz subdomain inside a rank.  512 = the
      // block stream of csrc/ilu.hpp (throughput path); 0 = one subdomain per rank = the whole local matrix, what the
      // reference factors (level-scheduled, csrc/schwarz.hpp); > 1024 = large subdomains with "Overlap Level" layers.
      _param->set("isph: block rows", 512);
      // device-side extension (not a reference key), "Precond Type" = "ILU" only: "isph: ilu value bits" = 32 makes the
      // triangular solves of the block stream read the strict-L / strict-U values rounded to float
      // (isph_ilu_params::value_bits).  Not set here: absent means 64.
      // device-side extension (not a reference type): "Precond Type" = "GMRES Polynomial" is Belos' GMRES polynomial in
      // D^-1 A as a fixed preconditioner (isph_prec_create_gmres_poly) with "isph: polynomial degree" roots (1..25,
      // absent means 4); the null vector of a singular system is passed on (setNullVector).
    } else if (_param.get() != param) {
      _param = Teuchos::rcp(param, false);
    }
    return _param.get();
  }

  // Device-side extension (not a reference method): the additive-Schwarz subdomains INSIDE this rank as consecutive row
  // ranges, block b = rows block_ptr[b] .. block_ptr[b+1] (at most 1024 rows each).  The reference has one subdomain per
  // rank, a brick of LAMMPS' decomposition; an adapter that numbers the rank's particles brick by brick passes the brick
  // boundaries here and gets compact subdomains instead of a cut every "isph: block rows" rows.  Any level of fill,
  // overlap 0 (isph_prec_create_blocks_fill).  nblocks = 0 clears the table.
  void setSubdomains(int nblocks, const int *block_ptr) {
    _bptr.clear();
    if (nblocks > 0 && block_ptr != NULL) _bptr.assign(block_ptr, block_ptr + nblocks + 1);
  }

  // Device-side extension with the signature of PrecondWrapper_ML::setCoordinates (ref: precond_ml.h:25,63-94): the
  // coordinates of the rank's rows (three arrays of NumMyRows doubles, borrowed until the solve; z unused in 2-D).  The
  // reference hands coordinates to ML only (pair_isph.cpp:1290-1303); an adapter that makes the same three-line call for
  // this wrapper gets the library's own row numbering for the host matrix: subdomains = compact bricks of about 500
  // particles, whatever the atom order (on the 100^3 TGV system in create_atoms order 71 iterations instead of 164).
  // INTEGRATION.md shows the call.  NULL pointers clear them.
  void setCoordinates(const int dim, double *x, double *y, double *z) { storeCoordinates(dim, x, y, z); }

  // "Precond Type" = "GMRES Polynomial" projects its set-up with the null vector of a singular system (borrowed until
  // the solve, as PrecondWrapper_ML borrows it); the other types have no use for it
  virtual void setNullVector(double *n) { _null = n; }
  virtual bool usesNullVector() const { return _param.get() != NULL && _param->get("Precond Type", "ILU") == "GMRES Polynomial"; }

 protected:
  // the throughput path (block-Jacobi ILU(0), overlap 0 inside the rank) can be built during the matrix ingress
  virtual int fusedIngressBlockRows() {
    setParameters(_param.get());
    const int block = _param->get("isph: block rows", 512);
    // coordinates: the matrix crosses the link as it lies in the caller's memory and is permuted on the device; the set-up
    // follows in createOnDevice.  (isph_mat_create_csr_coords_bjacobi stages the rows in the new order on the host and
    // runs the set-up behind the link; on the 16-core share of the GPU box the gathered staging reaches 35 GB/s where
    // the flat copy reaches 54, so the fused form loses 5-10 ms against this one: profiles/r05_dropin.txt)
    if (_cx != nullptr) return 0;
    if (_param->get("Precond Type", "ILU") != "ILU" || _param->get("fact: level-of-fill", 1) != 0) return 0;
    // the fused set-up builds an fp64 stream: any other width is built (or refused) in createOnDevice
    if (_param->get("isph: ilu value bits", 64) != 64) return 0;
    if (tableUsable()) {
      int cap = 64;
      for (size_t b = 0; b + 1 < _bptr.size(); ++b) cap = std::max(cap, _bptr[b + 1] - _bptr[b]);
      noticeOnce(0, cap, _param->get("Overlap Level", 1));
      return (cap + 63) / 64 * 64;
    }
    if (block < 64 || block > 1024 || block % 64 != 0) return 0;
    noticeOnce(0, block, _param->get("Overlap Level", 1));
    return block;
  }
  // A table that does not fit the matrix at hand -- left over from a matrix with another row count, a subdomain above
  // the 1024 rows of the block stream, offsets that do not ascend -- is set aside with a notice and the solve goes on
  // with "isph: block rows" consecutive rows; it never fails the solve.
  bool tableUsable() {
    if (_bptr.empty()) return false;
    const int nrows = _A.get() != NULL ? _A->NumMyRows() : -1;
    bool ok = _bptr.front() == 0 && (nrows < 0 || _bptr.back() == nrows);
    for (size_t b = 0; ok && b + 1 < _bptr.size(); ++b) ok = _bptr[b + 1] > _bptr[b] && _bptr[b + 1] - _bptr[b] <= 1024;
    if (!ok && _comm.MyPID() == 0 && !_warned_table) {
      std::printf(">> PrecondWrapper_Ifpack(HIP): the subdomain table of setSubdomains does not fit this matrix (rows %d, table "
                  "ends at %d, blocks of 1..1024 rows required): ignored, subdomains are \"isph: block rows\" consecutive rows\n",
                  nrows, _bptr.back());
      _warned_table = true;
    }
    return ok;
  }
  virtual bool orderedIngressFusable() {
    setParameters(_param.get());
    const int block = _param->get("isph: block rows", 512);
    return _param->get("Precond Type", "ILU") == "ILU" && _param->get("fact: level-of-fill", 1) == 0 && block > 0 && block <= 1024 &&
           _param->get("isph: ilu value bits", 64) == 64;   // the fused set-up builds an fp64 stream
  }
  virtual bool fusedIngressSubdomains(int &nblocks, const int *&bptr) {
    if (_cx != nullptr || !tableUsable()) return false;   // with coordinates the library's own bricks win over a table
    nblocks = (int)_bptr.size() - 1;
    bptr = _bptr.data();
    return true;
  }
  void noticeOnce(int fill, int block, int overlap) {
    if (_comm.MyPID() == 0 && !_warned) {
      if (block < 0)
        std::printf(">> PrecondWrapper_Ifpack(HIP): block-Jacobi ILU(%d) on the library's bricks of about 500 particles (rows "
                    "numbered by the coordinates of setCoordinates), overlap 0 (reference: one subdomain per rank, Overlap Level %d)\n",
                    fill, overlap);
      else
        std::printf(">> PrecondWrapper_Ifpack(HIP): block-Jacobi ILU(%d) on %d-row subdomains, overlap 0 (reference: one "
                    "subdomain per rank, Overlap Level %d); set \"isph: block rows\" = 0 for the reference's decomposition\n",
                    fill, block, overlap);
      _warned = true;
    }
  }
  virtual int createOnDevice(isph_ctx *ctx, const isph_mat *A) {
    setParameters(_param.get());
    const std::string type = _param->get("Precond Type", "ILU");
    const int fill = _param->get("fact: level-of-fill", 1);
    const int overlap = _param->get("Overlap Level", 1);
    if (type == "Chebyshev") {
      // Ifpack_Chebyshev with its own keys and defaults; a polynomial in D^-1 A has no subdomains and no overlap
      isph_cheb_params cp;
      isph_cheb_params_default(&cp);
      cp.degree = _param->get("chebyshev: degree", cp.degree);
      cp.ratio = _param->get("chebyshev: ratio eigenvalue", cp.ratio);
      cp.lambda_max = _param->get("chebyshev: max eigenvalue", cp.lambda_max);
      cp.lambda_min = _param->get("chebyshev: min eigenvalue", cp.lambda_min);
      // device-side extension (not a reference key): 32 = the sweeps read the matrix values rounded to float, the
      // polynomial is that of fl32(A) (isph_cheb_params::value_bits).  Read for this type only.
      cp.value_bits = _param->get("isph: chebyshev value bits", 64);
      if (cp.value_bits != 64 && cp.value_bits != 32) {
        std::fprintf(stderr, ">> PrecondWrapper_Ifpack(HIP): \"isph: chebyshev value bits\" = %d is not available; available: 64, 32\n",
                     cp.value_bits);
        return ISPH_FAILURE;
      }
      // device-side extensions (not reference keys): where "chebyshev: max eigenvalue" is not given, "Anorm" (the default)
      // takes lambda_max = rho = ||D^-1 A||_inf, "arnoldi" the estimate after "... iterations" Arnoldi steps, clipped by rho
      // (isph_cheb_params::eig_type)
      const std::string eig = _param->get("isph: chebyshev eigen-analysis", "Anorm");
      if (eig != "Anorm" && eig != "arnoldi") {
        std::fprintf(stderr, ">> PrecondWrapper_Ifpack(HIP): \"isph: chebyshev eigen-analysis\" = '%s' is not available; available: "
                             "\"Anorm\", \"arnoldi\"\n", eig.c_str());
        return ISPH_FAILURE;
      }
      cp.eig_type = eig == "arnoldi" ? 1 : 0;
      cp.eig_iters = _param->get("isph: chebyshev eigen-analysis iterations", cp.eig_iters);
      if (_comm.MyPID() == 0 && !_warned) {
        std::printf(">> PrecondWrapper_Ifpack(HIP): Chebyshev polynomial of degree %d in D^-1 A (%d-bit matrix values); "
                    "\"Overlap Level\" and \"isph: block rows\" mean nothing for this type and are ignored\n", cp.degree,
                    cp.value_bits);
        _warned = true;
      }
      // holdPattern: the polynomial kept by free() is set up again on the updated matrix (nothing of a pattern is kept:
      // bit for bit the fresh create)
      if (refactorKept(ctx, A)) return ISPH_SUCCESS;
      destroyDevice();
      _kept_sig = deviceSignature();
      const int rc = isph_prec_create_chebyshev(ctx, A, &cp, &_M);
      _refreshable = rc == ISPH_SUCCESS;
      return rc;
    }
    if (type == "GMRES Polynomial") {
      // Belos' GMRES polynomial in D^-1 A: no subdomains, no overlap, no interval
      isph_poly_params pp;
      isph_poly_params_default(&pp);
      pp.degree = _param->get("isph: polynomial degree", pp.degree);
      if (_comm.MyPID() == 0 && !_warned) {
        std::printf(">> PrecondWrapper_Ifpack(HIP): GMRES polynomial of degree %d in D^-1 A%s; \"Overlap Level\" and \"isph: block "
                    "rows\" mean nothing for this type and are ignored\n", pp.degree, _null != nullptr ? " with the null vector" : "");
        _warned = true;
      }
      // (a kept polynomial is not refreshed: its null vector is borrowed per solve -- the set-up runs again)
      destroyDevice();
      _kept_sig = deviceSignature();
      return isph_prec_create_gmres_poly(ctx, A, &pp, _null, /*on_device=*/0, &_M);
    }
    if (type != "ILU") {
      std::fprintf(stderr, ">> PrecondWrapper_Ifpack(HIP): Precond Type '%s' is not available; available: \"ILU\", \"Chebyshev\", "
                           "\"GMRES Polynomial\"\n",
                   type.c_str());
      return ISPH_FAILURE;
    }
    if (fill < 0 || fill > 8) {
      std::fprintf(stderr, ">> PrecondWrapper_Ifpack(HIP): fact: level-of-fill %d is outside [0,8]\n", fill);
      return ISPH_FAILURE;
    }
    // device-side extension (not a reference key): 32 = the block stream's solves read the factor values rounded to float
    // (isph_ilu_params::value_bits).  Read for this type only; honoured on the three block-Jacobi routes below.
    const int bits = _param->get("isph: ilu value bits", 64);
    if (bits != 64 && bits != 32) {
      std::fprintf(stderr, ">> PrecondWrapper_Ifpack(HIP): \"isph: ilu value bits\" = %d is not available; available: 64, 32\n", bits);
      return ISPH_FAILURE;
    }
    // holdPattern: a block-stream ILU kept by free() takes the new values of the updated matrix and is done
    if (refactorKept(ctx, A)) return ISPH_SUCCESS;
    destroyDevice();
    _kept_sig = deviceSignature();
    const int block = _param->get("isph: block rows", 512);
    const std::string mode = _param->get("schwarz: combine mode", "Add");
    // "isph: block rows" = 0: the reference's own decomposition -- one subdomain per rank = the whole local matrix,
    // ILU(fill) level-scheduled on the device (isph_prec_create_schwarz).  "Overlap Level" extends a subdomain by rows
    // of the neighbouring RANKS (Ifpack ignores it on one rank): level 1 = the rows of the matrix' ghost columns,
    // fetched with the matrix' importer (halo_lists.h) and factored with the rank's own (isph_prec_create_overlap);
    // level L > 1 = L such layers, each gathered by one all-to-all round (rows of non-neighbour ranks included).
    // The choice is made from rank-uniform information (the parameters and "does ANY rank have ghost columns"): the row
    // import below is collective, so a rank without ghost columns -- an isolated subdomain -- must enter it as well,
    // with empty lists, and a failure on one rank must fail all of them.
    const int any_ghosts = _A.get() != NULL ? _comm.MaxAll(_A->NumMyCols() > _A->NumMyRows() ? 1 : 0) : 0;
    if (bits == 32 && ((block == 0 && overlap >= 1 && any_ghosts) || (!tableUsable() && (block == 0 || block > 1024)))) {
      // the level-scheduled Schwarz and overlap routes have no float plane: refused, never built in fp64 silently
      std::fprintf(stderr, ">> PrecondWrapper_Ifpack(HIP): \"isph: ilu value bits\" = 32 is not available with \"isph: block rows\" = %d "
                           "(the Schwarz and overlap routes stream fp64 only); choose \"isph: block rows\" in 64..1024, a table of "
                           "subdomains or coordinates, or 64 bits\n", block);
      return ISPH_FAILURE;
    }
    isph_ilu_params ip;
    isph_ilu_params_default(&ip);
    ip.level_of_fill = fill;
    ip.value_bits = bits;
    if (block == 0 && overlap >= 1 && any_ghosts) {
      HaloLists H, XH;
      std::vector<int> rp, ci;
      std::vector<double> v;
      int bad = halo_lists_from_import(*_A, H) != ISPH_SUCCESS ? 1 : 0;
      bool layered = false;
#ifdef ISPH_HAVE_MPI
      // more than one rank: L layers of imported rows, each its own all-to-all round (halo_lists.h extend_rows_levels)
      if (_comm.NumProc() > 1) {
        layered = true;
        if (_comm.MaxAll(bad) == 0) bad = extend_rows_levels(*_A, _comm, H, overlap, rp, ci, v, XH) != ISPH_SUCCESS ? 1 : 0;
      }
#endif
      if (!layered) {
        if (_comm.MaxAll(bad) == 0) bad = extend_rows_one_layer(*_A, _comm, H, rp, ci, v) != ISPH_SUCCESS ? 1 : 0;
        XH = H;
        if (overlap > 1 && _comm.MyPID() == 0 && !_warned) {  // the self-peer importer of a one-rank run: one layer
          std::printf(">> PrecondWrapper_Ifpack(HIP): Overlap Level %d on one rank with a self importer is factored as Overlap Level 1\n", overlap);
          _warned = true;
        }
      }
      if (_comm.MaxAll(bad)) {
        if (_comm.MyPID() == 0)
          std::fprintf(stderr, ">> PrecondWrapper_Ifpack(HIP): cannot import the rows of the ghost columns (Overlap Level %d)\n", overlap);
        return ISPH_FAILURE;
      }
      const int next = (int)rp.size() - 1;
      isph_mat *Aext = NULL;
      int ierr = isph_mat_create_csr(ctx, next, next, rp.data(), ci.data(), v.data(), 0, &Aext);
      if (ierr != ISPH_SUCCESS) return ierr;
      ierr = isph_prec_create_overlap(ctx, Aext, _A->NumMyRows(), fill, (mode == "Zero") ? 1 : 0, XH.npeers(), XH.peers.data(),
                                      XH.send_ptr.data(), XH.send_idx.data(), XH.recv_ptr.data(), &_M);
      isph_mat_destroy(Aext);
      return ierr;
    }
    if (tableUsable()) {  // the caller's subdomains (setSubdomains), any level of fill
      noticeOnce(fill, 0, overlap);
      ip.nblocks = (int)_bptr.size() - 1;
      ip.block_ptr = _bptr.data();
      _block_ilu = true;
      return isph_prec_create_ilu(ctx, A, &ip, &_M);   // 64 bits: isph_prec_create_blocks_fill, bit for bit
    }
    if (block == 0 || block > 1024) {
      isph_schwarz_params sp;
      isph_schwarz_params_default(&sp);
      sp.level_of_fill = fill;
      sp.block_size = block;
      sp.overlap = block == 0 ? 0 : overlap;    // subdomains inside one rank are extended by schwarz.hpp itself
      sp.combine = (mode == "Zero") ? 1 : 0;
      return isph_prec_create_schwarz(ctx, A, &sp, &_M);
    }
    {  // a matrix the library numbered itself (setCoordinates): its bricks are the subdomains
      long long oi[3] = {0, 0, 0};
      if (isph_mat_ordering_info(A, oi, NULL) == ISPH_SUCCESS && oi[0] == 1) {
        noticeOnce(fill, -1, overlap);
        ip.block_size = 0;
        _block_ilu = true;
        return isph_prec_create_ilu(ctx, A, &ip, &_M);   // 64 bits: isph_prec_create("bjacobi-ilu<fill>", 0), bit for bit
      }
    }
    // default: the throughput path -- block-Jacobi ILU(fill) on subdomains of `block` rows inside the rank, overlap 0.
    // This is NOT what the reference factors (one subdomain per rank, overlap 1): iteration counts differ (on the 100^3
    // TGV system 116 iterations against 49 for the whole-matrix ILU(0)); the notice is printed once, on every build.
    noticeOnce(fill, block, overlap);
    ip.block_size = block;
    _block_ilu = true;
    return isph_prec_create_ilu(ctx, A, &ip, &_M);   // 64 bits: isph_prec_create("bjacobi-ilu<fill>", block), bit for bit
  }
  // what a kept block-stream ILU was built with: any change between two held solves means a fresh build
  virtual std::string deviceSignature() {
    setParameters(_param.get());
    std::string sig = _param->get("Precond Type", "ILU");
    char buf[96];
    std::snprintf(buf, sizeof(buf), "|%d|%d|%d|%d|%d|", _param->get("fact: level-of-fill", 1), _param->get("isph: block rows", 512),
                  _param->get("isph: ilu value bits", 64), _param->get("Overlap Level", 1), _cx != nullptr ? _cdim : 0);
    sig += buf;
    for (int v : _bptr) { std::snprintf(buf, sizeof(buf), "%d,", v); sig += buf; }
    if (sig.compare(0, 9, "Chebyshev") == 0) {
      char cb[200];
      std::snprintf(cb, sizeof(cb), "|%d|%.17g|%.17g|%.17g|%d|%d|", _param->get("chebyshev: degree", 1),
                    _param->get("chebyshev: ratio eigenvalue", 30.0), _param->get("chebyshev: max eigenvalue", 0.0),
                    _param->get("chebyshev: min eigenvalue", 0.0), _param->get("isph: chebyshev value bits", 64),
                    _param->get("isph: chebyshev eigen-analysis iterations", 10));
      sig += cb;
      sig += _param->get("isph: chebyshev eigen-analysis", "Anorm");
    }
    if (sig.compare(0, 16, "GMRES Polynomial") == 0) {
      std::snprintf(buf, sizeof(buf), "|%d|%d|", _param->get("isph: polynomial degree", 4), _null != nullptr ? 1 : 0);
      sig += buf;
    }
    return sig;
  }
  double *_null = nullptr;  // setNullVector
  bool _warned = false, _warned_table = false;
  std::vector<int> _bptr;  // setSubdomains
};

}  // namespace LAMMPS_NS
