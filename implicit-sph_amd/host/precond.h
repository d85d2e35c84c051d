// precond.h -- PrecondWrapper: header-compatible with the reference
// (ref: precond.h:17-46) so PairISPH::initializeSolvers compiles unchanged,
// forwarding to libisph_hip through the C ABI (include/isph_hip.h).
#pragma once
#include <algorithm>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "isph_compat.h"
#include "isph_hip.h"

namespace LAMMPS_NS {

class SolverLin_HIP;
class PrecondWrapper;

// SolverLin_HIP::holdPattern: shared by the solver and the wrappers it has solved with while the pattern is held, so that
// either side may go first (a wrapper takes itself off the list when it is destroyed)
struct PatternHold {
  bool on = false;
  std::vector<PrecondWrapper *> precs;
};

class PrecondWrapper {
 protected:
  Epetra_MpiComm _comm;
  Teuchos::RCP<Teuchos::ParameterList> _param;
  Teuchos::RCP<Epetra_CrsMatrix> _A;
  // device side (owned): created by create(), released by free()
  isph_prec *_M = nullptr;
  friend class SolverLin_HIP;
  // hook used by SolverLin_HIP: build the device preconditioner for matrix A
  virtual int createOnDevice(isph_ctx *, const isph_mat *) { return ISPH_SUCCESS; }
  // > 0: this wrapper's device object is the block-Jacobi ILU(0) on subdomains of that many rows, which the host matrix
  // ingress can set up while the matrix is still crossing PCIe (isph_mat_create_csr_bjacobi); SolverLin_HIP then hands
  // the finished object over with adoptDevice() instead of calling createOnDevice()
  virtual int fusedIngressBlockRows() { return 0; }
  // the wrapper's own table of subdomains for that fused set-up (isph_mat_create_csr_blocks), if it has one
  virtual bool fusedIngressSubdomains(int &, const int *&) { return false; }
  void adoptDevice(isph_prec *M) { destroyDevice(); _M = M; _block_ilu = M != nullptr; _kept_sig = deviceSignature(); }
  // While SolverLin_HIP holds the pattern (holdPattern(true)), free() KEEPS the device object of a block-stream ILU: the next
  // createOnDevice on the updated matrix refactors it (isph_prec_refactor: Ifpack's Compute() without Initialize()) when
  // the wrapper's parameters are the ones it was built with.  So it does for a wrapper that marks its object _refreshable:
  // the Chebyshev polynomial of PrecondWrapper_Ifpack, and the hierarchy of PrecondWrapper_ML when "isph: amg refresh" asks
  // for ML's ReComputePreconditioner.  Every other device object is released as always.
  std::shared_ptr<PatternHold> _hold;
  bool _block_ilu = false;   // _M is a "bjacobi-ilu<k>" (the three block-Jacobi routes of PrecondWrapper_Ifpack, or adopted)
  bool _refreshable = false; // _M is a "chebyshev<d>" or an "sa-amg" whose wrapper wants it refreshed by isph_prec_refactor
  bool _kept = false;        // _M was kept by free(): stale until refactored
  bool _warned_refactor = false;
  std::string _kept_sig;     // the parameters _M was built with
  virtual std::string deviceSignature() { return std::string(); }
  void destroyDevice() {
    if (_M) { isph_prec_destroy(_M); _M = nullptr; }
    _block_ilu = false; _refreshable = false; _kept = false;
  }
  // true: the kept object now holds the factorisation of A; false: nothing kept (or it did not fit and was released)
  bool refactorKept(isph_ctx *ctx, const isph_mat *A) {
    if (!_kept || !_M) return false;
    if (_kept_sig == deviceSignature() && isph_prec_refactor(ctx, _M, A) == ISPH_SUCCESS) { _kept = false; return true; }
    if (_comm.MyPID() == 0 && !_warned_refactor) {
      std::printf(">> PrecondWrapper(HIP): the kept preconditioner could not be refactored (%s): built anew\n",
                  _kept_sig == deviceSignature() ? isph_last_error() : "its parameters changed");
      _warned_refactor = true;
    }
    destroyDevice();
    return false;
  }
  void dropKept() { destroyDevice(); _hold.reset(); }
  // Coordinates of the rows, as PrecondWrapper_ML::setCoordinates receives them (ref: precond_ml.h:63-94; borrowed
  // pointers into the adapter's Epetra_MultiVector, pair_isph.cpp:1290-1303).  When a wrapper has them, SolverLin_HIP
  // brings the host matrix in through isph_mat_create_csr_coords: the library then numbers the rows itself (bricks of
  // about 500 particles) instead of keeping LAMMPS' atom order.
  int _cdim = 0;
  const double *_cx = nullptr, *_cy = nullptr, *_cz = nullptr;
  void storeCoordinates(int dim, const double *x, const double *y, const double *z) {
    const bool ok = x != NULL && y != NULL && (dim == 2 || (dim == 3 && z != NULL));
    _cdim = ok ? dim : 0; _cx = ok ? x : nullptr; _cy = ok ? y : nullptr; _cz = ok ? z : nullptr;
  }
  // true when this wrapper's device object is the block ILU(0) on the library's bricks (fill 0), which
  // isph_mat_create_csr_coords_bjacobi can set up during the ordered ingress
  virtual bool orderedIngressFusable() { return false; }
  virtual bool ingressCoordinates(int &dim, const double *&x, const double *&y, const double *&z) {
    if (_cx == nullptr) return false;
    dim = _cdim; x = _cx; y = _cy; z = _cz;
    return true;
  }

 public:
  PrecondWrapper(MPI_Comm comm) : _comm(comm) {}
  virtual ~PrecondWrapper() {
    destroyDevice();
    if (_hold) _hold->precs.erase(std::remove(_hold->precs.begin(), _hold->precs.end(), this), _hold->precs.end());
  }

  virtual void setMatrix(Epetra_CrsMatrix *A) {
    if (A != NULL) _A = Teuchos::rcp(A, false);
  }
  // ref: precond.h:33-36.  The blocked operator is assembled from the scalar blocks SolverLin::setBlock was given, so
  // the Thyra object is accepted for interface compatibility and not used.
  virtual void setBlockMatrix(Thyra::PhysicallyBlockedLinearOpBase<double> *) { return; }
  virtual Teuchos::ParameterList *setParameters(Teuchos::ParameterList *param = NULL) { return _param.get(); }
  virtual void setNullVector(double *) { return; }  // base no-op, ref: precond.h:40
  // true when setNullVector() is more than the base no-op: SolverLin_HIP then forms the host copy of the null vector
  // before create() like the reference (solver_lin_belos.h:149-151); for the others the 8 n bytes are not touched per
  // solve (the device forms its own null vector from the mask) and getNullVector() builds the host copy on demand
  virtual bool usesNullVector() const { return false; }
  // The reference builds the Ifpack/ML object here; the device object needs the
  // device matrix, which SolverLin_HIP owns, so create() only records the request
  // and the build happens inside solveProblem (same place in the timeline:
  // solver_lin_belos.h:147-156), via createOnDevice().
  virtual void create() { return; }
  virtual void create(const int) { return; }
  virtual void free() {
    if (_M && (_block_ilu || _refreshable) && _hold && _hold->on) { _kept = true; return; }   // holdPattern: kept for isph_prec_refactor
    destroyDevice();
  }
  virtual Epetra_Operator *getPrecondOperator() { return NULL; }
  // ref: precond.h:45.  No Thyra operator crosses the boundary: solveBlockProblem applies the device preconditioner to
  // every component itself (precond_ml.h:138-155) and raises the reference's error when there is none.
  virtual Thyra::LinearOpBase<double> *getBlockPrecondOperator() { return NULL; }
};

}  // namespace LAMMPS_NS
