// precond_ml.h -- PrecondWrapper_ML over the HIP smoothed-aggregation AMG
// (ref: precond_ml.h:28-171: same parameter keys and defaults, same setNullVector behaviour).
#pragma once
#include <cstdio>
#include <string>

#include "precond.h"

namespace LAMMPS_NS {

class PrecondWrapper_ML : public PrecondWrapper {
 public:
  PrecondWrapper_ML(MPI_Comm comm) : PrecondWrapper(comm) {}
  virtual ~PrecondWrapper_ML() {}

  virtual Teuchos::ParameterList *setParameters(Teuchos::ParameterList *param = NULL) {
    if (param == NULL) {
      _param = Teuchos::rcp(new Teuchos::ParameterList);
      _param->set("ML output", 10);                               // ref: precond_ml.h:46
      _param->set("max levels", 5);                               // :47
      _param->set("increasing or decreasing", "increasing");      // :48
      _param->set("aggregation: type", "Uncoupled");              // :49
      _param->set("smoother: type", "symmetric Gauss-Seidel");    // :50
      _param->set("smoother: sweeps", 1);                         // :51
      _param->set("smoother: pre or post", "both");               // :52
      _param->set("coarse: type", "Amesos-KLU");                  // :53
      // ML's own defaults, spelled out because the device side needs them
      _param->set("coarse: max size", 128);
      _param->set("aggregation: damping factor", 4.0 / 3.0);
      _param->set("aggregation: threshold", 0.0);
      // device-side extension: rows the Gauss-Seidel sweeps are local to (ML: the processor).  Not a reference key.
      _param->set("isph: block rows", 512);
      // device-side extension (not a reference key), read under SolverLin_HIP::holdPattern only: true = the hierarchy of
      // the first held solve is kept and REFRESHED on the values of the following ones (isph_prec_refactor: ML's
      // ReComputePreconditioner -- aggregates and patterns stand, every number is redone); false = rebuilt per solve
      _param->set("isph: amg refresh", false);
    } else if (_param.get() != param) {
      _param = Teuchos::rcp(param, false);
    }
    return _param.get();
  }

  // ref: precond_ml.h:62-94.  In the reference the coordinates feed ML's Zoltan repartitioning of the coarse rows, which
  // has no device counterpart; here they let the library number the matrix rows by position (precond.h
  // ingressCoordinates): the sliced-ELL slices and the Gauss-Seidel blocks of the smoother are then compact in space
  // whatever LAMMPS' atom order is.  NULL pointers clear them.
  virtual void setCoordinates(const int dim, double *x, double *y, double *z) { storeCoordinates(dim, x, y, z); }

  // ref: precond_ml.h:97-127 -- one pre-computed null-space vector; the smoother becomes the coarse solver
  virtual void setNullVector(double *n) { _null = n; }
  virtual bool usesNullVector() const { return true; }

 protected:
  virtual int createOnDevice(isph_ctx *ctx, const isph_mat *A) {
    setParameters(_param.get());
    const std::string agg = _param->get("aggregation: type", "Uncoupled");
    const std::string smo = _param->get("smoother: type", "symmetric Gauss-Seidel");
    // "symmetric Gauss-Seidel" (the wrapper's default), or ML's Gauss-Seidel with "smoother: Gauss-Seidel efficient
    // symmetric" -- forward sweeps before the coarse correction, backward sweeps after it -- which is what the ml.xml of
    // the reference's benchmark protocol asks for (bench-script/hopper/tgv/1728/ml.xml)
    const bool gs = smo == "ML Gauss-Seidel" || smo == "Gauss-Seidel";
    const bool eff = gs && _param->get("smoother: Gauss-Seidel efficient symmetric", false);
    // "Chebyshev" ("MLS" is ML's old name for it; the line the benchmark's ml.xml carries commented out): a polynomial of
    // degree "smoother: sweeps" in D^-1 A on [rho / "smoother: Chebyshev alpha", 1.1 rho]
    const bool cheb = smo == "Chebyshev" || smo == "MLS";
    // "IFPACK" with "smoother: ifpack type" = "ILU", "smoother: ifpack overlap" = 0 and "fact: level-of-fill" in the sublist
    // "smoother: ifpack list" (sph-script/ml-ifpack.xml): block ILU(k) Richardson sweeps, isph_amg_params::smoother = 4
    const bool ifpack = smo == "IFPACK";
    if (agg != "Uncoupled" || !(smo == "symmetric Gauss-Seidel" || eff || cheb || ifpack)) {
      std::fprintf(stderr, ">> PrecondWrapper_ML(HIP): aggregation '%s' with smoother '%s' is not available; available: "
                           "\"Uncoupled\" aggregation with \"symmetric Gauss-Seidel\", with \"Gauss-Seidel\" / \"ML Gauss-Seidel\" "
                           "plus \"smoother: Gauss-Seidel efficient symmetric\", with \"Chebyshev\" / \"MLS\", or with \"IFPACK\" "
                           "(\"smoother: ifpack type\" = \"ILU\")\n",
                   agg.c_str(), smo.c_str());
      return ISPH_FAILURE;
    }
    isph_amg_params prm;
    isph_amg_params_default(&prm);
    prm.smoother = ifpack ? 4 : cheb ? 2 : eff ? 1 : 0;
    if (ifpack) {
      const std::string itype = _param->get("smoother: ifpack type", "ILU");
      const int overlap = _param->get("smoother: ifpack overlap", 0);
      if (itype != "ILU") {
        std::fprintf(stderr, ">> PrecondWrapper_ML(HIP): \"smoother: ifpack type\" = '%s' is not available; available: \"ILU\"\n",
                     itype.c_str());
        return ISPH_FAILURE;
      }
      if (overlap != 0) {
        std::fprintf(stderr, ">> PrecondWrapper_ML(HIP): \"smoother: ifpack overlap\" = %d is not available; available: 0\n", overlap);
        return ISPH_FAILURE;
      }
      // Ifpack's default level of fill is 0; a value outside 0..8 is refused by the create call, ilu_fill named
      const Teuchos::ParameterList &ilist = *_param;
      prm.ilu_fill = ilist.sublist("smoother: ifpack list").get("fact: level-of-fill", 0);
    }
    if (cheb) prm.cheb_ratio = _param->get("smoother: Chebyshev alpha", 20.0);
    // device-side extension (not a reference key), read for the Chebyshev smoother only: 32 = the smoother's sweeps read
    // the level operators rounded to float (isph_amg_params::cheb_value_bits); the hierarchy itself stays fp64
    if (cheb) prm.cheb_value_bits = _param->get("isph: chebyshev value bits", 64);
    if (cheb && prm.cheb_value_bits != 64 && prm.cheb_value_bits != 32) {
      std::fprintf(stderr, ">> PrecondWrapper_ML(HIP): \"isph: chebyshev value bits\" = %d is not available; available: 64, 32\n",
                   prm.cheb_value_bits);
      return ISPH_FAILURE;
    }
    // device-side extension, read beside it: 32 = the whole V cycle in single-precision storage (isph_amg_params::cycle_bits;
    // the solver must then be flexible GMRES, SolverLin_Belos' default)
    if (cheb) prm.cycle_bits = _param->get("isph: amg cycle bits", 64);
    if (cheb && prm.cycle_bits != 64 && prm.cycle_bits != 32) {
      std::fprintf(stderr, ">> PrecondWrapper_ML(HIP): \"isph: amg cycle bits\" = %d is not available; available: 64, 32\n",
                   prm.cycle_bits);
      return ISPH_FAILURE;
    }
    // ML's own keys.  "Anorm" -- the bound rho = ||D^-1 A||_inf -- is this wrapper's default and a kept departure (ML's
    // default is "cg"); "cg" asks for the estimate after "eigen-analysis: iterations" steps, which the device takes with
    // Arnoldi (isph_amg_params::eig_type = 1: correct for the nonsymmetric matrices too, the same projection otherwise)
    const std::string eig = _param->get("eigen-analysis: type", "Anorm");
    if (eig != "Anorm" && eig != "cg") {
      std::fprintf(stderr, ">> PrecondWrapper_ML(HIP): \"eigen-analysis: type\" = '%s' is not available; available: \"Anorm\", \"cg\"\n",
                   eig.c_str());
      return ISPH_FAILURE;
    }
    prm.eig_type = eig == "cg" ? 1 : 0;
    prm.eig_iters = _param->get("eigen-analysis: iterations", 10);
    // (ml.xml of the benchmark protocol asks for 10 levels; the device hierarchy holds 8, and 3-4 are reached at 10^6 rows)
    prm.max_levels = _param->get("max levels", 5) > 8 ? 8 : _param->get("max levels", 5);
    prm.coarse_max = _param->get("coarse: max size", 128);
    prm.omega = _param->get("aggregation: damping factor", 4.0 / 3.0);
    prm.theta = _param->get("aggregation: threshold", 0.0);
    prm.sweeps = _param->get("smoother: sweeps", 1);
    prm.block = _param->get("isph: block rows", 512);
    // holdPattern with "isph: amg refresh": the hierarchy kept by free() takes the null vector of this solve and the new
    // values of the updated matrix and is done; any changed parameter (deviceSignature) means a fresh build
    if (_kept && _M && _null != nullptr && _kept_sig == deviceSignature()) (void)isph_prec_amg_set_nullvec(ctx, _M, _null, 0);
    if (refactorKept(ctx, A)) return ISPH_SUCCESS;
    destroyDevice();
    _kept_sig = deviceSignature();
    const int rc = isph_prec_create_amg(ctx, A, &prm, _null, /*on_device=*/0, &_M);
    _refreshable = rc == ISPH_SUCCESS && _param->get("isph: amg refresh", false);
    return rc;
  }
  // what a kept hierarchy was built with
  virtual std::string deviceSignature() {
    setParameters(_param.get());
    const Teuchos::ParameterList &ilist = *_param;
    std::string sig = _param->get("aggregation: type", "Uncoupled") + "|" + _param->get("smoother: type", "symmetric Gauss-Seidel") +
                      "|" + _param->get("eigen-analysis: type", "Anorm") + "|" + _param->get("smoother: ifpack type", "ILU");
    char buf[256];
    std::snprintf(buf, sizeof(buf), "|%d|%d|%d|%d|%d|%d|%d|%d|%d|%.17g|%.17g|%.17g|%d|%d|%d|",
                  (int)_param->get("smoother: Gauss-Seidel efficient symmetric", false), _param->get("smoother: sweeps", 1),
                  _param->get("isph: chebyshev value bits", 64), _param->get("isph: amg cycle bits", 64),
                  _param->get("eigen-analysis: iterations", 10), _param->get("max levels", 5), _param->get("coarse: max size", 128),
                  _param->get("isph: block rows", 512), ilist.sublist("smoother: ifpack list").get("fact: level-of-fill", 0),
                  _param->get("aggregation: damping factor", 4.0 / 3.0), _param->get("aggregation: threshold", 0.0),
                  _param->get("smoother: Chebyshev alpha", 20.0), (int)_param->get("isph: amg refresh", false), _null != nullptr ? 1 : 0,
                  _cx != nullptr ? _cdim : 0);
    return sig + buf;
  }
  double *_null = nullptr;
};

}  // namespace LAMMPS_NS
