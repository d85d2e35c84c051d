// SolverLin_HIP::holdPattern with PrecondWrapper_ML ("isph: amg refresh") and PrecondWrapper_Ifpack ("Precond Type" =
// "Chebyshev") (host/*.h): the device object of the first held solve is kept and refreshed by isph_prec_refactor on the
// values of the next one.  ONE Epetra matrix whose value array is refilled between solveProblem calls, as the adapter does.
// usage: test_amg_refresh_wrappers in.bin out.bin
//   in.bin  = n, nnz, rp, ci, val[2][nnz], b[2][n]
//   out.bin = the solutions, n doubles each, in the order of the printed "call" lines
// One solver object runs, per wrapper (ml: a null vector set, "coarse: max size" 64; cheb: degree 3), two solves without
// hold ("<w>plain"), then holdPattern(true), the same two solves ("<w>held"), holdPattern(false); then "mlchanged": two held
// solves of the ML wrapper with "smoother: sweeps" changed in between (the kept hierarchy must be built anew).
// Every solve prints "call seq=<name> k=<call> converged=.. iters=.. refreshes=.." (refreshes: isph_prec_amg_refreshes of
// the wrapper's device object after the solve, -1 when it has none).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "precond_ifpack.h"
#include "precond_ml.h"
#include "solver_lin_hip.h"

using namespace LAMMPS_NS;

#ifdef ISPH_HAVE_MPI
static const MPI_Comm kWorld = MPI_COMM_WORLD;
#else
static const MPI_Comm kWorld = 0;
#endif

struct MLProbe : PrecondWrapper_ML {
  MLProbe(MPI_Comm c) : PrecondWrapper_ML(c) {}
  long long refreshes() const { return _M ? isph_prec_amg_refreshes(_M) : -1; }
};
struct ChebProbe : PrecondWrapper_Ifpack {
  ChebProbe(MPI_Comm c) : PrecondWrapper_Ifpack(c) {}
  long long refreshes() const { return _M ? 0 : -1; }
};

static int run(int argc, char **argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n = 0, nnz = 0;
  if (std::fread(&n, 4, 1, f) != 1 || std::fread(&nnz, 4, 1, f) != 1) return 2;
  std::vector<int> rp((size_t)n + 1), ci((size_t)nnz), gid((size_t)n);
  std::vector<double> vals((size_t)2 * nnz), bs((size_t)2 * n);
  if (std::fread(rp.data(), 4, rp.size(), f) != rp.size() || std::fread(ci.data(), 4, ci.size(), f) != ci.size() ||
      std::fread(vals.data(), 8, vals.size(), f) != vals.size() || std::fread(bs.data(), 8, bs.size(), f) != bs.size()) return 2;
  std::fclose(f);
  for (int i = 0; i < n; ++i) gid[(size_t)i] = i + 1;
  std::vector<double> val((size_t)nnz), b((size_t)n), x((size_t)n, 0.0), nv((size_t)n, 1.0);   // what the adapter refills

  MPI_Comm world = kWorld;
  Epetra_Map nodalmap(-1, n, gid.data(), 1, Epetra_MpiComm(world));
  Epetra_CrsMatrix AA(n, n, rp.data(), ci.data(), val.data());
  MLProbe ml(world);
  Teuchos::ParameterList *pm = ml.setParameters();
  pm->set("coarse: max size", 64);
  pm->set("isph: block rows", 256);
  pm->set("isph: amg refresh", true);
  ml.setNullVector(nv.data());
  ChebProbe cheb(world);
  Teuchos::ParameterList *pc = cheb.setParameters();
  pc->set("Precond Type", "Chebyshev");
  pc->set("chebyshev: degree", 3);
  SolverLin_Belos li_solver(world);
  li_solver.setParameters();
  li_solver.setNodalMap(&nodalmap);
  li_solver.createSolutionMultiVector(x.data(), n, 1);
  li_solver.createLoadMultiVector(b.data(), n, 1);
  li_solver.setMatrix(&AA);
  ml.setMatrix(&AA);
  cheb.setMatrix(&AA);
  li_solver.setInitialSolution(SolverLin::Zero);

  FILE *out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  int bad = 0;
  auto solve = [&](PrecondWrapper *prec, long long (*count)(void *), void *who, const char *seq, int k, int set) {
    std::memcpy(val.data(), vals.data() + (size_t)set * nnz, sizeof(double) * (size_t)nnz);
    std::memcpy(b.data(), bs.data() + (size_t)set * n, sizeof(double) * (size_t)n);
    std::fill(x.begin(), x.end(), 0.0);
    if (li_solver.solveProblem(prec, seq) != LAMMPS_SUCCESS) { ++bad; return; }
    const isph_solve_info &info = li_solver.lastSolveInfo();
    std::printf("call seq=%s k=%d converged=%d iters=%d refreshes=%lld\n", seq, k, info.converged, info.iters, count(who));
    std::fwrite(x.data(), 8, x.size(), out);
  };
  auto ml_count = [](void *w) { return static_cast<MLProbe *>(w)->refreshes(); };
  auto cheb_count = [](void *w) { return static_cast<ChebProbe *>(w)->refreshes(); };
  for (int k = 0; k < 2; ++k) solve(&ml, ml_count, &ml, "mlplain", k, k);
  li_solver.holdPattern(true);
  for (int k = 0; k < 2; ++k) solve(&ml, ml_count, &ml, "mlheld", k, k);
  li_solver.holdPattern(false);
  for (int k = 0; k < 2; ++k) solve(&cheb, cheb_count, &cheb, "chebplain", k, k);
  li_solver.holdPattern(true);
  for (int k = 0; k < 2; ++k) solve(&cheb, cheb_count, &cheb, "chebheld", k, k);
  li_solver.holdPattern(false);
  li_solver.holdPattern(true);
  solve(&ml, ml_count, &ml, "mlchanged", 0, 0);
  pm->set("smoother: sweeps", 2);
  solve(&ml, ml_count, &ml, "mlchanged", 1, 1);
  li_solver.holdPattern(false);
  std::fclose(out);
  return bad ? 1 : 0;
}

int main(int argc, char **argv) {
#ifdef ISPH_HAVE_MPI
  MPI_Init(&argc, &argv);
  const int rc = run(argc, argv);
  MPI_Finalize();
  return rc;
#else
  return run(argc, argv);
#endif
}
