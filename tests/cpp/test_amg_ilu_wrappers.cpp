// ML's IFPACK smoother through PrecondWrapper_ML (isph_amg_params::smoother = 4): the keys of sph-script/ml-ifpack.xml set
// by hand --
//   "smoother: type" = "IFPACK", "smoother: ifpack type" = "ILU", "smoother: ifpack overlap" = 0,
//   sublist "smoother: ifpack list" { "fact: level-of-fill" }, "smoother: sweeps", "smoother: pre or post" = "both"
// -- with "coarse: max size" 64 and "isph: block rows" 256, and SolverLin_Belos' default flexible GMRES.
// usage: test_amg_ilu_wrappers in.bin out.bin singular(0/1) fill sweeps [ifpack type] [overlap]
//   in.bin = n, nnz, rp, ci, val, b (test_solver_lin's format); out.bin = x
// Prints "converged=.. iters=.." of the solve.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "precond_ml.h"
#include "solver_lin_hip.h"

using namespace LAMMPS_NS;

#ifdef ISPH_HAVE_MPI
static const MPI_Comm kWorld = MPI_COMM_WORLD;
#else
static const MPI_Comm kWorld = 0;
#endif

static int run(int argc, char **argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: %s in.bin out.bin singular(0/1) fill sweeps [ifpack type] [overlap]\n", argv[0]); return 2; }
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n = 0, nnz = 0;
  if (std::fread(&n, 4, 1, f) != 1 || std::fread(&nnz, 4, 1, f) != 1) return 2;
  std::vector<int> rp((size_t)n + 1), ci((size_t)nnz), gid((size_t)n);
  std::vector<double> val((size_t)nnz), b((size_t)n), x((size_t)n, 0.0);
  if (std::fread(rp.data(), 4, rp.size(), f) != rp.size() || std::fread(ci.data(), 4, ci.size(), f) != ci.size() ||
      std::fread(val.data(), 8, val.size(), f) != val.size() || std::fread(b.data(), 8, b.size(), f) != b.size()) return 2;
  std::fclose(f);
  for (int i = 0; i < n; ++i) gid[(size_t)i] = i + 1;
  const bool singular = std::atoi(argv[3]) != 0;
  const int fill = std::atoi(argv[4]), sweeps = std::atoi(argv[5]);
  const std::string itype = argc > 6 ? argv[6] : "ILU";
  const int overlap = argc > 7 ? std::atoi(argv[7]) : 0;

  MPI_Comm world = kWorld;
  Epetra_Map nodalmap(-1, n, gid.data(), 1, Epetra_MpiComm(world));
  Epetra_CrsMatrix AA(n, n, rp.data(), ci.data(), val.data());
  PrecondWrapper_ML prec(world);
  Teuchos::ParameterList *pp = prec.setParameters();
  pp->set("coarse: max size", 64);
  pp->set("isph: block rows", 256);
  pp->set("smoother: type", "IFPACK");
  pp->set("smoother: ifpack type", itype);
  pp->set("smoother: ifpack overlap", overlap);
  if (pp->isSublist("smoother: ifpack list")) return 2;   // created on first use
  pp->sublist("smoother: ifpack list").set("fact: level-of-fill", fill);
  if (!pp->isSublist("smoother: ifpack list") || pp->sublist("smoother: ifpack list").get("fact: level-of-fill", -1) != fill) return 2;
  pp->set("smoother: sweeps", sweeps);
  pp->set("smoother: pre or post", "both");
  SolverLin_Belos li_solver(world);
  li_solver.setParameters();
  li_solver.setNodalMap(&nodalmap);
  li_solver.createSolutionMultiVector(x.data(), n, 1);
  li_solver.createLoadMultiVector(b.data(), n, 1);
  Epetra_IntSerialDenseVector null_mask(n);
  if (singular) {
    for (int i = 0; i < n; ++i) null_mask[i] = 1;
    li_solver.setNullVectorMask(&null_mask);
    li_solver.setMatrixIsSingular(true);
  }
  li_solver.setMatrix(&AA);
  prec.setMatrix(&AA);
  li_solver.setInitialSolution(SolverLin::Zero);
  if (li_solver.solveProblem(&prec, "amg ifpack smoother") != LAMMPS_SUCCESS) return 1;
  const isph_solve_info &info = li_solver.lastSolveInfo();
  std::printf("converged=%d iters=%d rel=%.3e\n", info.converged, info.iters, info.rel_res_implicit);
  f = std::fopen(argv[2], "wb");
  std::fwrite(x.data(), 8, x.size(), f);
  std::fclose(f);
  return info.converged ? 0 : 3;
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
