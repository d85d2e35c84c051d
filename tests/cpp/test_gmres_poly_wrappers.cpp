// PrecondWrapper_Ifpack's "Precond Type" = "GMRES Polynomial" with "isph: polynomial degree": the GMRES polynomial in
// D^-1 A behind the wrapper, the null vector of a singular system passed on (setNullVector).
// usage: test_gmres_poly_wrappers in.bin out.bin singular(0/1) mode
//   in.bin = n, nnz, rp, ci, val, b (test_solver_lin's format); out.bin = x
//   mode: default (the key is not set: degree 4) | degree<d> ("isph: polynomial degree" = d, 26 is refused by the library)
// Prints "converged=.. iters=.." of the solve.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "precond_ifpack.h"
#include "solver_lin_hip.h"

using namespace LAMMPS_NS;

#ifdef ISPH_HAVE_MPI
static const MPI_Comm kWorld = MPI_COMM_WORLD;
#else
static const MPI_Comm kWorld = 0;
#endif

static int run(int argc, char **argv) {
  if (argc < 5) { std::fprintf(stderr, "usage: %s in.bin out.bin singular(0/1) mode\n", argv[0]); return 2; }
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
  const std::string mode = argv[4];

  MPI_Comm world = kWorld;
  Epetra_Map nodalmap(-1, n, gid.data(), 1, Epetra_MpiComm(world));
  Epetra_CrsMatrix AA(n, n, rp.data(), ci.data(), val.data());
  PrecondWrapper_Ifpack prec(world);
  Teuchos::ParameterList *pp = prec.setParameters();
  pp->set("Precond Type", "GMRES Polynomial");
  if (mode.compare(0, 6, "degree") == 0) pp->set("isph: polynomial degree", std::atoi(mode.c_str() + 6));
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
  if (li_solver.solveProblem(&prec, "GMRES polynomial wrapper") != LAMMPS_SUCCESS) {
    std::fprintf(stderr, "%s\n", isph_last_error());
    return 1;
  }
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
