// The device-side key "isph: recycle across solves" of SolverLin_Belos (host/solver_lin_hip.h): one solver object,
// "Solver Type" = "Recycling GMRES", solves a list of systems that alternate between two names the way the Helmholtz and
// the Poisson system of a time step alternate through PairISPH's solver, without a preconditioner.
// usage: test_recycle in.bin out.bin key num_blocks num_recycled [again]
//   in.bin  = nsys, then per system: name length, name, singular (int), n, nnz, rp, ci, val, b
//   out.bin = the solutions, one after the other
//   key     = the value of "isph: recycle across solves"; negative: the key is not set
//   again   = index of a system before which setParameters is called once more with the same list (it frees the spaces)
// Prints one line "name=.. converged=.. iters=.. restarts=.." per solve, and at the end one line per name with the
// figures of isph_recycle_info ("recycle name=.. none" when no space is kept for it).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "solver_lin_hip.h"

using namespace LAMMPS_NS;

#ifdef ISPH_HAVE_MPI
static const MPI_Comm kWorld = MPI_COMM_WORLD;
#else
static const MPI_Comm kWorld = 0;
#endif

static int run(int argc, char **argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: %s in.bin out.bin key num_blocks num_recycled\n", argv[0]); return 2; }
  FILE *f = std::fopen(argv[1], "rb");
  FILE *fo = std::fopen(argv[2], "wb");
  if (!f || !fo) return 2;
  const int key = std::atoi(argv[3]), m = std::atoi(argv[4]), k = std::atoi(argv[5]);
  const int again = argc > 6 ? std::atoi(argv[6]) : -1;
  int nsys = 0;
  if (std::fread(&nsys, 4, 1, f) != 1) return 2;

  MPI_Comm world = kWorld;
  SolverLin_Belos li_solver(world);
  Teuchos::ParameterList sp;
  sp.set("Solver Type", "Recycling GMRES");
  sp.set("Num Blocks", m);
  sp.set("Num Recycled Blocks", k);
  if (key >= 0) sp.set("isph: recycle across solves", key);
  li_solver.setParameters(&sp);

  std::vector<std::string> names;
  std::set<std::string> seen;
  // the solver borrows what it is given: every system's objects stay alive until the solver is gone
  std::vector<std::unique_ptr<Epetra_Map>> maps;
  std::vector<std::unique_ptr<Epetra_CrsMatrix>> mats;
  std::vector<std::unique_ptr<Epetra_IntSerialDenseVector>> masks;
  for (int s = 0; s < nsys; ++s) {
    int len = 0, singular = 0, n = 0, nnz = 0;
    if (std::fread(&len, 4, 1, f) != 1 || len < 0 || len > 255) return 2;
    std::string name((size_t)len, ' ');
    if (std::fread(&name[0], 1, (size_t)len, f) != (size_t)len) return 2;
    if (std::fread(&singular, 4, 1, f) != 1 || std::fread(&n, 4, 1, f) != 1 || std::fread(&nnz, 4, 1, f) != 1) return 2;
    std::vector<int> rp((size_t)n + 1), ci((size_t)nnz), gid((size_t)n);
    std::vector<double> val((size_t)nnz), b((size_t)n), x((size_t)n, 0.0);
    if (std::fread(rp.data(), 4, rp.size(), f) != rp.size() || std::fread(ci.data(), 4, ci.size(), f) != ci.size() ||
        std::fread(val.data(), 8, val.size(), f) != val.size() || std::fread(b.data(), 8, b.size(), f) != b.size()) return 2;
    for (int i = 0; i < n; ++i) gid[(size_t)i] = i + 1;
    maps.emplace_back(new Epetra_Map(-1, n, gid.data(), 1, Epetra_MpiComm(world)));
    mats.emplace_back(new Epetra_CrsMatrix(n, n, rp.data(), ci.data(), val.data()));
    masks.emplace_back(new Epetra_IntSerialDenseVector(n));
    Epetra_IntSerialDenseVector &null_mask = *masks.back();
    li_solver.setNodalMap(maps.back().get());
    li_solver.createSolutionMultiVector(x.data(), n, 1);
    li_solver.createLoadMultiVector(b.data(), n, 1);
    for (int i = 0; i < n; ++i) null_mask[i] = 1;
    li_solver.setNullVectorMask(&null_mask);  // read by a singular solve only
    li_solver.setMatrixIsSingular(singular != 0);
    li_solver.setMatrix(mats.back().get());
    li_solver.setInitialSolution(SolverLin::Zero);
    if (s == again) li_solver.setParameters(&sp);
    if (li_solver.solveProblem(NULL, name.c_str()) != LAMMPS_SUCCESS) return 1;
    const isph_solve_info &info = li_solver.lastSolveInfo();
    std::printf("name=%s converged=%d iters=%d restarts=%d\n", name.c_str(), info.converged, info.iters, info.restarts);
    std::fwrite(x.data(), 8, x.size(), fo);
    if (seen.insert(name).second) names.push_back(name);
  }
  std::fclose(f);
  std::fclose(fo);
  for (size_t i = 0; i < names.size(); ++i) {
    long long ri[8];
    if (li_solver.recycleInfo(names[i].c_str(), ri) != ISPH_SUCCESS) std::printf("recycle name=%s none\n", names[i].c_str());
    else
      std::printf("recycle name=%s n=%lld vectors=%lld started=%lld discarded=%lld reason=%lld applications=%lld steps=%lld\n",
                  names[i].c_str(), ri[0], ri[1], ri[2], ri[3], ri[4], ri[5], ri[6]);
  }
  return 0;
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
