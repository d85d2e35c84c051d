// SolverLin_HIP::holdPattern with PrecondWrapper_Ifpack and PrecondWrapper_ML (host/*.h), driven the way the adapter
// would: ONE Epetra matrix whose value array is refilled between solveProblem calls.
// usage: test_pattern_hold_wrappers in.bin out.bin fill coords(0/1) move_row
//   in.bin  = n, nnz, rp, ci, val[3][nnz], b[3][n], x[n], y[n] (coordinates of the rows)
//   out.bin = the solutions, n doubles each, in the order of the printed "call" lines
//   fill: "fact: level-of-fill"; coords: 1 = prec.setCoordinates (the library's bricks), 0 = "isph: block rows" = 256;
//   move_row: a row whose last entry may move to the front of the next row (the test picked it): rowptr[move_row + 1]
//   is lowered by one IN PLACE for one call -- same pointers, same counts, another pattern
// One solver object runs, in this order:
//   plain   three solves, one per value set, without hold
//   held    holdPattern(true), the same three solves
//   moved   a fourth solve under hold with the changed row pointer (and the values of set 0)
//   then holdPattern(false), and the pool must be back at its size after "plain"
//   mlplain / mlheld   two solves each with PrecondWrapper_ML on the same solver object
// Every solve prints "call seq=<name> k=<call> converged=.. iters=.. link_bytes=.."; the pool line is "pool before=.. after=..".
//
// usage: test_pattern_hold_wrappers in.bin coords.bin timed repeat          (scripts/time_pattern_hold.py)
//   in.bin = n, nnz, rp, ci, val, b (test_solver_lin's format, singular system); coords.bin = x[n], y[n], z[n]
//   "bjacobi-ilu0" on the library's bricks (setCoordinates).  Per repetition, in ONE process: a solve without hold; then
//   holdPattern(true), a first solve (full ingress + the entry map), a second solve (value update + refactor),
//   holdPattern(false).  Prints one line per kind with the median (min - max) of ingress / set-up / Krylov / wall ms.
#include <algorithm>
#include <chrono>
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

static long long pool_live() {
  long long info[4] = {0, 0, 0, 0};
  isph_pool_info(info, 0);
  return info[1];
}

static std::string spread(std::vector<double> t) {
  std::sort(t.begin(), t.end());
  char buf[96];
  std::snprintf(buf, sizeof(buf), "%.2f (%.2f - %.2f)", t[t.size() / 2], t.front(), t.back());
  return buf;
}

static int run_timed(int argc, char **argv) {
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n = 0, nnz = 0;
  if (std::fread(&n, 4, 1, f) != 1 || std::fread(&nnz, 4, 1, f) != 1) return 2;
  std::vector<int> rp((size_t)n + 1), ci((size_t)nnz), gid((size_t)n);
  std::vector<double> val((size_t)nnz), b0((size_t)n), x((size_t)n, 0.0), coords((size_t)3 * n);
  if (std::fread(rp.data(), 4, rp.size(), f) != rp.size() || std::fread(ci.data(), 4, ci.size(), f) != ci.size() ||
      std::fread(val.data(), 8, val.size(), f) != val.size() || std::fread(b0.data(), 8, b0.size(), f) != b0.size()) return 2;
  std::fclose(f);
  f = std::fopen(argv[2], "rb");
  if (!f || std::fread(coords.data(), 8, coords.size(), f) != coords.size()) return 2;
  std::fclose(f);
  const int repeat = argc > 4 ? std::atoi(argv[4]) : 5;
  for (int i = 0; i < n; ++i) gid[(size_t)i] = i + 1;
  std::vector<double> b = b0;
  MPI_Comm world = kWorld;
  Epetra_Map nodalmap(-1, n, gid.data(), 1, Epetra_MpiComm(world));
  Epetra_CrsMatrix AA(n, n, rp.data(), ci.data(), val.data());
  PrecondWrapper_Ifpack prec(world);
  Teuchos::ParameterList *pp = prec.setParameters();
  pp->set("fact: level-of-fill", 0);
  pp->set("Overlap Level", 0);
  pp->set("isph: block rows", 512);
  prec.setCoordinates(3, coords.data(), coords.data() + n, coords.data() + 2 * (size_t)n);
  SolverLin_Belos li_solver(world);
  li_solver.setParameters();
  li_solver.setNodalMap(&nodalmap);
  li_solver.createSolutionMultiVector(x.data(), n, 1);
  li_solver.createLoadMultiVector(b.data(), n, 1);
  Epetra_IntSerialDenseVector null_mask(n);
  for (int i = 0; i < n; ++i) null_mask[i] = 1;
  li_solver.setNullVectorMask(&null_mask);
  li_solver.setMatrixIsSingular(true);
  li_solver.setTiming(true);
  const char *kinds[3] = {"full ingress + create (no hold)", "first held solve (full ingress + map + create)",
                          "held solve (value update + refactor)"};
  std::vector<double> t[3][5];
  double bytes[3] = {0, 0, 0};
  int iters[3] = {0, 0, 0}, conv = 1;
  auto one = [&](int kind, bool record) -> int {
    b = b0;
    li_solver.setMatrix(&AA);
    prec.setMatrix(&AA);
    li_solver.setInitialSolution(SolverLin::Zero);
    const std::chrono::steady_clock::time_point w0 = std::chrono::steady_clock::now();
    if (li_solver.solveProblem(&prec, NULL) != LAMMPS_SUCCESS) return 1;
    const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    if (!record) return 0;
    const double *ms = li_solver.lastTimingsMs();
    for (int q = 0; q < 4; ++q) t[kind][q].push_back(ms[q]);
    t[kind][4].push_back(wall);
    double gi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    li_solver.lastIngressInfo(gi);
    bytes[kind] = gi[6];
    iters[kind] = li_solver.lastSolveInfo().iters;
    conv = conv && li_solver.lastSolveInfo().converged;
    return 0;
  };
  for (int k = 0; k < repeat + 1; ++k) {   // the first round creates the context, the pinned ring and the device pool
    if (one(0, k > 0)) return 1;
    li_solver.holdPattern(true);
    if (one(1, k > 0) || one(2, k > 0)) return 1;
    li_solver.holdPattern(false);
  }
  std::printf("rows %d entries %d repetitions %d converged %d\n", n, nnz, repeat, conv);
  for (int kind = 0; kind < 3; ++kind)
    std::printf("%-48s iterations %3d  link bytes %12.0f  ms: ingress %s  set-up %s  Krylov %s  release %s  wall %s\n", kinds[kind],
                iters[kind], bytes[kind], spread(t[kind][0]).c_str(), spread(t[kind][1]).c_str(), spread(t[kind][2]).c_str(),
                spread(t[kind][3]).c_str(), spread(t[kind][4]).c_str());
  std::printf("entry map bytes %.0f\n", 4.0 * nnz);
  return conv ? 0 : 3;
}

static int run(int argc, char **argv) {
  if (argc > 3 && std::string(argv[3]) == "timed") return run_timed(argc, argv);
  if (argc < 6) { std::fprintf(stderr, "usage: %s in.bin out.bin fill coords(0/1) move_row\n", argv[0]); return 2; }
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n = 0, nnz = 0;
  if (std::fread(&n, 4, 1, f) != 1 || std::fread(&nnz, 4, 1, f) != 1) return 2;
  std::vector<int> rp((size_t)n + 1), ci((size_t)nnz), gid((size_t)n);
  std::vector<double> vals((size_t)3 * nnz), bs((size_t)3 * n), cx((size_t)n), cy((size_t)n);
  if (std::fread(rp.data(), 4, rp.size(), f) != rp.size() || std::fread(ci.data(), 4, ci.size(), f) != ci.size() ||
      std::fread(vals.data(), 8, vals.size(), f) != vals.size() || std::fread(bs.data(), 8, bs.size(), f) != bs.size() ||
      std::fread(cx.data(), 8, cx.size(), f) != cx.size() || std::fread(cy.data(), 8, cy.size(), f) != cy.size()) return 2;
  std::fclose(f);
  for (int i = 0; i < n; ++i) gid[(size_t)i] = i + 1;
  const int fill = std::atoi(argv[3]);
  const bool coords = std::atoi(argv[4]) != 0;
  const int move_row = std::atoi(argv[5]);
  std::vector<double> val((size_t)nnz), b((size_t)n), x((size_t)n, 0.0);   // what the adapter refills

  MPI_Comm world = kWorld;
  Epetra_Map nodalmap(-1, n, gid.data(), 1, Epetra_MpiComm(world));
  Epetra_CrsMatrix AA(n, n, rp.data(), ci.data(), val.data());
  PrecondWrapper_Ifpack ifpack(world);
  Teuchos::ParameterList *pp = ifpack.setParameters();
  pp->set("Precond Type", "ILU");
  pp->set("fact: level-of-fill", fill);
  pp->set("isph: block rows", 256);
  if (coords) ifpack.setCoordinates(2, cx.data(), cy.data(), NULL);
  PrecondWrapper_ML ml(world);
  Teuchos::ParameterList *pm = ml.setParameters();
  pm->set("coarse: max size", 64);
  pm->set("isph: block rows", 256);
  SolverLin_Belos li_solver(world);
  li_solver.setParameters();
  li_solver.setNodalMap(&nodalmap);
  li_solver.createSolutionMultiVector(x.data(), n, 1);
  li_solver.createLoadMultiVector(b.data(), n, 1);
  li_solver.setMatrix(&AA);
  ifpack.setMatrix(&AA);
  ml.setMatrix(&AA);
  li_solver.setInitialSolution(SolverLin::Zero);

  FILE *out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  int bad = 0;
  auto solve = [&](PrecondWrapper *prec, const char *seq, int k, int set) {
    std::memcpy(val.data(), vals.data() + (size_t)set * nnz, sizeof(double) * (size_t)nnz);
    std::memcpy(b.data(), bs.data() + (size_t)set * n, sizeof(double) * (size_t)n);
    std::fill(x.begin(), x.end(), 0.0);
    if (li_solver.solveProblem(prec, seq) != LAMMPS_SUCCESS) { ++bad; return; }
    const isph_solve_info &info = li_solver.lastSolveInfo();
    double ing[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    li_solver.lastIngressInfo(ing);
    std::printf("call seq=%s k=%d converged=%d iters=%d link_bytes=%.0f\n", seq, k, info.converged, info.iters, ing[6]);
    std::fwrite(x.data(), 8, x.size(), out);
  };
  for (int k = 0; k < 3; ++k) solve(&ifpack, "plain", k, k);
  const long long before = pool_live();
  li_solver.holdPattern(true);
  for (int k = 0; k < 3; ++k) solve(&ifpack, "held", k, k);
  rp[(size_t)move_row + 1] -= 1;            // the last entry of move_row now opens the next row
  solve(&ifpack, "moved", 0, 0);
  rp[(size_t)move_row + 1] += 1;
  li_solver.holdPattern(false);
  std::printf("pool before=%lld after=%lld\n", before, pool_live());
  for (int k = 0; k < 2; ++k) solve(&ml, "mlplain", k, k);
  li_solver.holdPattern(true);
  for (int k = 0; k < 2; ++k) solve(&ml, "mlheld", k, k);
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
