// Host-only check of csrc/gmres_host.hpp (the Hessenberg / Givens state of a GMRES cycle and the restart rule): reads
// commands from stdin, prints what the header computes.  Driven by tests/test_gmres_host.py against numpy.
//   H m beta, then the (m+1) x m matrix row by row: pushes its columns one at a time and prints after each push
//     "residual cs sn g[j] g[j+1]" and y[0..j+1) on a second line
//   U f32 converged iters restarts residual_restarts max_iters max_restarts: gmres_after_update
//   R f32 converged iters restarts residual_restarts max_iters max_restarts beta scale tol: gmres_after_residual
//     both print "decision converged iters restarts residual_restarts"
#include <cstdio>
#include <vector>

#include "gmres_host.hpp"

struct Info { int converged, iters, restarts, residual_restarts; };

int main() {
  char cmd = 0;
  while (std::scanf(" %c", &cmd) == 1) {
    if (cmd == 'H') {
      int m = 0;
      isph::GmresCycle c;
      if (std::scanf("%d %lf", &m, &c.beta) != 2 || m < 1) return 2;
      std::vector<double> A((size_t)(m + 1) * m);
      for (auto &v : A) if (std::scanf("%lf", &v) != 1) return 2;
      c.reset(m);
      c.start();
      for (int j = 0; j < m; ++j) {
        double *h = c.column();
        for (int i = 0; i <= j + 1; ++i) h[i] = A[(size_t)i * m + j];
        const double res = c.push();
        std::printf("%.17g %.17g %.17g %.17g %.17g\n", res, c.cs[j], c.sn[j], c.g[j], c.g[j + 1]);
        const double *y = c.solve();
        for (int i = 0; i <= j; ++i) std::printf("%.17g ", y[i]);
        std::printf("\n");
      }
    } else if (cmd == 'U' || cmd == 'R') {
      int f32 = 0, max_iters = 0, max_restarts = 0;
      Info inf;
      if (std::scanf("%d %d %d %d %d %d %d", &f32, &inf.converged, &inf.iters, &inf.restarts, &inf.residual_restarts, &max_iters,
                     &max_restarts) != 7) return 2;
      bool go;
      if (cmd == 'U') {
        go = isph::gmres_after_update(f32 != 0, inf, max_iters, max_restarts);
      } else {
        double beta = 0.0, scale = 1.0, tol = 0.0;
        if (std::scanf("%lf %lf %lf", &beta, &scale, &tol) != 3) return 2;
        go = isph::gmres_after_residual(f32 != 0, inf, max_iters, max_restarts, beta, scale, tol);
      }
      std::printf("%d %d %d %d %d\n", go ? 1 : 0, inf.converged, inf.iters, inf.restarts, inf.residual_restarts);
    } else {
      return 2;
    }
  }
  return 0;
}
