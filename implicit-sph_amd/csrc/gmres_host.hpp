// gmres_host.hpp -- the host side of one restarted GMRES solve, block size 1: the Hessenberg matrix rotated in place by
// Givens rotations, the rotated right-hand side g, the back-substitution for y, and the restart rule.  No device code:
// gmres_t, gmres_lockstep_t (solver.hpp) and gcrodr (gcrodr.hpp) fill one column per Arnoldi step and share this
// arithmetic, so a lockstep column carries the bits of its single solve by construction (tests/test_gmres_host.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace isph {

struct GmresCycle {
  int m = 0, j = 0;                     // columns a cycle may take, columns pushed so far
  std::vector<double> H, cs, sn, g, y;  // H: (m+1) x m, column j at H[j*(m+1)]
  double beta = 0.0, scale = 1.0;       // the caller's: residual norm the cycle starts from, |r0| (Belos: zero -> 1)

  void reset(int m_) {
    m = m_; j = 0;
    H.assign((size_t)(m + 1) * (size_t)m, 0.0);
    cs.assign((size_t)m, 0.0); sn.assign((size_t)m, 0.0); g.assign((size_t)m + 1, 0.0); y.assign((size_t)m, 0.0);
  }
  void start() {  // a new cycle: g = beta e_0
    std::fill(g.begin(), g.end(), 0.0);
    g[0] = beta;
    j = 0;
  }
  double *column() { return &H[(size_t)j * (size_t)(m + 1)]; }  // h[0..j+1] of the next column, for the caller to fill
  // applies the earlier rotations to column j, forms the one that removes h[j+1], updates g; returns the recurrence
  // residual |g[j+1]| (not yet divided by scale)
  double push() {
    double *h = column();
    for (int k = 0; k < j; ++k) {
      const double a = cs[k] * h[k] + sn[k] * h[k + 1];
      h[k + 1] = -sn[k] * h[k] + cs[k] * h[k + 1];
      h[k] = a;
    }
    const double a = h[j], bb = h[j + 1], rr = std::hypot(a, bb);
    cs[j] = rr == 0.0 ? 1.0 : a / rr;
    sn[j] = rr == 0.0 ? 0.0 : bb / rr;
    h[j] = rr;
    h[j + 1] = 0.0;
    g[j + 1] = -sn[j] * g[j];
    g[j] = cs[j] * g[j];
    ++j;
    return std::fabs(g[j]);
  }
  const double *solve() {  // y[0..j): R y = g by back-substitution
    for (int k = j - 1; k >= 0; --k) {
      double s = g[k];
      for (int l = k + 1; l < j; ++l) s -= H[(size_t)l * (size_t)(m + 1) + k] * y[l];
      y[k] = s / H[(size_t)k * (size_t)(m + 1) + k];
    }
    return y.data();
  }
};

// The restart rule, once x has been updated at the end of a cycle; Info is isph_solve_info.  With the float basis (f32)
// a recurrence residual <= tol only says "converged": the true residual decides, and forming it counts no restart.
// Returns whether the residual b - Op x is needed; false ends the solve.
template <typename Info>
inline bool gmres_after_update(bool f32, Info &inf, int max_iters, int max_restarts) {
  if (f32 && inf.converged) return true;
  if (inf.converged || inf.iters >= max_iters || inf.restarts >= max_restarts) return false;
  ++inf.restarts;
  return true;
}

// ... and once that residual's norm beta is on the host (f32 && converged still means "to be confirmed": without it
// gmres_after_update only goes on when converged is 0).  Returns whether a new cycle starts from beta.
template <typename Info>
inline bool gmres_after_residual(bool f32, Info &inf, int max_iters, int max_restarts, double beta, double scale, double tol) {
  if (f32 && inf.converged) {
    if (beta / scale <= tol) return false;
    inf.converged = 0;  // restart from this residual
    if (inf.iters >= max_iters || inf.restarts >= max_restarts) return false;
    ++inf.restarts;
    ++inf.residual_restarts;
  }
  if (beta == 0.0) { inf.converged = 1; return false; }
  return true;
}

}  // namespace isph
