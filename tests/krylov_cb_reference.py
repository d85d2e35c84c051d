"""Plain numpy restatement of restarted GMRES(m) with the Krylov basis stored in single precision -- the compressed
basis of isph_solver_params::basis_bits = 32 (host only, not a test module).  Nothing here shares code with the device.

Rounding points (bits = 32), as include/isph_hip.h states them: v_0 = fl32(r * (1 / beta)) and
v_{j+1} = fl32(w_final * (1 / |w_final|)), numpy's astype(float32) (round to nearest even, subnormals kept).  Every
stored vector is widened to float64 wherever it is read; the preconditioner and the operator get the widened rounded
vector.  Z, w, x, b, the dots, the norms, the Hessenberg matrix and the Givens rotations are float64.  With bits = 64
nothing is rounded and the iterates are those of krylov_reference.gmres_iterates.

Two things of the device are mirrored because they are not negligible once V^T V = I + O(6e-8):
  * the orthogonalisation variant: ICGS always makes two classical Gram-Schmidt passes, DGKS the second one only when
    |w_new| < |w_old| / sqrt(2); the pass ratios |w_new| / |w_old| are kept per step (Result.ratios);
  * the norm of the final vector: the float path of the device keeps the formula of the fp64 path, so it is restated,
    not replaced by a direct norm: |w_final|^2 = |w_new|^2 - |c2|^2 after a second pass (c2 = V^T w_new), |w_new|^2
    without one.
The singular form is the explicit projection: b <- b - (b.n) n, operator P A with P = I - n n^T in float64 (the null
vector is never rounded), x <- x - (x.n) n at the end.

Convergence (tol > 0): when the recurrence residual reaches tol the cycle ends and x is updated.  bits = 32 with
confirm=True then computes the true residual |b - Op(x)| / scale (what a restart computes): <= tol is convergence,
otherwise the method restarts from that residual (restarts and residual_restarts both count it).  confirm=False is the
recurrence test alone.
"""
import numpy as np

import krylov_reference as kr

DGKS, ICGS = 0, 1


def rnd(v, bits):
    """the stored form of a basis vector, widened again"""
    v = np.asarray(v, dtype=np.float64)
    return v.astype(np.float32).astype(np.float64) if bits == 32 else v.copy()


class Cycle:
    """one restart cycle: V[(j+1) x n] stored basis (widened), Z[j x n], H[(j+1) x j] the raw Hessenberg matrix,
    AZ[j x n] the operator applied to Z"""

    def __init__(self, V, Z, H, AZ):
        self.V, self.Z, self.H, self.AZ = V, Z, H, AZ


class Result:
    def __init__(self):
        self.x = None
        self.iters = self.restarts = self.residual_restarts = self.reorth = self.converged = 0
        self.rec_res = np.inf        # recurrence residual / scale after the last iteration
        self.true_res = np.inf       # |P(b - A x)| / scale of the returned x (longdouble accumulation)
        self.ratios = []             # per step: |w| after / before the first Gram-Schmidt pass
        self.iterates = {}           # k -> Snapshot
        self.cycles = []
        self.confirmations = []      # true residual / scale of every confirmation (bits = 32, confirm=True)

    def dgks_margin(self):
        r = np.asarray(self.ratios)
        return float(np.min(np.abs(r / kr.DGKS_TOL - 1.0))) if len(r) else np.inf


class Snapshot:
    """x: the k-th iterate (projected when singular); rel_res: its true residual / scale; rec_res: the recurrence
    residual / scale at that iteration; restarts, reorth: the counters after k iterations; margin: smallest relative
    distance of a first-pass ratio to the DGKS threshold so far"""

    def __init__(self, x, rel_res, rec_res, restarts, reorth, margin):
        self.x, self.rel_res, self.rec_res, self.restarts, self.reorth, self.margin = x, rel_res, rec_res, restarts, reorth, margin


def gmres_cb(A, b, x0, m, bits, ortho=DGKS, Minv=None, null=None, flexible=True, tol=0.0, max_iters=500,
             max_restarts=10 ** 6, confirm=True, ks=(), keep_cycles=False):
    assert bits in (32, 64) and ortho in (DGKS, ICGS)
    A = kr.as_csr(A)
    n = A.shape[0]
    Minv = Minv or (lambda r: r.copy())
    b = kr._proj(np.asarray(b, dtype=np.float64), null)
    x = np.array(x0, dtype=np.float64)
    ks = set(int(k) for k in ks)
    res = Result()

    def op(v):
        return kr._proj(A @ v, null)

    r = b - op(x)
    beta = float(np.sqrt(r @ r))
    scale = beta if beta > 0.0 else 1.0
    res.rec_res = beta / scale
    res.converged = int(beta / scale <= tol)

    def margin():
        return res.dgks_margin()

    def snapshot(k, xk, rec):
        res.iterates[k] = Snapshot(kr._proj(xk, null), kr.true_residual_norm(A, b, xk, null) / scale, rec, res.restarts,
                                   res.reorth, margin())

    while not res.converged and res.iters < max_iters:
        V = np.zeros((m + 1, n))
        Z = np.zeros((m, n))
        AZ = np.zeros((m, n))
        Hraw = np.zeros((m + 1, m))
        R = np.zeros((m + 1, m))      # the Hessenberg matrix under the Givens rotations
        cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        V[0] = rnd(r * (1.0 / beta), bits)
        g[0] = beta
        j = 0

        def update(jj):
            y = np.zeros(jj)
            for k in range(jj - 1, -1, -1):
                y[k] = (g[k] - R[k, k + 1:jj] @ y[k + 1:jj]) / R[k, k]
            if flexible:
                return x + Z[:jj].T @ y
            return x + Minv(V[:jj].T @ y)

        while j < m:
            Z[j] = Minv(V[j])
            w = op(Z[j])
            AZ[j] = w
            Vj = V[:j + 1]
            ww_old = w @ w
            c1 = Vj @ w
            w = w - Vj.T @ c1
            ww_new = w @ w
            c2 = Vj @ w
            ratio = np.sqrt(ww_new) / np.sqrt(ww_old) if ww_old > 0 else 0.0
            res.ratios.append(ratio)
            second = ortho == ICGS or np.sqrt(ww_new) < kr.DGKS_TOL * np.sqrt(ww_old)
            h = c1.copy()
            if second:
                w = w - Vj.T @ c2
                h += c2
                wf2 = max(ww_new - c2 @ c2, 0.0)
                res.reorth += 1
            else:
                wf2 = ww_new
            hn = np.sqrt(wf2)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                V[j + 1] = rnd(w * (1.0 / np.sqrt(wf2)), bits)
            Hraw[:j + 1, j] = h
            Hraw[j + 1, j] = hn
            col = np.append(h, hn)
            for k in range(j):
                a = cs[k] * col[k] + sn[k] * col[k + 1]
                col[k + 1] = -sn[k] * col[k] + cs[k] * col[k + 1]
                col[k] = a
            rr = np.hypot(col[j], col[j + 1])
            cs[j] = 1.0 if rr == 0.0 else col[j] / rr
            sn[j] = 0.0 if rr == 0.0 else col[j + 1] / rr
            col[j], col[j + 1] = rr, 0.0
            R[:j + 2, j] = col
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            j += 1
            res.iters += 1
            res.rec_res = abs(g[j]) / scale
            if res.rec_res <= tol:
                res.converged = 1
                break
            if res.iters >= max_iters:
                break
            if res.iters in ks and j < m:
                snapshot(res.iters, update(j), res.rec_res)
        x = update(j)
        if keep_cycles:
            res.cycles.append(Cycle(V[:j + 1].copy(), Z[:j].copy(), Hraw[:j + 1, :j].copy(), AZ[:j].copy()))
        if res.iters in ks and res.iters not in res.iterates:
            snapshot(res.iters, x, res.rec_res)
        check = bits == 32 and confirm and res.converged
        if not check:
            if res.converged or res.iters >= max_iters or res.restarts >= max_restarts:
                break
            res.restarts += 1
        r = b - op(x)
        beta = float(np.sqrt(r @ r))
        if check:
            res.confirmations.append(beta / scale)
            if beta / scale <= tol:
                break
            res.converged = 0
            if res.iters >= max_iters or res.restarts >= max_restarts:
                break
            res.restarts += 1
            res.residual_restarts += 1
        if beta == 0.0:
            res.converged = 1
            break
    res.true_res = kr.true_residual_norm(A, b, x, null) / scale
    res.x = kr._proj(x, null)
    for k in ks:   # the method ended before k: the later iterates are the last one
        if k not in res.iterates:
            res.iterates[k] = Snapshot(res.x, res.true_res, res.rec_res, res.restarts, res.reorth, margin())
    return res


def iterates(A, b, x0, ks, m, bits, ortho=DGKS, Minv=None, null=None, flexible=True):
    """{k: Snapshot} of the k-th iterates (tol = 0), k iterations in total, restarts included"""
    ks = sorted(set(int(k) for k in ks))
    return gmres_cb(A, b, x0, m, bits, ortho, Minv, null, flexible, tol=0.0, max_iters=ks[-1], ks=ks).iterates


def arnoldi_defects(cycle):
    """per column j of a cycle: (|Op Z_j - V_{j+1} Hbar_j|, |h_{j+1,j}| |v_{j+1}|)"""
    out = []
    for j in range(cycle.Z.shape[0]):
        d = cycle.AZ[j] - cycle.V[:j + 2].T @ cycle.H[:j + 2, j]
        out.append((float(np.linalg.norm(d)), float(abs(cycle.H[j + 1, j]) * np.linalg.norm(cycle.V[j + 1]))))
    return out
