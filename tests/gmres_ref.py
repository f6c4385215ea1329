"""NumPy restatement of the method behind cs3_gmres (include/csparse3_amd.h): restarted GMRES(restart), right-preconditioned
with any `solve` callable, for ONE system.

Per cycle: r = b - A x, v0 = r (1 / ||r||), then w = A solve(v_j), classical Gram-Schmidt applied twice (the two passes'
coefficients added), Givens rotations, g updated; the system freezes when the recurrence's residual |g_{j+1}| is
<= rtol ||b||, on a lucky breakdown (||w|| == 0) or when it has used max_iters iterations; then x += solve(V y).
Convergence is decided on the TRUE residual at the start of the next cycle.  ||b|| == 0: x = 0, 0 iterations, relres 0.
A non-finite norm or Hessenberg entry: relres NaN, x as the last completed cycle left it."""
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "x iters relres history cycles V ncols", defaults=(None, 0))
# history: |g_{j+1}| / ||b|| after every iteration; cycles: (that estimate at the cycle's end, the true relative residual
# after the cycle's update) per completed cycle; V [n, number of basis vectors built], ncols: the basis and the number of
# Hessenberg columns of the last cycle that ran (keep_basis only)


def _norm(v):
    return float(np.sqrt(np.dot(v, v)))


def gmres(A, solve, b, x0, rtol=1e-12, restart=30, max_iters=100, keep_basis=False):
    b = np.asarray(b, dtype=np.float64)
    x = np.array(x0, dtype=np.float64, copy=True)
    bnorm = _norm(b)
    if bnorm == 0.0:
        return Result(np.zeros_like(x), 0, 0.0, [], [])
    iters, history, cycles, pending = 0, [], [], None
    m = restart
    last = (None, 0)

    def result(relres):
        return Result(x, iters, relres, history, cycles, *last)

    while True:
        r = b - A @ x
        rn = _norm(r)
        if not (np.isfinite(rn) and np.isfinite(bnorm)):
            return result(float("nan"))
        relres = rn / bnorm
        if pending is not None:
            cycles.append((pending, relres))
            pending = None
        if relres <= rtol or iters >= max_iters:
            return result(relres)
        V = [r * (1.0 / rn)]
        R = np.zeros((m, m))
        cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        g[0] = rn
        ncols = 0
        for j in range(m):
            w = A @ solve(V[j])
            h = np.zeros(j + 1)
            for _ in range(2):
                hp = np.array([np.dot(V[i], w) for i in range(j + 1)])
                for i in range(j + 1):
                    w = w - hp[i] * V[i]
                h += hp
            hn = _norm(w)
            if not (np.all(np.isfinite(h)) and np.isfinite(hn)):
                return result(float("nan"))
            prev = h[0]
            for i in range(j):
                nxt = h[i + 1]
                h[i] = cs[i] * prev + sn[i] * nxt
                prev = cs[i] * nxt - sn[i] * prev
            denom = float(np.hypot(prev, hn))
            if denom == 0.0 or not np.isfinite(denom):
                return result(float("nan"))
            cs[j], sn[j] = prev / denom, hn / denom
            h[j] = denom
            R[:j + 1, j] = h
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            iters += 1
            ncols = j + 1
            est = abs(g[j + 1])
            history.append(est / bnorm)
            if est <= rtol * bnorm or hn == 0.0 or iters >= max_iters:
                break
            V.append(w * (1.0 / hn))
        y = np.zeros(ncols)
        for i in range(ncols - 1, -1, -1):
            y[i] = (g[i] - np.dot(R[i, i + 1:ncols], y[i + 1:])) / R[i, i]
        u = np.zeros_like(x)
        for i in range(ncols):
            u += y[i] * V[i]
        x = x + solve(u)
        if keep_basis:
            last = (np.stack(V, axis=1), ncols)
        pending = history[-1]
