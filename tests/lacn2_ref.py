"""NumPy port of LAPACK's dlacn2 (ITMAX = 5), the 1-norm estimator behind dgecon / klu_condest, in the step table the
library's device state machine follows:

    J1  x = A^-1 (1/n) 1   est = ||x||_1 (n = 1: |x_0|, done); s = sign(x)          -> A^-T s
    J2  x = A^-T s         j = first argmax |x_i|; iter = 2                          -> A^-1 e_j
    J3  x = A^-1 e_j       estold = est, est = ||x||_1; sign(x) == s or est <= estold -> final; else s = sign(x), A^-T s
    J4  x = A^-T s         jlast = j, j = first argmax |x_i|; x[jlast] != |x[j]| and iter < 5: iter += 1, A^-1 e_j;
                           else final
    J5  x = A^-1 alt       alt_i = (-1)^i (1 + i / (n - 1)); t = 2 (||x||_1 / (3 n)); est = t if t > est

sign(v) = +1 for v >= 0 (-0.0 included), else -1.  A non-finite entry in a solution ends the estimate at +inf.
lacn2(n, solve, solve_t) -> (est, number of solves); solve(b) = A^-1 b, solve_t(b) = A^-T b.
"""
import numpy as np

ITMAX = 5


def _sign(x):
    return np.where(x >= 0.0, 1.0, -1.0)


def lacn2(n, solve, solve_t):
    if n == 0:
        return 0.0, 0
    count = [0]

    def run(fn, v):
        count[0] += 1
        return np.asarray(fn(np.ascontiguousarray(v, dtype=np.float64)), dtype=np.float64).reshape(-1)

    def finite(x):
        return bool(np.all(np.isfinite(x)))

    x = run(solve, np.full(n, 1.0 / n))                                  # J1
    if not finite(x):
        return np.inf, count[0]
    if n == 1:
        return float(abs(x[0])), count[0]
    est = float(np.abs(x).sum())
    s = _sign(x)
    x = run(solve_t, s)                                                  # J2
    if not finite(x):
        return np.inf, count[0]
    j = int(np.argmax(np.abs(x)))
    it = 2
    while True:
        e = np.zeros(n)
        e[j] = 1.0
        x = run(solve, e)                                                # J3
        if not finite(x):
            return np.inf, count[0]
        estold, est = est, float(np.abs(x).sum())
        sx = _sign(x)
        if np.array_equal(sx, s) or est <= estold:
            break
        s = sx
        x = run(solve_t, s)                                              # J4
        if not finite(x):
            return np.inf, count[0]
        jlast, j = j, int(np.argmax(np.abs(x)))
        if x[jlast] != abs(x[j]) and it < ITMAX:
            it += 1
            continue
        break
    alt = 1.0 + np.arange(n, dtype=np.float64) / (n - 1)                 # J5
    alt[1::2] *= -1.0
    x = run(solve, alt)
    if not finite(x):
        return np.inf, count[0]
    t = 2.0 * (float(np.abs(x).sum()) / (3 * n))
    return (t if t > est else est), count[0]
