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
lacn2_traced: the same with a record of the path, the exits, the ties and the margins, and the edge suite's mutants.
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


def lacn2_traced(n, solve, solve_t, itmax=ITMAX, last_argmax=False, strict_growth=False, drop_j5=False, iter0=2):
    """lacn2 with a record of what it did: -> (est, number of solves, trace).  With the defaults est and the number of
    solves are lacn2's, bit for bit.  The keywords are the mutants of the edge suite: another iteration cap, the LAST
    index of the largest |x_i| at J2 / J4, `<` for `<=` in the no-growth test of J3, no J5, another start of `iter`.

    trace: path      [("J1",), ("J2", j), ("J3",), ("J4", j), ..., ("J5",)]
           j3_exit   None (the loop ended at J4), "same_signs" or "no_growth" (the signs differed and est <= estold)
           j4_exit   None, "repeat" (x[jlast] == max |x_i|) or "cap" (iter reached the cap)
           j5_won    t > est
           ties      [(index into path, the indices that share the largest |x_i|)] at J2 / J4, where more than one, and
                     (index into path, "est") at a J3 with est == estold exactly; ties do not enter `margin`
           amax      the largest |x_i| at every J2 / J4
           sign_diff per J3: the indices where sign(x) != s
           est_j3    the estimate after every J3
           t         J5's alternative estimate (None where J5 did not run)
           margin    the smallest relative margin of all decisions: |est - estold| / max at J3; |x[jlast] - max| / max and
                     (max - second) / max at J2 / J4; |t - est| / max at J5; min |x_i| / max |x| over the nonzero entries
                     whenever sign(x) is taken or compared (J1, J3)
           nonfinite the estimate ended at +inf"""
    tr = dict(path=[], j3_exit=None, j4_exit=None, j5_won=False, ties=[], amax=[], sign_diff=[], est_j3=[], t=None, margin=np.inf,
              nonfinite=False)
    if n == 0:
        return 0.0, 0, tr
    count = [0]

    def run(fn, v):
        count[0] += 1
        return np.asarray(fn(np.ascontiguousarray(v, dtype=np.float64)), dtype=np.float64).reshape(-1)

    def finite(x):
        ok = bool(np.all(np.isfinite(x)))
        tr["nonfinite"] = not ok
        return ok

    def margin(m):
        tr["margin"] = min(tr["margin"], float(m))

    def sign_margin(x):
        a = np.abs(x)
        nz = a[a > 0.0]
        if len(nz):
            margin(nz.min() / a.max())

    def argmax(x):
        a = np.abs(x)
        top = np.flatnonzero(a == a.max())
        tr["amax"].append(float(a.max()))
        if len(top) > 1:
            tr["ties"].append((len(tr["path"]), [int(i) for i in top]))
        elif n > 1 and a.max() > 0.0:
            margin((a.max() - np.partition(a, -2)[-2]) / a.max())
        return int(top[-1] if last_argmax else top[0])

    x = run(solve, np.full(n, 1.0 / n))                                  # J1
    tr["path"].append(("J1",))
    if not finite(x):
        return np.inf, count[0], tr
    if n == 1:
        return float(abs(x[0])), count[0], tr
    est = float(np.abs(x).sum())
    s = _sign(x)
    sign_margin(x)
    x = run(solve_t, s)                                                  # J2
    if not finite(x):
        tr["path"].append(("J2", None))
        return np.inf, count[0], tr
    j = argmax(x)
    tr["path"].append(("J2", j))
    it = iter0
    while True:
        e = np.zeros(n)
        e[j] = 1.0
        x = run(solve, e)                                                # J3
        tr["path"].append(("J3",))
        if not finite(x):
            return np.inf, count[0], tr
        estold, est = est, float(np.abs(x).sum())
        tr["est_j3"].append(est)
        if est == estold:
            tr["ties"].append((len(tr["path"]) - 1, "est"))
        else:
            margin(abs(est - estold) / max(est, estold))
        sx = _sign(x)
        sign_margin(x)
        diff = np.flatnonzero(sx != s)
        tr["sign_diff"].append([int(i) for i in diff])
        if len(diff) == 0:
            tr["j3_exit"] = "same_signs"
            break
        if (est < estold) if strict_growth else (est <= estold):
            tr["j3_exit"] = "no_growth"
            break
        s = sx
        x = run(solve_t, s)                                              # J4
        if not finite(x):
            tr["path"].append(("J4", None))
            return np.inf, count[0], tr
        jlast, j = j, argmax(x)
        tr["path"].append(("J4", j))
        mx = abs(x[j])
        margin(abs(x[jlast] - mx) / mx if x[jlast] != mx else np.inf)
        if x[jlast] == mx:
            tr["j4_exit"] = "repeat"
            break
        if it >= itmax:
            tr["j4_exit"] = "cap"
            break
        it += 1
    if drop_j5:
        return est, count[0], tr
    alt = 1.0 + np.arange(n, dtype=np.float64) / (n - 1)                 # J5
    alt[1::2] *= -1.0
    x = run(solve, alt)
    tr["path"].append(("J5",))
    if not finite(x):
        return np.inf, count[0], tr
    t = 2.0 * (float(np.abs(x).sum()) / (3 * n))
    tr["t"] = t
    margin(abs(t - est) / max(t, est))
    tr["j5_won"] = t > est
    return (t if t > est else est), count[0], tr
