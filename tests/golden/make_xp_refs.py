"""Writes tests/golden/xp_refs.npz: for every refinement case of tests/xp_cases.py

  <name>_Ap, _Ai, _Ax, _Ax0, _b   the inputs (regenerating them must reproduce these arrays bit for bit)
  <name>_xh, _xt                  the solution of op(A) x = b computed with mpmath at 80 digits, as a double head and tail
  <name>_cond                     cond_1(A) from the 80-digit inverse
  <name>_etail                    e_tail_ref: max |(x + xt) - x*| / max |x*| that tests/xp_ref.py reached from x0 = solve(b)
                                  with SuperLU as the inner solver (natural order, diagonal pivots, double)

  python tests/golden/make_xp_refs.py

Needs mpmath and scipy, neither the library nor a GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import xp_cases as xc  # noqa: E402
import xp_ref  # noqa: E402

DIGITS = 80


def exact_solution(case):
    """-> (x as a list of mpf, cond_1)"""
    import mpmath as mp
    mp.mp.dps = DIGITS
    A = mp.matrix(case.n, case.n)
    for j in range(case.n):
        for p in range(case.Ap[j], case.Ap[j + 1]):
            i = int(case.Ai[p])
            if case.trans:
                A[j, i] = mp.mpf(float(case.Ax[p]))
            else:
                A[i, j] = mp.mpf(float(case.Ax[p]))
    x = mp.lu_solve(A, mp.matrix([mp.mpf(float(v)) for v in case.b]))
    cond = mp.mnorm(A, 1) * mp.mnorm(mp.inverse(A), 1)
    return [x[i] for i in range(case.n)], float(cond)


def tail_error(case, x_exact):
    """The error of x + xt of the NumPy restatement against the 80-digit solution, relative in the infinity norm."""
    import mpmath as mp
    solve = xc.superlu_solver(case)
    res = xp_ref.refine_xp(solve, case.n, case.Ap, case.Ai, case.Ax, case.b, solve(case.b), 10, case.trans)
    num = max(abs(mp.mpf(float(h)) + mp.mpf(float(t)) - e) for h, t, e in zip(res["x"], res["xt"], x_exact))
    return float(num / max(abs(e) for e in x_exact)), res


def main():
    import mpmath as mp
    out = {}
    for name, case in xc.refinement_cases().items():
        x, cond = exact_solution(case)
        xh = np.array([float(v) for v in x])
        xt = np.array([float(v - mp.mpf(float(h))) for v, h in zip(x, xh)])
        etail, res = tail_error(case, x)
        err = np.abs(res["x"] - xh).max() / np.abs(xh).max()
        print("%-14s n %3d cond %.1e  restatement: iters %2d flag %d rate %.2e ferr %.2e berr %.2e  err(head) %.2e  e_tail %.2e"
              % (name, case.n, cond, res["iters"], res["flag"], res["rate"], res["ferr"], res["berr"], err, etail))
        for key, val in (("Ap", case.Ap), ("Ai", case.Ai), ("Ax", case.Ax), ("Ax0", case.Ax0), ("b", case.b), ("xh", xh),
                         ("xt", xt), ("cond", np.float64(cond)), ("etail", np.float64(etail))):
            out["%s_%s" % (name, key)] = val
    np.savez_compressed(os.path.join(HERE, "xp_refs.npz"), **out)


if __name__ == "__main__":
    main()
