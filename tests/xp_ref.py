"""NumPy restatement of the extra-precise refinement (cs3_residual_xp*, cs3_refine_xp*, csrc/refine_xp.hip): the doubled
residual operation for operation, and the iteration around any inner solver.

NumPy rounds every elementwise operation on its own, which is the kernel's "no contraction".  The one FMA of the kernel,
pl = fma(a, x, -fl(a x)), is the exact error of the product; Dekker's split product yields the same number whenever
nothing overflows, so resid_xp matches the device bit for bit."""
import numpy as np

EPS = 2.0 ** -52
STALL_RATIO = 0.5
SPLIT = 134217729.0          # 2^27 + 1


def two_sum(a, b):
    """Knuth: s = fl(a + b) and the exact error of that sum."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def two_prod(a, x):
    """Dekker / Veltkamp: p = fl(a x) and the exact error of that product (what fma(a, x, -p) returns)."""
    a, x = np.asarray(a, dtype=np.float64), np.asarray(x, dtype=np.float64)
    p = a * x
    c = SPLIT * a
    ah = c - (c - a)
    al = a - ah
    c = SPLIT * x
    xh = c - (c - x)
    xl = x - xh
    return p, ((ah * xh - p) + ah * xl + al * xh) + al * xl


def row_view(n, Ap, Ai, trans=False):
    """(Rp, Rj, Rmap): the entries of every row of op(A) in the order the kernels take them.  Plain: ascending column
    (entries of equal row keep their storage order, which is ascending column); trans: column i of A in storage order."""
    Ap, Ai = np.asarray(Ap, dtype=np.int64), np.asarray(Ai, dtype=np.int64)
    nnz = int(Ap[n])
    if trans:
        return Ap.copy(), Ai[:nnz].copy(), np.arange(nnz, dtype=np.int64)
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap[:n + 1]))
    order = np.argsort(Ai[:nnz], kind="stable")
    Rp = np.zeros(n + 1, dtype=np.int64)
    Rp[1:] = np.cumsum(np.bincount(Ai[:nnz], minlength=n))
    return Rp, cols[order], order


def resid_xp(n, Ap, Ai, Ax, b, x, xt=None, trans=False):
    """-> (r, s) shaped like b ([n] or [n, k]): r = b - op(A) (x + xt) in doubled precision rounded once,
    s = |b| + |op(A)| |x|.  All rows advance together, entry q of every row at step q: the order inside a row is kept."""
    Ax = np.asarray(Ax, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    shape = b.shape
    B = b.reshape(n, -1)
    X = np.asarray(x, dtype=np.float64).reshape(n, -1)
    XT = None if xt is None else np.asarray(xt, dtype=np.float64).reshape(n, -1)
    Rp, Rj, Rmap = row_view(n, Ap, Ai, trans)
    length = np.diff(Rp)
    sh, sl, den = B.copy(), np.zeros_like(B), np.abs(B)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(int(length.max(initial=0))):
            rows = np.nonzero(length > q)[0]
            p = Rp[rows] + q
            a = Ax[Rmap[p]][:, None]
            xj = X[Rj[p]]
            ph, pl = two_prod(a, xj)
            s, e = two_sum(sh[rows], -ph)
            sh[rows] = s
            c = e - pl
            if XT is not None:
                c = c - a * XT[Rj[p]]
            sl[rows] = sl[rows] + c
            den[rows] = den[rows] + np.abs(a) * np.abs(xj)
        r = sh + sl
    return r.reshape(shape), den.reshape(shape)


def _max_nan(v):
    """max of non-negative numbers in which a NaN wins (the kernels' maxima)."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if v.size == 0:
        return 0.0
    return float("nan") if np.isnan(v).any() else float(v.max())


def berr(n, Ap, Ai, Ax, b, x, trans=False):
    """Per column: max_i |r_i| / s_i of x alone (0 / 0 counts as 0, non-zero over zero is +inf) -> [k]."""
    r, s = resid_xp(n, Ap, Ai, Ax, b, x, None, trans)
    r, s = r.reshape(n, -1), s.reshape(n, -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where((r == 0.0) & (s == 0.0), 0.0, np.abs(r) / s)
    return np.array([_max_nan(ratio[:, t]) for t in range(ratio.shape[1])])


def ferr_rule(iters, flag, rate, nd_prev, nxf):
    if flag == 3:
        return float("nan")
    if iters == 0:
        return float("inf")
    if rate >= 1.0:
        return float("inf")
    if nd_prev == 0.0 and nxf == 0.0:
        return 0.0
    with np.errstate(divide="ignore"):
        return float(max(EPS, (np.float64(nd_prev) / np.float64(nxf)) / (1.0 - rate)))


def refine_xp(solve, n, Ap, Ai, Ax, b, x0, max_iters=10, trans=False):
    """One system b [n] from x0 with the inner solver `solve` (r -> op(A)^-1 r, approximately): the iteration of
    cs3_refine_xp_dev.  -> dict(x, xt, iters, flag, ferr, berr, rate, nd_prev)."""
    b = np.asarray(b, dtype=np.float64)
    x = np.array(x0, dtype=np.float64)
    xt = np.zeros(n)
    iters, flag, rate, nd_prev = 0, 0, 0.0, 0.0
    for _ in range(max_iters):
        r, _s = resid_xp(n, Ap, Ai, Ax, b, x, xt, trans)
        dx = np.asarray(solve(r), dtype=np.float64)
        nd, nx = _max_nan(np.abs(dx)), _max_nan(np.abs(x))
        if not (np.isfinite(nd) and np.isfinite(nx)):
            flag = 3
            break
        if iters > 0:
            rate = max(rate, nd / nd_prev)
            if nd > STALL_RATIO * nd_prev:
                flag = 2
                break
        s, e = two_sum(x, dx)
        x, xt = two_sum(s, xt + e)
        iters += 1
        nd_prev = nd
        if nd <= EPS * nx:
            flag = 1
            break
    nxf = _max_nan(np.abs(x))
    return dict(x=x, xt=xt, iters=iters, flag=flag, rate=rate, nd_prev=nd_prev, berr=float(berr(n, Ap, Ai, Ax, b, x, trans)[0]),
                ferr=ferr_rule(iters, flag, rate, nd_prev, nxf))


def plain_rounds(solve, n, Ap, Ai, Ax, b, x0, rounds=10, trans=False):
    """`rounds` of x += solve(b - op(A) x) with the residual summed in working precision (what cs3_refine_dev does)."""
    import scipy.sparse as sp
    A = sp.csc_matrix((np.asarray(Ax, dtype=np.float64), np.asarray(Ai), np.asarray(Ap)), shape=(n, n))
    A = A.T.tocsr() if trans else A.tocsr()
    x = np.array(x0, dtype=np.float64)
    for _ in range(rounds):
        x = x + solve(b - A @ x)
    return x


def _max_row(v):
    """(maximum with a NaN winning, its first row, its ratio to the runner-up of the column) of non-negative numbers.  A
    column of one entry has ratio inf, a column with a NaN ratio nan and the row of its first NaN."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if v.size == 0:
        return 0.0, -1, float("inf")
    nan = np.isnan(v)
    if nan.any():
        return float("nan"), int(np.argmax(nan)), float("nan")
    row = int(np.argmax(v))
    rest = np.delete(v, row)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float("inf") if rest.size == 0 else float(np.float64(v[row]) / np.float64(rest.max()))
    return float(v[row]), row, ratio


def refine_xp_all(solve_all, n, Ap, Ai, AX, B, X0, max_iters=10, trans=False):
    """All batch * k systems in lock-step, as refine_xp_run (api.cpp) drives them: AX [batch, nnz], B and X0 [batch, n, k],
    solve_all(R [batch, n, k]) -> the corrections of the whole array in one call.  Every pass: resid_xp with the tail on
    every system (stopped ones included), one solve_all, the maxima, the control rule and the update per system; the loop
    ends when no system is active.  -> dict(x, xt [batch, n, k]; iters, flag, rate, ferr, berr, nd_prev [batch * k];
    trace: one dict per pass of [batch, k] arrays nd, nx, row_d, row_x (the row of each maximum), ratio_d, ratio_x (its
    ratio to the runner-up of the column), apply, stopped (after the pass))."""
    AX = np.asarray(AX, dtype=np.float64).reshape(-1, int(np.asarray(Ap)[n]))
    batch = AX.shape[0]
    B = np.asarray(B, dtype=np.float64).reshape(batch, n, -1)
    k = B.shape[2]
    X = np.array(X0, dtype=np.float64).reshape(batch, n, k)
    XT = np.zeros_like(X)
    iters, flag = np.zeros((batch, k), dtype=np.int32), np.zeros((batch, k), dtype=np.int32)
    rate, nd_prev = np.zeros((batch, k)), np.zeros((batch, k))
    stopped = np.zeros((batch, k), dtype=bool)
    trace = []
    active = batch * k if n > 0 else 0
    for _ in range(max_iters):
        if not active:
            break
        R = np.stack([resid_xp(n, Ap, Ai, AX[m], B[m], X[m], XT[m], trans)[0] for m in range(batch)])
        D = np.asarray(solve_all(R), dtype=np.float64).reshape(batch, n, k)
        step = {key: np.zeros((batch, k), dtype=dt) for key, dt in (("nd", float), ("nx", float), ("row_d", np.int64),
                                                                     ("row_x", np.int64), ("ratio_d", float),
                                                                     ("ratio_x", float), ("apply", bool))}
        for m in range(batch):
            for t in range(k):
                nd, step["row_d"][m, t], step["ratio_d"][m, t] = _max_row(np.abs(D[m, :, t]))
                nx, step["row_x"][m, t], step["ratio_x"][m, t] = _max_row(np.abs(X[m, :, t]))
                step["nd"][m, t], step["nx"][m, t] = nd, nx
                if stopped[m, t]:
                    continue
                if not (np.isfinite(nd) and np.isfinite(nx)):
                    flag[m, t], stopped[m, t] = 3, True
                    continue
                if iters[m, t] > 0:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        q = float(np.float64(nd) / np.float64(nd_prev[m, t]))
                    if q > rate[m, t]:
                        rate[m, t] = q
                    if nd > STALL_RATIO * nd_prev[m, t]:
                        flag[m, t], stopped[m, t] = 2, True
                        continue
                step["apply"][m, t] = True
                iters[m, t] += 1
                nd_prev[m, t] = nd
                if nd <= EPS * nx:
                    flag[m, t], stopped[m, t] = 1, True
            cols = np.nonzero(step["apply"][m])[0]
            if cols.size:
                with np.errstate(invalid="ignore", over="ignore"):
                    s, e = two_sum(X[m][:, cols], D[m][:, cols])
                    X[m][:, cols], XT[m][:, cols] = two_sum(s, XT[m][:, cols] + e)
        step["stopped"] = stopped.copy()
        trace.append(step)
        active = int((~stopped).sum())
    be = np.stack([berr(n, Ap, Ai, AX[m], B[m], X[m], trans) for m in range(batch)]) if n > 0 else np.zeros((batch, k))
    fe = np.array([[ferr_rule(int(iters[m, t]), int(flag[m, t]), float(rate[m, t]), float(nd_prev[m, t]),
                              _max_nan(np.abs(X[m, :, t]))) for t in range(k)] for m in range(batch)])
    return dict(x=X, xt=XT, iters=iters.reshape(-1), flag=flag.reshape(-1), rate=rate.reshape(-1), ferr=fe.reshape(-1),
                berr=be.reshape(-1), nd_prev=nd_prev.reshape(-1), trace=trace)
