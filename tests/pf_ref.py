"""NumPy restatement of the AC power flow (include/csparse3_amd.h, "AC power flow"): the Jacobian's pattern, the maps,
the mismatch and the Jacobian's values on separate real and imaginary arrays, and the driver's state machine around any
inner solver.  Every reference the power-flow tests use comes from here."""
import numpy as np

EPS = np.finfo(np.float64).eps


def plan_ref(n, Yp, Yi, pv, pq):
    """-> dict(Jp, Ji, jpos[4, nnz], Rp, Rj, Rpos, upos_a, upos_m, ubus, yrow, ycol, nj, npvpq)."""
    Yp, Yi = np.asarray(Yp, dtype=np.int64), np.asarray(Yi, dtype=np.int64)
    pv, pq = np.asarray(pv, dtype=np.int64).reshape(-1), np.asarray(pq, dtype=np.int64).reshape(-1)
    nnz, npv, npq = int(Yp[n]), len(pv), len(pq)
    npvpq, nj = npv + npq, npv + 2 * npq
    upos_a, upos_m = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    upos_a[pv] = np.arange(npv)
    upos_a[pq] = npv + np.arange(npq)
    upos_m[pq] = npvpq + np.arange(npq)
    ubus = np.concatenate([pv, pq, pq]).astype(np.int32)
    ycol = np.repeat(np.arange(n), np.diff(Yp)).astype(np.int32)
    jpos = np.full((4, nnz), -1, dtype=np.int32)
    Jp, Ji = np.zeros(nj + 1, dtype=np.int32), []
    for c in range(nj):
        j = int(ubus[c])
        top, bot = (1, 3) if c >= npvpq else (0, 2)
        for q in range(Yp[j], Yp[j + 1]):
            if upos_a[Yi[q]] >= 0:
                jpos[top, q] = len(Ji); Ji.append(upos_a[Yi[q]])
        for q in range(Yp[j], Yp[j + 1]):
            if upos_m[Yi[q]] >= 0:
                jpos[bot, q] = len(Ji); Ji.append(upos_m[Yi[q]])
        Jp[c + 1] = len(Ji)
    # Y by rows, ascending column: a stable sort of the entries (stored column by column) by row
    order = np.argsort(Yi[:nnz], kind="stable")
    Rp = np.zeros(n + 1, dtype=np.int32)
    Rp[1:] = np.cumsum(np.bincount(Yi[:nnz], minlength=n))
    return dict(Jp=Jp, Ji=np.asarray(Ji, dtype=np.int32), jpos=jpos, Rp=Rp, Rj=ycol[order].astype(np.int32),
                Rpos=order.astype(np.int32), upos_a=upos_a, upos_m=upos_m, ubus=ubus, yrow=Yi[:nnz].astype(np.int32),
                ycol=ycol, nj=nj, npvpq=npvpq, n=n, nnz=nnz)


def mismatch_ref(P, Yz, S, vm, va):
    """One scenario.  -> dict(F [nj] (= -mismatch, what the device writes), norm, Ir, Ii, bound [nj]): bound is the
    derived (d + 16) eps sum |terms| + eps |S_i| of every entry, d the stored entries of its row."""
    n = P["n"]
    yr, yi = np.real(Yz), np.imag(Yz)
    wr, wi = vm * np.cos(va), vm * np.sin(va)
    i, k = P["yrow"], P["ycol"]
    Ir = np.bincount(i, weights=yr * wr[k] - yi * wi[k], minlength=n)
    Ii = np.bincount(i, weights=yr * wi[k] + yi * wr[k], minlength=n)
    A = np.bincount(i, weights=np.hypot(yr, yi) * np.abs(vm[k]), minlength=n)
    A *= np.abs(vm)                                              # sum |V_i| |Y_ik| |V_k| over the row
    d = np.diff(P["Rp"])
    with np.errstate(invalid="ignore"):
        mr = wr * Ir + wi * Ii - np.real(S)
        mi = wi * Ir - wr * Ii - np.imag(S)
    F, bound = np.zeros(P["nj"]), np.zeros(P["nj"])
    a, m = P["upos_a"], P["upos_m"]
    F[a[a >= 0]] = -mr[a >= 0]
    F[m[m >= 0]] = -mi[m >= 0]
    row = (d + 16) * EPS * A
    with np.errstate(invalid="ignore"):
        bound[a[a >= 0]] = (row + EPS * np.abs(np.real(S)))[a >= 0]
        bound[m[m >= 0]] = (row + EPS * np.abs(np.imag(S)))[m >= 0]
    norm = np.abs(F).max() if not np.isnan(F).any() else np.nan
    return dict(F=F, norm=norm, Ir=Ir, Ii=Ii, bound=bound, rowsum=A, d=d)


def jacobian_ref(P, Yz, vm, va, cur=None):
    """One scenario.  -> (Jx [nnz_j], bound [nnz_j]) on the pattern of plan_ref; the bound as for the mismatch, d = 1 off
    the diagonal."""
    if cur is None:
        cur = mismatch_ref(P, Yz, np.zeros(P["n"], dtype=complex), vm, va)
    Ir, Ii, rowsum, drow = cur["Ir"], cur["Ii"], cur["rowsum"], cur["d"]
    nnz_j = int(P["Jp"][-1])
    Jx, bound = np.zeros(nnz_j), np.zeros(nnz_j)
    yr, yi = np.real(Yz), np.imag(Yz)
    c_, s_ = np.cos(va), np.sin(va)
    i, j = P["yrow"], P["ycol"]
    vir, vii = vm[i] * c_[i], vm[i] * s_[i]
    wr, wi = yr * c_[j] - yi * s_[j], yr * s_[j] + yi * c_[j]
    ur, ui = vir * wr + vii * wi, vii * wr - vir * wi                # V_i conj(Y_ij Vn_j)
    tr, ti = vm[j] * ur, vm[j] * ui                                  # V_i conj(Y_ij V_j)
    ay = np.hypot(yr, yi)
    h, m, nn, l = ti.copy(), -tr, ur.copy(), ui.copy()
    bt = 17 * EPS * np.abs(vm[i]) * ay * np.abs(vm[j])
    bv = 17 * EPS * np.abs(vm[i]) * ay
    dg = i == j
    sr, sm = vir * Ir[i] + vii * Ii[i], vii * Ir[i] - vir * Ii[i]    # V_i conj(I_i)
    h[dg], m[dg] = (ti - sm)[dg], (sr - tr)[dg]
    nn[dg] = (ur + (Ir[i] * c_[i] + Ii[i] * s_[i]))[dg]
    l[dg] = (ui + (Ir[i] * s_[i] - Ii[i] * c_[i]))[dg]
    with np.errstate(divide="ignore", invalid="ignore"):
        bt[dg] = ((drow[i] + 16) * EPS * (rowsum[i] + vm[i] * vm[i] * ay))[dg]
        bv[dg] = ((drow[i] + 16) * EPS * (rowsum[i] / np.abs(vm[i]) + np.abs(vm[i]) * ay))[dg]
    for blk, val, b in ((0, h, bt), (1, nn, bv), (2, m, bt), (3, l, bv)):
        pos = P["jpos"][blk]
        Jx[pos[pos >= 0]], bound[pos[pos >= 0]] = val[pos >= 0], b[pos >= 0]
    return Jx, bound


def dense_jacobian(P, Jx):
    J = np.zeros((P["nj"], P["nj"]))
    for c in range(P["nj"]):
        for p in range(P["Jp"][c], P["Jp"][c + 1]):
            J[P["Ji"][p], c] = Jx[p]
    return J


def dense_solve(P, Jx, rhs):
    return np.linalg.solve(dense_jacobian(P, Jx), rhs)


def newton_ref(P, Yz, S, vm, va, tol, max_iters, refactor_every=1, solver=dense_solve):
    """The driver's state machine for one scenario.  -> dict(vm, va, iters, norm, flag, norms): norms lists the norm of
    every iteration that was evaluated."""
    vm, va = np.array(vm, dtype=float), np.array(va, dtype=float)
    norms, held = [], None
    it = 0
    while True:
        cur = mismatch_ref(P, Yz, S, vm, va)
        norms.append(cur["norm"])
        if not np.isfinite(cur["norm"]):
            flag = 2; break
        if cur["norm"] <= tol:
            flag = 0; break
        if it == max_iters:
            flag = 1; break
        if it % refactor_every == 0:
            held = jacobian_ref(P, Yz, vm, va, cur)[0]
        dx = solver(P, held, cur["F"])
        va[P["ubus"][:P["npvpq"]]] += dx[:P["npvpq"]]
        vm[P["ubus"][P["npvpq"]:]] += dx[P["npvpq"]:]
        it += 1
    return dict(vm=vm, va=va, iters=it, norm=norms[-1], flag=flag, norms=norms)


def unknowns(P, vm, va):
    return np.concatenate([va[P["ubus"][:P["npvpq"]]], vm[P["ubus"][P["npvpq"]:]]])
