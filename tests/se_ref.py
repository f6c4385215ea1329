"""NumPy restatement of the AC state estimation (include/csparse3_amd.h, "AC state estimation"): the pattern of the
measurement Jacobian H by rows and in CSC with its maps, the measurement functions and the values of H on separate real and
imaginary arrays with derived error bounds, the gradient in the device's summation order, the Gauss-Newton state machine
around a dense solver, and the dense normalised residuals.  Every reference the state-estimation tests use comes from here.

Bounds, as pf_ref.py derives its own: per entry |dev - ref| <= (d + 16) eps sum |terms| (+ eps |z_i| for a residual), d the
stored entries of the row of Y behind an injection, d = 2 for a flow, d = 1 for an off-diagonal derivative: a term is three
roundings deep plus 2 ulp each from sin and cos, under 8 eps, a sum of d terms adds d - 1, and the bound doubles that."""
import numpy as np

EPS = np.finfo(np.float64).eps


def plan_ref(n, Yp, Yi, ref, end_from, end_to, kind, where):
    """-> dict: Y by rows (Rp, Rj, Rpos), upos_a, upos_m, sbus, H by rows (Hrp, Hrj), in CSC (Hp, Hi), cpos, and per
    row-order entry e_row, e_src (entry of Yz / branch end), e_bus (the state's bus), e_fam (0 one, 1 injection, 2 flow),
    e_imag, e_mag, e_near (the diagonal of an injection row, the from-bus of a flow row)."""
    Yp, Yi = np.asarray(Yp, dtype=np.int64), np.asarray(Yi, dtype=np.int64)
    ref = np.asarray(ref, dtype=np.int64).reshape(-1)
    end_from, end_to = np.asarray(end_from, dtype=np.int64).reshape(-1), np.asarray(end_to, dtype=np.int64).reshape(-1)
    kind, where = np.asarray(kind, dtype=np.int64).reshape(-1), np.asarray(where, dtype=np.int64).reshape(-1)
    nnz, m = int(Yp[n]), len(kind)
    na, ns = n - len(ref), 2 * n - len(ref)
    upos_a = np.zeros(n, dtype=np.int32)
    upos_a[ref] = -1
    upos_a[upos_a >= 0] = np.arange(na)
    upos_m = (na + np.arange(n)).astype(np.int32)
    sbus = np.concatenate([np.flatnonzero(upos_a >= 0), np.arange(n)]).astype(np.int32)
    ycol = np.repeat(np.arange(n), np.diff(Yp))
    order = np.argsort(Yi[:nnz], kind="stable")                  # Y by rows, ascending column
    Rp = np.zeros(n + 1, dtype=np.int64)
    Rp[1:] = np.cumsum(np.bincount(Yi[:nnz], minlength=n))
    Rj, Rpos = ycol[order], order
    # one tuple per entry, in row order: (state, row, src, bus, family, imag, mag, near); plain Python, it is a definition
    ent = []
    Hrp = np.zeros(m + 1, dtype=np.int64)
    ua, um, rj, rpos, rp = upos_a.tolist(), upos_m.tolist(), Rj.tolist(), Rpos.tolist(), Rp.tolist()
    ef, et = end_from.tolist(), end_to.tolist()
    for i, (k, at) in enumerate(zip(kind.tolist(), where.tolist())):
        im = k in (2, 4)
        if k == 0:
            ent.append((um[at], i, 0, at, 0, False, True, False))
        elif k <= 2:
            seg = range(rp[at], rp[at + 1])
            ent += [(ua[rj[p]], i, rpos[p], rj[p], 1, im, False, rj[p] == at) for p in seg if ua[rj[p]] >= 0]
            ent += [(um[rj[p]], i, rpos[p], rj[p], 1, im, True, rj[p] == at) for p in seg]
        else:
            sides = ((ef[at], True), (et[at], False))
            ent += [(ua[j], i, at, j, 2, im, False, nr) for j, nr in sides if ua[j] >= 0]
            ent += [(um[j], i, at, j, 2, im, True, nr) for j, nr in sides]
        Hrp[i + 1] = len(ent)
    E = np.array(ent, dtype=np.int64).reshape(-1, 8)
    Hrj, e_row = E[:, 0], E[:, 1]
    by_col = np.argsort(Hrj, kind="stable")                      # CSC: ascending measurement inside a column
    cpos = np.empty(len(Hrj), dtype=np.int64)
    cpos[by_col] = np.arange(len(Hrj))
    Hp = np.zeros(ns + 1, dtype=np.int64)
    Hp[1:] = np.cumsum(np.bincount(Hrj, minlength=ns))
    return dict(n=n, nnz=nnz, m=m, na=na, ns=ns, ne=len(end_from), nnz_h=len(Hrj), Rp=Rp, Rj=Rj, Rpos=Rpos, yrow=Yi[:nnz], ycol=ycol,
                upos_a=upos_a, upos_m=upos_m, sbus=sbus, kind=kind, where=where, end_from=end_from, end_to=end_to,
                Hrp=Hrp.astype(np.int32), Hrj=Hrj.astype(np.int32), Hp=Hp.astype(np.int32), Hi=e_row[by_col].astype(np.int32),
                cpos=cpos.astype(np.int32), e_row=e_row, e_src=E[:, 2], e_bus=E[:, 3], e_fam=E[:, 4], e_imag=E[:, 5] != 0,
                e_mag=E[:, 6] != 0, e_near=E[:, 7] != 0)


def _ends(P, Ye):
    Ye = np.asarray(Ye, dtype=np.complex128).reshape(-1, 2)
    return Ye[:, 0].real, Ye[:, 0].imag, Ye[:, 1].real, Ye[:, 1].imag


def measure_ref(P, Yz, Ye, z, vm, va):
    """-> dict(h, r [m], bound [m], Ir, Ii, rowsum, d, and the flow currents Fr, Fi, flowsum [ne])."""
    n = P["n"]
    yr, yi = np.real(Yz), np.imag(Yz)
    wr, wi = vm * np.cos(va), vm * np.sin(va)
    i, k = P["yrow"], P["ycol"]
    Ir = np.bincount(i, weights=yr * wr[k] - yi * wi[k], minlength=n)
    Ii = np.bincount(i, weights=yr * wi[k] + yi * wr[k], minlength=n)
    rowsum = np.abs(vm) * np.bincount(i, weights=np.hypot(yr, yi) * np.abs(vm[k]), minlength=n)     # sum |V_i| |Y_ik| |V_k|
    d = np.diff(P["Rp"])
    f, t = P["end_from"], P["end_to"]
    ffr, ffi, ftr, fti = _ends(P, Ye)
    Fr = (ffr * wr[f] - ffi * wi[f]) + (ftr * wr[t] - fti * wi[t])
    Fi = (ffr * wi[f] + ffi * wr[f]) + (ftr * wi[t] + fti * wr[t])
    flowsum = np.abs(vm[f]) * (np.hypot(ffr, ffi) * np.abs(vm[f]) + np.hypot(ftr, fti) * np.abs(vm[t]))
    kind, at = P["kind"], P["where"]
    h, terms, depth = np.zeros(P["m"]), np.zeros(P["m"]), np.zeros(P["m"])
    for kk in range(5):
        sel = kind == kk
        a = at[sel]
        if kk == 0:
            h[sel], terms[sel] = vm[a], np.abs(vm[a])
        elif kk <= 2:
            h[sel] = (wr[a] * Ir[a] + wi[a] * Ii[a]) if kk == 1 else (wi[a] * Ir[a] - wr[a] * Ii[a])
            terms[sel], depth[sel] = rowsum[a], d[a]
        else:
            h[sel] = (wr[f[a]] * Fr[a] + wi[f[a]] * Fi[a]) if kk == 3 else (wi[f[a]] * Fr[a] - wr[f[a]] * Fi[a])
            terms[sel], depth[sel] = flowsum[a], 2
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        r = z - h
        bound = (depth + 16) * EPS * terms + EPS * np.abs(z)
    return dict(h=h, r=r, bound=bound, Ir=Ir, Ii=Ii, rowsum=rowsum, d=d, Fr=Fr, Fi=Fi, flowsum=flowsum)


def jacobian_ref(P, Yz, Ye, vm, va, cur=None):
    """-> (Hr [nnz_h] in row order, bound [nnz_h])."""
    if cur is None:
        cur = measure_ref(P, Yz, Ye, np.zeros(P["m"]), vm, va)
    c_, s_ = np.cos(va), np.sin(va)
    row, src, j = P["e_row"], P["e_src"], P["e_bus"]
    fam, imag, mag, near = P["e_fam"], P["e_imag"], P["e_mag"], P["e_near"]
    Hr, bound = np.ones(P["nnz_h"]), np.zeros(P["nnz_h"])
    # injections: the formulas of pf_ref.jacobian_ref
    e = np.flatnonzero(fam == 1)
    if len(e):
        i, jj, q = P["where"][row[e]], j[e], src[e]
        yr, yi = np.real(Yz)[q], np.imag(Yz)[q]
        Ir, Ii = cur["Ir"][i], cur["Ii"][i]
        vir, vii = vm[i] * c_[i], vm[i] * s_[i]
        wr, wi = yr * c_[jj] - yi * s_[jj], yr * s_[jj] + yi * c_[jj]
        ur, ui = vir * wr + vii * wi, vii * wr - vir * wi                # V_i conj(Y_ij Vn_j)
        tr, ti = vm[jj] * ur, vm[jj] * ui                                # V_i conj(Y_ij V_j)
        sr, sm = vir * Ir + vii * Ii, vii * Ir - vir * Ii                # V_i conj(I_i)
        ay = np.hypot(yr, yi)
        dg, mg, im = near[e], mag[e], imag[e]
        th_re, th_im = np.where(dg, ti - sm, ti), np.where(dg, sr - tr, -tr)
        mg_re = np.where(dg, ur + (Ir * c_[i] + Ii * s_[i]), ur)
        mg_im = np.where(dg, ui + (Ir * s_[i] - Ii * c_[i]), ui)
        Hr[e] = np.where(mg, np.where(im, mg_im, mg_re), np.where(im, th_im, th_re))
        drow, rowsum = cur["d"][i], cur["rowsum"][i]
        with np.errstate(divide="ignore", invalid="ignore"):
            bt = np.where(dg, (drow + 16) * EPS * (rowsum + vm[i] * vm[i] * ay), 17 * EPS * np.abs(vm[i]) * ay * np.abs(vm[jj]))
            bv = np.where(dg, (drow + 16) * EPS * (rowsum / np.abs(vm[i]) + np.abs(vm[i]) * ay), 17 * EPS * np.abs(vm[i]) * ay)
        bound[e] = np.where(mg, bv, bt)
    # flows
    e = np.flatnonzero(fam == 2)
    if len(e):
        k = src[e]
        f, t = P["end_from"][k], P["end_to"][k]
        ffr, ffi, ftr, fti = (a[k] for a in _ends(P, Ye))
        fr, fi = vm[f] * c_[f], vm[f] * s_[f]
        wr, wi = ftr * c_[t] - fti * s_[t], ftr * s_[t] + fti * c_[t]     # yft Vn_t
        ur, ui = fr * wr + fi * wi, fi * wr - fr * wi                    # V_f conj(yft Vn_t)
        ar, ai = vm[t] * ur, vm[t] * ui                                  # A = V_f conj(yft V_t)
        Fr, Fi = cur["Fr"][k], cur["Fi"][k]
        nr, mg, im = near[e], mag[e], imag[e]
        th = np.where(nr, np.where(im, ar, -ai), np.where(im, -ar, ai))  # j A at the from-bus, -j A at the to-bus
        own_re = (Fr * c_[f] + Fi * s_[f]) + vm[f] * ffr                 # conj(I_k) Vn_f + |V_f| conj(yff)
        own_im = (Fr * s_[f] - Fi * c_[f]) - vm[f] * ffi
        mgv = np.where(nr, np.where(im, own_im, own_re), np.where(im, ui, ur))
        Hr[e] = np.where(mg, mgv, th)
        aff, aft = np.hypot(ffr, ffi), np.hypot(ftr, fti)
        b_th = 18 * EPS * np.abs(vm[f]) * aft * np.abs(vm[t])
        b_to = 18 * EPS * np.abs(vm[f]) * aft
        b_own = 18 * EPS * (2 * aff * np.abs(vm[f]) + aft * np.abs(vm[t]))
        bound[e] = np.where(mg, np.where(nr, b_own, b_to), b_th)
    return Hr, bound


def dense_h(P, Hr):
    H = np.zeros((P["m"], P["ns"]))
    H[P["e_row"], P["Hrj"]] = Hr
    return H


def _sequential_columns(terms, ptr):
    """Per column the sum s = 0; s += t0; s += t1; ... of its terms, all columns at once."""
    ncol = len(ptr) - 1
    length = np.diff(ptr)
    s = np.zeros(ncol)
    for k in range(int(length.max(initial=0))):
        sel = np.flatnonzero(length > k)
        s[sel] = s[sel] + terms[ptr[sel] + k]
    return s


def _tree(v):
    """64 lanes: lane l += lane l + off for l < off, off = 32, 16, ..., 1; lane 0."""
    v = np.asarray(v, dtype=np.float64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v[:off] + v[off:2 * off]
    return v[0]


def _waves(s):
    """256 threads: the tree inside each wave, then the four waves in order."""
    S = [_tree(s[64 * v:64 * v + 64]) for v in range(4)]
    return ((S[0] + S[1]) + S[2]) + S[3]


def _strided(terms, nthreads):
    """thread j: the sequential sum of terms j, j + nthreads, ..."""
    out = np.zeros(nthreads)
    for j in range(nthreads):
        for v in terms[j::nthreads]:
            out[j] = out[j] + v
    return out


def gradient_ref(P, Hc, wr, wave_col):
    """g [ns] = H' (w r) as k_se_gradient adds it: every product rounded, a column of at most wave_col entries in stored
    order, a longer one by 64 lanes taking entries l, l + 64, ... in order and then the tree."""
    Hp, Hi = P["Hp"].astype(np.int64), P["Hi"]
    terms = np.asarray(Hc) * np.asarray(wr)[Hi]
    g = _sequential_columns(terms, Hp)
    for j in np.flatnonzero(np.diff(Hp) > wave_col):
        g[j] = _tree(_strided(terms[Hp[j]:Hp[j + 1]], 64))
    return g


def cost_ref(w, r):
    """J = sum w (r r) by the tree of k_se_residual / k_se_close: groups of 256 consecutive rows (zeros behind the last),
    each by the tree and the waves; then thread j takes the groups j, j + 256, ... in order, and again the tree and the waves."""
    x = np.asarray(w) * (np.asarray(r) * np.asarray(r))
    ngroups = -(-len(x) // 256)
    padded = np.zeros(ngroups * 256)
    padded[:len(x)] = x
    parts = np.array([_waves(padded[g * 256:(g + 1) * 256]) for g in range(ngroups)])
    return _waves(_strided(parts, 256))


def state_of(P, vm, va):
    return np.concatenate([np.asarray(va)[P["sbus"][:P["na"]]], np.asarray(vm)])


def gain_ref(P, Hr, w):
    H = dense_h(P, Hr)
    return H, H.T @ (np.asarray(w)[:, None] * H)


def gauss_newton_ref(P, Yz, Ye, z, w, vm, va, tol, max_iters):
    """The driver's state machine around a dense Cholesky solve.  -> dict(vm, va, iters, step, flag, J, r, steps, spd):
    steps lists max |dx| of every iteration; spd is False when a gain matrix was not positive definite (the voltages are
    then those before that iteration)."""
    vm, va = np.array(vm, dtype=float), np.array(va, dtype=float)
    w = np.asarray(w, dtype=float)
    steps, flag, spd = [], 1, True
    for _ in range(max_iters):
        cur = measure_ref(P, Yz, Ye, z, vm, va)
        H, G = gain_ref(P, jacobian_ref(P, Yz, Ye, vm, va, cur)[0], w)
        try:
            L = np.linalg.cholesky(G)
        except np.linalg.LinAlgError:
            spd = False
            break
        with np.errstate(invalid="ignore"):
            g = H.T @ (w * cur["r"])
            dx = np.linalg.solve(L.T, np.linalg.solve(L, g))
        va[P["sbus"][:P["na"]]] += dx[:P["na"]]
        vm += dx[P["na"]:]
        steps.append(np.abs(dx).max() if np.isfinite(dx).all() else np.nan)
        if not np.isfinite(steps[-1]):
            flag = 2; break
        if steps[-1] <= tol:
            flag = 0; break
        flag = 1
    cur = measure_ref(P, Yz, Ye, z, vm, va)
    with np.errstate(invalid="ignore"):
        J = float(np.sum(w * cur["r"] * cur["r"]))
    return dict(vm=vm, va=va, iters=len(steps), step=steps[-1] if steps else 0.0, flag=flag, J=J, r=cur["r"], steps=steps, spd=spd)


def baddata_ref(P, Hr, w, r):
    """Dense Omega = W^-1 - H G^-1 H'.  -> dict(t, omega, rn [m], scale [m] = sum |h_a| |Z(a, b)| |h_b| per row, cond_1 of G)."""
    H, G = gain_ref(P, Hr, w)
    Z = np.linalg.inv(G)
    cond = float(np.abs(G).sum(axis=0).max() * np.abs(Z).sum(axis=0).max())
    t = ((H @ Z) * H).sum(axis=1)
    scale = ((np.abs(H) @ np.abs(Z)) * np.abs(H)).sum(axis=1)
    omega = 1.0 / np.asarray(w) - t
    with np.errstate(invalid="ignore"):
        rn = np.abs(r) / np.sqrt(omega)
    return dict(t=t, omega=omega, rn=rn, scale=scale, cond=cond)
