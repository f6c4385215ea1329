"""Weighted-least-squares AC state estimation on the device, in complex voltages: the sugar over csc_hip.StateEstPlan.

    se = StateEstimator(Y, ref, (end_from, end_to), (kind, where))      # Y: a complex CscMat, or (n, Yp, Yi)
    V, info = se.solve(Yz, Ye, z, w, V0)                                # V complex [n]; info: iters, step, J, flag
    rn, info = se.bad_data(Yz, Ye, z, w, V)                             # normalised residuals; info: worst, worst_row, ...

Gauss-Newton on J(x) = sum w (z - h(x))^2 with the residuals, the measurement Jacobian, the gain matrix H' W H, its
Cholesky factorisation, the solve and the update all on the GPU, and the largest-normalised-residual test on the selected
inverse of the gain matrix (include/csparse3_amd.h, "AC state estimation").  There is no CPU fallback.
"""
import numpy as np

from . import csc_hip


class StateEstimator:
    """Y: a CscMat with complex data (its values are the default Yz), or the pattern (n, Yp, Yi).  ref: the buses whose
    angle is fixed.  ends = (end_from, end_to): the branch-end table.  meas = (kind, where): the measurement rows
    (kind 0 |V|, 1 / 2 P / Q injection at a bus, 3 / 4 P / Q flow at a branch end)."""

    def __init__(self, Y, ref, ends, meas, order=csc_hip.ORDER_AMD):
        self.Yz = None
        if isinstance(Y, (tuple, list)):
            n, Yp, Yi = Y
        else:
            assert Y.m == Y.n, "square matrix required"
            n, Yp, Yi = Y.n, Y.indptr, Y.indices
            nnz = int(np.asarray(Yp)[n])
            self.Yz = np.asarray(Y.data, dtype=np.complex128)[:nnz]
        self.plan = csc_hip.StateEstPlan(n, Yp, Yi, ref, ends[0], ends[1], meas[0], meas[1], order=order)
        self.n, self.m, self.ns = self.plan.n, self.plan.m, self.plan.ns

    def close(self):
        self.plan.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def factorization(self):
        """The Cholesky handle on the gain matrix, borrowed from the plan (condest, slogdet, selinv ... at the solution)."""
        return self.plan.factorization

    def _values(self, Yz):
        if Yz is None:
            assert self.Yz is not None, "no admittance values: pass Yz"
            Yz = self.Yz
        return np.asarray(Yz, dtype=np.complex128)

    def residuals(self, Yz, Ye, z, w, V):
        """-> (r = z - h(x) float64[m], J = sum w r^2) at the complex voltages V."""
        V = np.asarray(V, dtype=np.complex128)
        return self.plan.measure(self._values(Yz), Ye, z, w, np.abs(V), np.angle(V))

    def jacobian(self, Yz, Ye, w, V):
        """-> (Hr, Hc, WHc) float64[nnz_h] on plan.pattern() at the complex voltages V."""
        V = np.asarray(V, dtype=np.complex128)
        return self.plan.jacobian(self._values(Yz), Ye, w, np.abs(V), np.angle(V))

    def solve(self, Yz, Ye, z, w, V0, tol=1e-8, max_iters=20):
        """Gauss-Newton from V0 (complex [n]).  -> (V complex [n], dict(iters, step, J, flag)): flag 0 converged
        (max |dx| <= tol after iters steps), 1 out of iterations, 2 a step that is not finite."""
        V0 = np.asarray(V0, dtype=np.complex128)
        vm, va, info = self.plan.solve(self._values(Yz), Ye, z, w, np.abs(V0), np.angle(V0), tol=tol, max_iters=max_iters)
        return vm * np.exp(1j * va), info

    def bad_data(self, Yz, Ye, z, w, V, crit_tol=1e-8):
        """The largest-normalised-residual test at V.  -> (rn float64[m], dict(t, omega, worst, worst_row, J, critical))."""
        V = np.asarray(V, dtype=np.complex128)
        out = self.plan.bad_data(self._values(Yz), Ye, z, w, np.abs(V), np.angle(V), crit_tol=crit_tol)
        return out.pop("rn"), out
