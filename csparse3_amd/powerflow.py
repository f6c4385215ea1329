"""Newton-Raphson AC power flow on the device, in complex voltages: the sugar over csc_hip.PowerFlowPlan.

    pf = PowerFlow(Y, pv, pq, batch=64)                  # Y: a complex CscMat, or (n, Yp, Yi)
    V, info = pf.solve(Yz, S, V0)                        # V complex [batch, n]; info: iters, norm, flag per scenario

The loop of GridCal-style dSbus_dV + pack_4_by_4 + solve, with the mismatch, the Jacobian values, the factorisation,
the solve and the update all on the GPU (include/csparse3_amd.h, "AC power flow").  There is no CPU fallback.
"""
import numpy as np

from . import csc_hip


class PowerFlow:
    """Y: a CscMat with complex data (its values are the default Yz), or the pattern (n, Yp, Yi).  pv, pq: the bus lists;
    every bus in neither is a reference bus.  batch scenarios advance in lock-step; y_batch = 1 (one Y for all) or batch."""

    def __init__(self, Y, pv, pq, batch=1, y_batch=1, order=csc_hip.ORDER_AMD):
        self.Yz = None
        if isinstance(Y, (tuple, list)):
            n, Yp, Yi = Y
        else:
            assert Y.m == Y.n, "square matrix required"
            n, Yp, Yi = Y.n, Y.indptr, Y.indices
            nnz = int(np.asarray(Yp)[n])
            self.Yz = np.asarray(Y.data, dtype=np.complex128)[:nnz]
        self.plan = csc_hip.PowerFlowPlan(n, Yp, Yi, pv, pq, batch=batch, y_batch=y_batch, order=order)
        self.n, self.batch, self.y_batch = self.plan.n, self.plan.batch, self.plan.y_batch

    def close(self):
        self.plan.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def factorization(self):
        """The LU handle on the Jacobian, borrowed from the plan (condest, slogdet, selinv, sens_plan ... at the solution)."""
        return self.plan.factorization

    def _values(self, Yz):
        if Yz is None:
            assert self.Yz is not None, "no admittance values: pass Yz"
            Yz = self.Yz
        Yz = np.asarray(Yz, dtype=np.complex128)
        if self.y_batch > 1 and Yz.size == self.plan.nnz_y:
            Yz = np.broadcast_to(Yz.reshape(1, -1), (self.y_batch, self.plan.nnz_y))
        return Yz

    def _full(self, a, dtype):
        a = np.asarray(a, dtype=dtype)
        return np.broadcast_to(a.reshape(-1, self.n), (self.batch, self.n))

    def mismatch(self, Yz, S, V):
        """-> (-F float64[batch, nj], max |F| float64[batch]) at the complex voltages V."""
        V = self._full(V, np.complex128)
        return self.plan.mismatch(self._values(Yz), self._full(S, np.complex128), np.abs(V), np.angle(V))

    def jacobian(self, Yz, V):
        """-> Jx float64[batch, nnz_j] on plan.pattern() at the complex voltages V."""
        V = self._full(V, np.complex128)
        return self.plan.jacobian(self._values(Yz), np.abs(V), np.angle(V))

    def solve(self, Yz, S, V0, tol=1e-8, max_iters=20, refactor_every=1, pivot_tol=1e-3):
        """Newton from V0 (complex [n] or [batch, n]).  -> (V complex [batch, n], dict(iters, norm, flag)): flag 0
        converged (max |F| <= tol after iters steps), 1 out of iterations, 2 a mismatch that is not finite."""
        V0 = self._full(V0, np.complex128)
        vm, va, info = self.plan.solve(self._values(Yz), self._full(S, np.complex128), np.abs(V0), np.angle(V0), tol=tol,
                                       max_iters=max_iters, refactor_every=refactor_every, pivot_tol=pivot_tol)
        return vm * np.exp(1j * va), info
