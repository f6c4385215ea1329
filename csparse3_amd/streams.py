"""Independent matrices with DISTINCT patterns, one matrix per HIP stream (BASELINE configs[4], "one matrix per GPU
stream"; SURVEY.md section 8d, second variant of config 5).

Matrices that share a pattern go through ONE batched handle (csc_hip.Factorization(batch=...)): one analysis, every
launch covers the whole batch.  Matrices with different patterns cannot share launches; what they can share is the GPU:
each gets its own handle (its own analysis, HBM state and hipGraph) and its factor + solve call is issued on one of a
small pool of streams, so that the per-level launches of different matrices overlap instead of queueing behind each
other.  torch supplies the streams and the device buffers; the numeric work is the C ABI's.

Matrices whose patterns differ only by a few entries (the cases of one network) do better than that: UnionBatch, below,
pads them to the union of their patterns and runs them as one batched handle.
"""
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from csparse3_amd import csc_hip


class DistinctBatch:
    """Handles for a list of matrices (m, n, Ap, Ai) with different patterns; analysis on construction.

    The analyses (ordering + symbolic, host C++ inside the library) are independent and run in a pool of threads: the
    ctypes call releases the interpreter lock and cs3_analyze keeps no shared state (its error string is per thread), so N
    patterns cost N / workers analyses of wall time instead of N (analysis_s records it).  workers=1 analyses in line."""

    def __init__(self, patterns, kind=csc_hip.CS3_LU, nstreams=8, device=None, workers=None):
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.kind = kind
        if workers is None:
            workers = min(len(patterns), os.cpu_count() or 1, 32)
        t0 = time.perf_counter()
        make = lambda p: csc_hip.Factorization(p[0], p[1], p[2], p[3], kind=kind)
        if workers > 1 and len(patterns) > 1:
            with ThreadPoolExecutor(max_workers=workers) as pool:
                self.handles = list(pool.map(make, patterns))           # (results in the order of `patterns`)
        else:
            self.handles = [make(p) for p in patterns]
        self.analysis_s = time.perf_counter() - t0
        self.workers = workers
        self.n = [int(p[1]) for p in patterns]
        self.streams = [torch.cuda.Stream(device=self.device) for _ in range(max(1, min(nstreams, len(patterns))))]

    def close(self):
        for h in self.handles:
            h.close()
        self.handles = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def factor_solve(self, values, rhs, tol=0.0):
        """values[i]: device tensor of matrix i's entries; rhs[i]: device tensor [n_i] or [n_i, k], overwritten by
        the solution.  Matrix i runs on stream i mod nstreams; returns after every stream has been waited for."""
        cur = torch.cuda.current_stream(self.device)
        for s in self.streams:
            s.wait_stream(cur)                       # the inputs were produced on the current stream
        for i, h in enumerate(self.handles):
            s = self.streams[i % len(self.streams)]
            x = rhs[i]
            k = 1 if x.dim() == 1 else x.shape[1]
            h.factor_solve_dev(values[i].data_ptr(), x.data_ptr(), k, tol, s.cuda_stream)
        for s in self.streams:
            cur.wait_stream(s)
        return rhs

    def status(self):
        """Raises for the first matrix whose factorisation failed (after synchronising)."""
        for i, h in enumerate(self.handles):
            h.factor_status(self.streams[i % len(self.streams)].cuda_stream)


class UnionBatch:
    """Matrices (m, n, Ap, Ai) of ONE order whose patterns differ but are all contained in a small common pattern -- the
    contingency cases, switching states or topology scans of one network -- on ONE batched handle.

    A matrix padded with explicit zeros to the union of the patterns has the factors of the unpadded matrix embedded in
    the union's structure, so the family runs as csc_hip.Factorization(n, n, Up, Ui, kind, batch=nmat): one analysis, one
    launch chain, every feature of a batched handle.  csc_hip.UnionPlan computes the union once; factor_solve() moves the
    members' values into the handle's [nmat, nnz_union] layout with one launch (no host copy) and factors + solves.
    handle_kwargs go to Factorization (order, q, schur, match_values); match_values are the values of ONE representative
    member in ITS pattern, given as (member index, values): they are padded to the union through the plan first.

    .plan, .factorization and .union_values (the device tensor [nmat, nnz_union] that the last factor_solve / embed
    filled) serve everything else: refine_dev, gmres_dev, condest_dev, ... take values in the handle's pattern, which is
    what union_values holds.

    Two limits follow from the handle code, which this class leaves as it is.  All members share n and, for Cholesky,
    the triangle convention.  And the factor status is one word per batch: a singular member (an islanded case, say)
    fails the whole call; with factorization.set_perturbation(delta) nothing fails and factorization.perturbed() says
    which member it was."""

    def __init__(self, patterns, kind=csc_hip.CS3_LU, device=None, **handle_kwargs):
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.kind = kind
        n = int(patterns[0][1])
        assert all(int(p[0]) == n and int(p[1]) == n for p in patterns), "square matrices of one order required"
        t0 = time.perf_counter()
        self.plan = csc_hip.UnionPlan(n, [(p[2], p[3]) for p in patterns])
        self.plan_s = time.perf_counter() - t0
        self.n, self.nmat, self.nnz = n, self.plan.nmat, self.plan.nnz
        Up, Ui = self.plan.pattern()
        mv = handle_kwargs.pop("match_values", None)
        if mv is not None:
            b, vals = mv
            off = self.plan.offsets()
            cat = np.zeros(int(off[-1]))
            cat[off[b]:off[b + 1]] = np.asarray(vals, dtype=np.float64).reshape(-1)[:off[b + 1] - off[b]]
            handle_kwargs["match_values"] = self.plan.values(cat)[b]
        self.factorization = csc_hip.Factorization(n, n, Up, Ui, kind=kind, batch=self.nmat, **handle_kwargs)
        self.union_values = torch.empty((self.nmat, self.nnz), dtype=torch.float64, device=self.device)
        self.plan.upload()

    def close(self):
        if self.factorization is not None:
            self.factorization.close()
            self.factorization = None
        self.plan.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def embed(self, values):
        """values: one concatenated device tensor (member b at plan.offsets()[b]) or a list of per-member device
        tensors, which is concatenated.  Fills and returns union_values, on the current stream."""
        if isinstance(values, (list, tuple)):
            values = torch.cat([v.reshape(-1) for v in values])
        assert values.dtype == torch.float64 and values.is_contiguous() and values.numel() >= self.plan.nnz_total
        self.plan.values_dev(values.data_ptr(), self.union_values.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        return self.union_values

    def factor_solve(self, values, rhs, tol=0.0):
        """values: as embed() takes them; rhs: device tensor [nmat, n] or [nmat, n, k], overwritten by the solutions.
        Embeds, then factors and solves the whole family on the current stream; asynchronous (status() reports)."""
        k = 1 if rhs.dim() == 2 else rhs.shape[2]
        assert rhs.shape[0] == self.nmat and rhs.shape[1] == self.n and rhs.is_contiguous()
        ux = self.embed(values)
        self.factorization.factor_solve_dev(ux.data_ptr(), rhs.data_ptr(), k, tol, torch.cuda.current_stream(self.device).cuda_stream)
        return rhs

    def status(self):
        """Raises if the factorisation of any member failed (after synchronising the current stream)."""
        self.factorization.factor_status(torch.cuda.current_stream(self.device).cuda_stream)
