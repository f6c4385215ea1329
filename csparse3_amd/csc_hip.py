"""ctypes binding of libcsparse3_hip.so -- the MI355X factor/solve kernels behind
the reference's flat-array calling convention.

Every function takes and returns what a kernel module of the reference does
(/root/reference/src/CSparse3/csc_numba.py): scalars int64, index arrays int32,
values float64, matrices as loose (m, n, Ap, Ai, Ax) arguments, results as
tuples of freshly allocated NumPy arrays, or in place for the solves.  The
binding idiom is the reference author's own (research/mkl.py:3-5,33-35):
ctypes.CDLL + ndarray.ctypes.data_as.

There is no CPU fallback: if the shared library is missing or no GPU is
visible the numeric entry points raise.
"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CS3_LIB_PATH") or os.path.join(_HERE, "libcsparse3_hip.so")   # (override: sanitizer builds, tools/asan_host.sh)

CS3_LU, CS3_CHOLESKY = 0, 1
CS3_ERR_ARG, CS3_ERR_ALLOC, CS3_ERR_HIP, CS3_ERR_PIVOT, CS3_ERR_NOT_SPD, CS3_ERR_STATE = -1, -2, -3, -4, -5, -6      # include/csparse3_amd.h
ORDER_NATURAL, ORDER_AMD, ORDER_GIVEN = 0, 1, 2

_i32p = C.POINTER(C.c_int32)
_f64p = C.POINTER(C.c_double)
I64 = C.c_int64


class Cs3Info(C.Structure):
    _fields_ = [("n", C.c_int64), ("nnz_a", C.c_int64), ("nnz_l", C.c_int64), ("nnz_u", C.c_int64),
                ("nsuper", C.c_int64), ("nlevels", C.c_int64), ("max_front", C.c_int64),
                ("max_width", C.c_int64), ("factor_bytes", C.c_int64), ("update_bytes", C.c_int64),
                ("batch", C.c_int64), ("fail_col", C.c_int64), ("flops_factor", C.c_double),
                ("t_order_s", C.c_double), ("t_symbolic_s", C.c_double)]


class SpgemmInfo(C.Structure):
    """cs3_spgemm_info: sizes of a product plan and how much of it went through each path."""
    _fields_ = [(name, C.c_int64) for name in ("m", "n", "nnz_a", "nnz_b", "nnz_c", "products", "cols_lds", "cols_global",
                                               "entries_sliced", "entries_long", "padded_pairs", "long_list")]


class SpgemmLimits(C.Structure):
    """cs3_spgemm_limits_t: the constants that separate the paths of the product."""
    _fields_ = [(name, C.c_int64) for name in ("lds_products", "lds_table_rows", "long_list", "slice_width",
                                               "rank_chunk_lds", "rank_chunk_global")]


class UnionInfo(C.Structure):
    """cs3_union_info: sizes of a union plan."""
    _fields_ = [(name, C.c_int64) for name in ("n", "nmat", "nnz_union", "nnz_total", "distinct_patterns", "padded", "dup_slots")]


class UnionLimits(C.Structure):
    """cs3_union_limits_t: the constants that shape the launch of the embedding kernel."""
    _fields_ = [(name, C.c_int64) for name in ("block", "grid_cap", "entries_per_lane")]


class CplxInfo(C.Structure):
    """cs3_cplx_info: sizes of a complex plan and of the real form the handle analyses."""
    _fields_ = [(name, C.c_int64) for name in ("n", "nnz", "batch", "rotate", "n_real", "nnz_real", "rows_without_diagonal")]


class CplxLimits(C.Structure):
    """cs3_cplx_limits_t: the constants that shape the launches of the complex glue kernels."""
    _fields_ = [(name, C.c_int64) for name in ("block", "grid_cap")]


class GmresLimits(C.Structure):
    """cs3_gmres_limits_t: the largest restart, the rows per chunk of the fixed-order reductions, the right-hand sides
    per tile of the kernels."""
    _fields_ = [(name, C.c_int64) for name in ("max_restart", "chunk_rows", "rhs_tile")]


class RefineXpLimits(C.Structure):
    """cs3_refine_xp_limits_t: threads per workgroup and the workgroup cap of the doubled-precision residual kernel, the
    default max_iters, eps = 2^-52 and the stall ratio of the extra-precise refinement, the workgroup cap over the rows of
    the maxima kernel."""
    _fields_ = [(name, C.c_int64) for name in ("block", "grid_cap", "max_iters_default")] + \
               [(name, C.c_double) for name in ("eps", "stall_ratio")] + [("maxima_grid_cap", C.c_int64)]


class SensInfo(C.Structure):
    """cs3_sens_info_t: sizes of a plan for Y = C op(A)^-1 B, the side it is evaluated from (1 right, 2 left), its tiles."""
    _fields_ = [(name, C.c_int64) for name in ("k", "p", "side", "trans", "ntiles", "max_width", "nnz_b", "nnz_c")]

    def __repr__(self):
        return "SensInfo(%s)" % ", ".join("%s=%d" % (f, getattr(self, f)) for f, _ in self._fields_)


class SensLimits(C.Structure):
    """cs3_sens_limits_t: the constants that shape the tiles and launches of the sparse right-hand-side path."""
    _fields_ = [(name, C.c_int64) for name in ("max_tile", "pad_width", "scatter_rows", "scatter_threads", "combine_cols",
                                               "combine_lanes", "tblock")]


class SelinvLimits(C.Structure):
    """cs3_selinv_limits_t: the front orders at which the selected inversion changes kernel, and its tile sizes."""
    _fields_ = [(name, C.c_int64) for name in ("lds_max_order", "wave_max_order", "gemm_tile", "diag_block")]


class SelinvInfo(C.Structure):
    """cs3_selinv_info_t: doubles of Z per matrix, fronts inside and beyond the LDS, launches of one selected inversion."""
    _fields_ = [(name, C.c_int64) for name in ("zpool_doubles", "nfronts_small", "nfronts_big", "nlaunches")]

    def __repr__(self):
        return "SelinvInfo(%s)" % ", ".join("%s=%d" % (f, getattr(self, f)) for f, _ in self._fields_)


class QuadLimits(C.Structure):
    """cs3_quad_limits_t: the term counts at which a row of the bilinear forms changes class, and the kernels' sizes."""
    _fields_ = [(name, C.c_int64) for name in ("lane_max_terms", "wave_max_terms", "block", "lane_chunk", "reduce_rows")]


class QuadInfo(C.Structure):
    """cs3_quad_info_t: rows, entries of C and B, terms, whether B = C, and the rows per class of a QuadPlan."""
    _fields_ = [(name, C.c_int64) for name in ("m", "nnz_c", "nnz_b", "nterms", "same_operand", "rows_lane", "rows_wave",
                                               "rows_workgroup")]

    def __repr__(self):
        return "QuadInfo(%s)" % ", ".join("%s=%d" % (f, getattr(self, f)) for f, _ in self._fields_)


class CplxUpdatesLimits(C.Structure):
    """cs3_cplx_updates_limits_t: the constants that shape the kernels of the complex low-rank-modified solves."""
    _fields_ = [(name, C.c_int64) for name in ("unit_rows", "unit_threads", "apply_stage", "apply_rows", "apply_threads_min",
                                               "max_rank", "max_tile", "max_tile_cases")]


class CplxSelinvLimits(C.Structure):
    """cs3_cplx_selinv_limits_t: threads per workgroup and the workgroup cap of the complex selected-inverse getters."""
    _fields_ = [(name, C.c_int64) for name in ("block", "grid_cap")]


class PfInfo(C.Structure):
    """cs3_pf_info: sizes of a power-flow plan and how its rows are summed."""
    _fields_ = [(name, C.c_int64) for name in ("n", "nnz_y", "npv", "npq", "nref", "nj", "nnz_j", "batch", "y_batch",
                                               "rows_lane", "rows_wave", "max_row")]

    def __repr__(self):
        return "PfInfo(%s)" % ", ".join("%s=%d" % (f, getattr(self, f)) for f, _ in self._fields_)


class PfLimits(C.Structure):
    """cs3_pf_limits_t: the constants that shape the launches of the power-flow kernels."""
    _fields_ = [(name, C.c_int64) for name in ("block", "grid_cap", "wave_row")]


class SeInfo(C.Structure):
    """cs3_se_info: sizes of a state-estimation plan (kind0 .. kind4: the rows per kind)."""
    _fields_ = [(name, C.c_int64) for name in ("n", "nnz_y", "nref", "na", "ns", "ne", "m", "nnz_h", "kind0", "kind1", "kind2",
                                               "kind3", "kind4", "max_row", "max_col", "rows_wave", "cols_wave", "nnz_g")]

    def __repr__(self):
        return "SeInfo(%s)" % ", ".join("%s=%d" % (f, getattr(self, f)) for f, _ in self._fields_)


class SeLimits(C.Structure):
    """cs3_se_limits_t: the constants that shape the launches of the state-estimation kernels."""
    _fields_ = [(name, C.c_int64) for name in ("block", "grid_cap", "wave_row", "wave_col")]


class Cs3Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("cs3 error %d: %s" % (code, msg))
        self.code = code


class SingularMatrix(Cs3Error, ArithmeticError):
    """A static diagonal pivot was zero, non-finite or rejected by tol (CS3_ERR_PIVOT)."""


class NotPositiveDefinite(Cs3Error, ArithmeticError):
    """Cholesky met a non-positive pivot (CS3_ERR_NOT_SPD)."""


_lib = None


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64.so / libhsa-runtime64.so; the
    stream handles and device pointers that callers hand to this library (torch.cuda.current_stream(),
    Tensor.data_ptr()) only mean something to the runtime that made them, and a second runtime copy in the
    process does not even see the GPU once the first has opened it (measured on the GPU box: loading this
    library first and importing torch afterwards leaves torch with "No HIP GPUs are available").  So when
    torch is installed but not imported yet, its runtime is loaded here, globally, before our library: the
    loader then binds our libamdhip64.so.7 dependency to that copy, and a later `import torch` finds it too.
    Without torch the system ROCm runtime is used.  CS3_SYSTEM_HIP=1 skips this."""
    if "torch" in sys.modules or os.environ.get("CS3_SYSTEM_HIP") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                return


def lib():
    """Load the shared library; fail loudly when it has not been built."""
    global _lib
    if _lib is None:
        _share_torch_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C csparse3_amd/csrc` -- there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.cs3_last_error.restype = C.c_char_p
        vp = C.c_void_p
        L.cs3_analyze.argtypes = [I64, I64, I64, _i32p, _i32p, _i32p, I64, C.POINTER(vp)]
        L.cs3_match_scale.argtypes = [I64, _i32p, _i32p, _f64p, _i32p, _f64p, _f64p]
        L.cs3_analyze_matched.argtypes = [I64, I64, _i32p, _i32p, _f64p, _i32p, I64, C.POINTER(vp)]
        L.cs3_get_matching.argtypes = [vp, _i32p, _f64p, _f64p, C.POINTER(C.c_double)]
        L.cs3_analyze_schur.argtypes = [I64, I64, I64, _i32p, _i32p, _i32p, I64, I64, _i32p, C.POINTER(vp)]
        L.cs3_schur_info.argtypes = [vp, C.POINTER(I64), _i32p]
        L.cs3_schur_get_dev.argtypes = [vp, vp, vp]
        L.cs3_schur_get.argtypes = [vp, _f64p]
        for f in (L.cs3_schur_fwd_dev, L.cs3_schur_bwd_dev):
            f.argtypes = [vp, vp, I64, vp]
        for f in (L.cs3_schur_fwd, L.cs3_schur_bwd):
            f.argtypes = [vp, _f64p, I64]
        L.cs3_free.argtypes = [vp]
        L.cs3_get_info.argtypes = [vp, C.POINTER(Cs3Info)]
        L.cs3_get_ordering.argtypes = [vp] + [_i32p] * 6
        L.cs3_get_supernodes.argtypes = [vp] + [_i32p] * 3
        L.cs3_factor.argtypes = [vp, _f64p, C.c_double]
        L.cs3_factor_dev.argtypes = [vp, vp, C.c_double, vp]
        L.cs3_factor_status.argtypes = [vp, vp]
        L.cs3_factor_solve_dev.argtypes = [vp, vp, C.c_double, vp, I64, vp]
        L.cs3_factor_solve_bx_dev.argtypes = [vp, vp, C.c_double, vp, vp, I64, vp]
        for f in (L.cs3_solve, L.cs3_lsolve, L.cs3_usolve, L.cs3_solve_t, L.cs3_ltsolve, L.cs3_utsolve):
            f.argtypes = [vp, _f64p, I64]
        for f in (L.cs3_solve_dev, L.cs3_lsolve_dev, L.cs3_usolve_dev, L.cs3_solve_t_dev, L.cs3_ltsolve_dev, L.cs3_utsolve_dev):
            f.argtypes = [vp, vp, I64, vp]
        for f in (L.cs3_residual_dev, L.cs3_residual_t_dev):
            f.argtypes = [vp, vp, vp, vp, vp, I64, vp]
        for f in (L.cs3_matvec_dev, L.cs3_matvec_t_dev):
            f.argtypes = [vp, vp, vp, vp, I64, vp]
        for f in (L.cs3_refine_dev, L.cs3_refine_t_dev):
            f.argtypes = [vp, vp, vp, vp, I64, I64, C.POINTER(C.c_double), vp]
        L.cs3_refine.argtypes = [vp, _f64p, _f64p, _f64p, I64, I64, C.POINTER(C.c_double)]
        L.cs3_gmres_limits.argtypes = [C.POINTER(GmresLimits)]
        L.cs3_gmres_dev.argtypes = [vp, vp, vp, vp, I64, I64, I64, C.c_double, I64, _i32p, _f64p, vp]
        L.cs3_gmres.argtypes = [vp, _f64p, _f64p, _f64p, I64, I64, I64, C.c_double, I64, _i32p, _f64p]
        L.cs3_debug_gmres_estimates.argtypes = [vp, _f64p, I64]
        L.cs3_debug_gmres_kernel.argtypes = [vp, I64, I64, vp]
        L.cs3_debug_gmres_basis.argtypes = [vp, _f64p, I64]
        L.cs3_refine_xp_limits.argtypes = [C.POINTER(RefineXpLimits)]
        L.cs3_residual_xp_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, I64, I64, vp]
        L.cs3_residual_xp.argtypes = [vp, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, I64, I64]
        L.cs3_refine_xp_dev.argtypes = [vp, vp, vp, vp, vp, I64, I64, I64, _i32p, _i32p, _f64p, _f64p, _f64p, vp]
        L.cs3_refine_xp.argtypes = [vp, _f64p, _f64p, _f64p, _f64p, I64, I64, I64, _i32p, _i32p, _f64p, _f64p, _f64p]
        L.cs3_set_pivot_perturbation.argtypes = [vp, C.c_double]
        L.cs3_get_perturbed.argtypes = [vp, C.POINTER(I64), vp]
        L.cs3_condest_dev.argtypes = [vp, vp, vp, vp, vp]
        L.cs3_condest.argtypes = [vp, _f64p, _f64p, _f64p]
        L.cs3_slogdet_dev.argtypes = [vp, vp, vp, vp]
        L.cs3_slogdet.argtypes = [vp, _f64p, _f64p]
        L.cs3_updates_plan.argtypes = [vp, I64, _i32p, _i32p, _i32p, C.POINTER(vp)]
        L.cs3_updates_free.argtypes = [vp]
        L.cs3_updates_info.argtypes = [vp] + [C.POINTER(I64)] * 4
        L.cs3_updates_solve_dev.argtypes = [vp, vp, vp, vp, C.c_double, vp, vp, vp]
        L.cs3_updates_solve.argtypes = [vp, vp, _f64p, _f64p, C.c_double, _f64p, _f64p]
        L.cs3_debug_updates_tiles.argtypes = [vp] + [_i32p] * 4
        L.cs3_debug_updates_tiles.restype = I64
        L.cs3_debug_alloc_counters.argtypes = [vp, C.POINTER(I64), C.POINTER(I64)]
        L.cs3_sens_limits.argtypes = [C.POINTER(SensLimits)]
        L.cs3_sens_plan.argtypes = [vp, I64, _i32p, _i32p, I64, _i32p, _i32p, I64, I64, C.POINTER(vp)]
        L.cs3_sens_free.argtypes = [vp]
        L.cs3_sens_info.argtypes = [vp, C.POINTER(SensInfo)]
        L.cs3_sens_solve_dev.argtypes = [vp, vp, vp, vp, vp, vp]
        L.cs3_sens_solve.argtypes = [vp, vp, _f64p, _f64p, _f64p]
        L.cs3_debug_sens_parts.argtypes = [vp, vp, I64, vp, vp, vp, vp]
        L.cs3_debug_live_device_buffers.argtypes = []
        L.cs3_selinv_limits.argtypes = [C.POINTER(SelinvLimits)]
        L.cs3_selinv_dev.argtypes = [vp, vp]
        L.cs3_selinv_info.argtypes = [vp, C.POINTER(SelinvInfo)]
        L.cs3_selinv_entries_dev.argtypes = [vp, I64, vp, vp]
        L.cs3_selinv_diag_dev.argtypes = [vp, vp, vp]
        L.cs3_selinv_entries.argtypes = [vp, I64, _f64p]
        L.cs3_selinv_diag.argtypes = [vp, _f64p]
        L.cs3_selinv_factors.argtypes = [vp, I64, _f64p, _f64p]
        L.cs3_debug_selinv_plan.argtypes = [vp, _i32p, _i32p, C.POINTER(I64), C.POINTER(I64)]
        L.cs3_debug_selinv_plan.restype = I64
        L.cs3_debug_live_device_buffers.restype = I64
        L.cs3_quad_limits.argtypes = [C.POINTER(QuadLimits)]
        L.cs3_quad_plan.argtypes = [vp, I64, _i32p, _i32p, _i32p, _i32p, C.POINTER(vp)]
        L.cs3_quad_free.argtypes = [vp]
        L.cs3_quad_info.argtypes = [vp, C.POINTER(QuadInfo)]
        L.cs3_quad_dev.argtypes = [vp, vp, vp, vp, vp, vp]
        L.cs3_quad.argtypes = [vp, vp, _f64p, _f64p, _f64p]
        L.cs3_quad_normres_dev.argtypes = [vp, vp, vp, vp, vp, C.c_double, vp, vp, vp, vp, vp]
        L.cs3_quad_normres.argtypes = [vp, vp, _f64p, _f64p, _f64p, C.c_double, _f64p, _f64p, _f64p, _f64p]
        L.cs3_debug_quad_plan.argtypes = [vp, _i32p, C.POINTER(I64), C.POINTER(I64)]
        L.cs3_export_factor_dev.argtypes = [vp, vp, vp]
        L.cs3_import_factor_dev.argtypes = [vp, vp, vp]
        L.cs3_get_factors.argtypes = [vp, I64, _i32p, _i32p, _f64p, _i32p, _i32p, _f64p]
        L.cs3_amd.argtypes = [I64, I64, I64, _i32p, _i32p, _i32p]
        L.cs3_etree.argtypes = [I64, _i32p, _i32p, _i32p]
        L.cs3_post.argtypes = [I64, _i32p, _i32p]
        L.cs3_counts.argtypes = [I64, _i32p, _i32p, _i32p, _i32p, _i32p]
        L.cs3_csc_lsolve.argtypes = [I64, _i32p, _i32p, _f64p, _f64p, I64]
        L.cs3_csc_usolve.argtypes = [I64, _i32p, _i32p, _f64p, _f64p, I64]
        L.cs3_csc_ltsolve.argtypes = [I64, _i32p, _i32p, _f64p, _f64p, I64]
        L.cs3_csc_utsolve.argtypes = [I64, _i32p, _i32p, _f64p, _f64p, I64]
        L.cs3_csc_matvec.argtypes = [I64, I64, _i32p, _i32p, _f64p, _f64p, _f64p, I64]
        L.cs3_csc_stack_4_by_4.argtypes = [I64, I64, _i32p, _i32p, _f64p] * 4 + [_i32p, _i32p, _f64p]
        L.cs3_csc_stack_4_by_4_dev.argtypes = [I64, I64, I64, vp, vp, vp] * 4 + [vp, vp, vp, vp, vp]
        L.cs3_restack_values_dev.argtypes = [I64, vp, I64, I64, I64, vp, vp, vp, vp, vp, vp]
        L.cs3_csc_transpose.argtypes = [I64, I64, _i32p, _i32p, _f64p, _i32p, _i32p, _f64p]
        L.cs3_coo_to_csc.argtypes = [I64, I64, I64, _i32p, _i32p, _f64p, _i32p, _i32p, _f64p]
        L.cs3_csc_norm.argtypes = [I64, _i32p, _f64p, C.POINTER(C.c_double)]
        L.cs3_csc_add.argtypes = [I64, I64, _i32p, _i32p, _f64p, _i32p, _i32p, _f64p, C.c_double, C.c_double, _i32p, _i32p, _f64p]
        L.cs3_csc_sub_matrix.argtypes = [I64, _i32p, _i32p, _f64p, _i32p, I64, _i32p, I64, _i32p, _i32p, _f64p, I64]
        L.cs3_find_islands.argtypes = [I64, _i32p, _i32p, _i32p]
        L.cs3_spgemm_limits.argtypes = [C.POINTER(SpgemmLimits)]
        L.cs3_spgemm_plan_create.argtypes = [I64, I64, _i32p, _i32p, I64, I64, _i32p, _i32p, C.c_int, C.POINTER(vp)]
        L.cs3_spgemm_plan_free.argtypes = [vp]
        L.cs3_spgemm_plan_info.argtypes = [vp, C.POINTER(SpgemmInfo)]
        L.cs3_spgemm_plan_pattern.argtypes = [vp, _i32p, _i32p]
        L.cs3_spgemm_plan_pattern_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.cs3_spgemm_values_dev.argtypes = [vp, vp, vp, vp, vp]
        L.cs3_spgemm_values.argtypes = [vp, _f64p, _f64p, _f64p]
        pp = C.POINTER(_i32p)
        L.cs3_union_limits.argtypes = [C.POINTER(UnionLimits)]
        L.cs3_union_plan_create.argtypes = [I64, I64, pp, pp, C.POINTER(vp)]
        L.cs3_union_plan_free.argtypes = [vp]
        L.cs3_union_plan_info.argtypes = [vp, C.POINTER(UnionInfo)]
        L.cs3_union_plan_pattern.argtypes = [vp, _i32p, _i32p]
        L.cs3_union_plan_offsets.argtypes = [vp, C.POINTER(I64)]
        L.cs3_union_plan_slots.argtypes = [vp, I64, _i32p]
        L.cs3_union_upload.argtypes = [vp]
        L.cs3_union_values_dev.argtypes = [vp, vp, vp, vp]
        L.cs3_union_values.argtypes = [vp, _f64p, _f64p]
        L.cs3_cplx_limits.argtypes = [C.POINTER(CplxLimits)]
        L.cs3_cplx_plan_create.argtypes = [I64, _i32p, _i32p, I64, I64, C.POINTER(vp)]
        L.cs3_cplx_plan_free.argtypes = [vp]
        L.cs3_cplx_plan_info.argtypes = [vp, C.POINTER(CplxInfo)]
        L.cs3_cplx_plan_pattern.argtypes = [vp, _i32p, _i32p]
        L.cs3_cplx_plan_order.argtypes = [vp, I64, _i32p, _i32p]
        L.cs3_cplx_upload.argtypes = [vp]
        L.cs3_cplx_workspace_dev.argtypes = [vp, I64, I64, C.POINTER(vp)]
        L.cs3_cplx_values_dev.argtypes = [vp, vp, vp, vp]
        L.cs3_cplx_pack_dev.argtypes = [vp, I64, vp, vp, I64, vp]
        L.cs3_cplx_unpack_dev.argtypes = [vp, I64, vp, vp, I64, I64, vp]
        L.cs3_cplx_residual_dev.argtypes = [vp, I64, vp, vp, vp, vp, I64, vp]
        L.cs3_cplx_rotation_dev.argtypes = [vp, C.POINTER(vp)]
        L.cs3_cplx_values.argtypes = [vp, _f64p, _f64p]
        L.cs3_cplx_pack.argtypes = [vp, I64, _f64p, _f64p, I64]
        L.cs3_cplx_unpack.argtypes = [vp, I64, _f64p, _f64p, I64, I64]
        L.cs3_cplx_residual.argtypes = [vp, I64, _f64p, _f64p, _f64p, _f64p, I64]
        L.cs3_cplx_rotation.argtypes = [vp, _f64p]
        L.cs3_debug_sens_tile.argtypes = [vp, I64, _f64p, I64]
        L.cs3_cplx_sens_limits.argtypes = [C.POINTER(SensLimits)]
        L.cs3_cplx_sens_plan.argtypes = [vp, vp, I64, _i32p, _i32p, I64, _i32p, _i32p, I64, I64, C.POINTER(vp)]
        L.cs3_cplx_sens_free.argtypes = [vp]
        L.cs3_cplx_sens_info.argtypes = [vp, C.POINTER(SensInfo)]
        L.cs3_cplx_sens_solve_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.cs3_cplx_sens_solve.argtypes = [vp, vp, vp, _f64p, _f64p, _f64p]
        L.cs3_debug_cplx_sens_parts.argtypes = [vp, vp, vp, I64, vp, vp, vp, vp]
        L.cs3_cplx_updates_limits.argtypes = [C.POINTER(CplxUpdatesLimits)]
        L.cs3_cplx_updates_plan.argtypes = [vp, vp, I64, _i32p, _i32p, _i32p, C.POINTER(vp)]
        L.cs3_cplx_updates_free.argtypes = [vp]
        L.cs3_cplx_updates_info.argtypes = [vp] + [C.POINTER(I64)] * 4
        L.cs3_debug_cplx_updates_tiles.argtypes = [vp] + [_i32p] * 4
        L.cs3_debug_cplx_updates_tiles.restype = I64
        L.cs3_cplx_updates_solve_dev.argtypes = [vp, vp, vp, vp, vp, C.c_double, vp, vp, vp]
        L.cs3_cplx_updates_solve.argtypes = [vp, vp, vp, _f64p, _f64p, C.c_double, _f64p, _f64p]
        L.cs3_debug_cplx_updates_parts.argtypes = [vp, vp, vp, I64, vp, vp, C.c_double, vp, vp, vp]
        L.cs3_cplx_plan_create_schur.argtypes =[I64, _i32p, _i32p, I64, I64, I64, _i32p, C.POINTER(vp)]
        L.cs3_cplx_plan_schur_info.argtypes = [vp, C.POINTER(I64), _i32p]
        L.cs3_cplx_plan_schur_order.argtypes = [vp, I64, _i32p, _i32p, _i32p]
        L.cs3_cplx_schur_get_dev.argtypes = [vp, vp, vp, vp]
        L.cs3_cplx_schur_get.argtypes = [vp, vp, _f64p]
        L.cs3_cplx_selinv_limits.argtypes = [C.POINTER(CplxSelinvLimits)]
        L.cs3_cplx_selinv_entries_dev.argtypes = [vp, vp, I64, vp, vp]
        L.cs3_cplx_selinv_diag_dev.argtypes = [vp, vp, vp, vp]
        L.cs3_cplx_selinv_thevenin_dev.argtypes = [vp, vp, vp, vp]
        L.cs3_cplx_selinv_entries.argtypes = [vp, vp, I64, _f64p]
        L.cs3_cplx_selinv_diag.argtypes = [vp, vp, _f64p]
        L.cs3_cplx_selinv_thevenin.argtypes = [vp, vp, _f64p]
        L.cs3_debug_cplx_selinv_maps.argtypes = [vp, vp] + [C.POINTER(I64)] * 3
        L.cs3_pf_limits.argtypes = [C.POINTER(PfLimits)]
        L.cs3_pf_plan_create.argtypes = [I64, _i32p, _i32p, I64, _i32p, I64, _i32p, I64, I64, I64, C.POINTER(vp)]
        L.cs3_pf_plan_free.argtypes = [vp]
        L.cs3_pf_handle.argtypes = [vp, C.POINTER(vp)]
        L.cs3_pf_plan_info.argtypes = [vp, C.POINTER(PfInfo)]
        L.cs3_pf_plan_pattern.argtypes = [vp, _i32p, _i32p]
        L.cs3_pf_plan_maps.argtypes = [vp] + [_i32p] * 6
        L.cs3_pf_mismatch_dev.argtypes = [vp] * 8
        L.cs3_pf_jacobian_dev.argtypes = [vp] * 6
        L.cs3_pf_solve_dev.argtypes = [vp, vp, vp, vp, vp, C.c_double, I64, I64, C.c_double, _i32p, _f64p, _i32p, vp]
        L.cs3_pf_mismatch.argtypes = [vp] + [_f64p] * 6
        L.cs3_pf_jacobian.argtypes = [vp] + [_f64p] * 4
        L.cs3_pf_solve.argtypes = [vp, _f64p, _f64p, _f64p, _f64p, C.c_double, I64, I64, C.c_double, _i32p, _f64p, _i32p]
        pi32, pdbl = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        L.cs3_se_limits.argtypes = [C.POINTER(SeLimits)]
        L.cs3_se_plan_create.argtypes = [I64, _i32p, _i32p, I64, _i32p, I64, _i32p, _i32p, I64, _i32p, _i32p, I64, C.POINTER(vp)]
        L.cs3_se_plan_free.argtypes = [vp]
        L.cs3_se_plan_info.argtypes = [vp, C.POINTER(SeInfo)]
        L.cs3_se_plan_pattern.argtypes = [vp] + [_i32p] * 4
        L.cs3_se_plan_maps.argtypes = [vp] + [_i32p] * 3
        L.cs3_se_handle.argtypes = [vp, C.POINTER(vp)]
        L.cs3_se_gain_pattern.argtypes = [vp, _i32p, _i32p]
        L.cs3_se_residuals_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.cs3_se_measure_dev.argtypes = [vp] * 10
        L.cs3_se_jacobian_dev.argtypes = [vp] * 10
        L.cs3_se_gradient_dev.argtypes = [vp] * 5
        L.cs3_se_solve_dev.argtypes = [vp] * 7 + [C.c_double, I64, pi32, pdbl, pdbl, pi32, vp]
        L.cs3_se_baddata_dev.argtypes = [vp] * 7 + [C.c_double] + [vp] * 5
        L.cs3_se_measure.argtypes = [vp] + [_f64p] * 8
        L.cs3_se_jacobian.argtypes = [vp] + [_f64p] * 8
        L.cs3_se_solve.argtypes = [vp] + [_f64p] * 6 + [C.c_double, I64, pi32, pdbl, pdbl, pi32]
        L.cs3_se_baddata.argtypes = [vp] + [_f64p] * 6 + [C.c_double] + [_f64p] * 4
        _lib = L
    return _lib


def _check(rc):
    if rc == 0:
        return
    msg = lib().cs3_last_error().decode("utf-8", "replace")
    if rc == -4:
        raise SingularMatrix(rc, msg)
    if rc == -5:
        raise NotPositiveDefinite(rc, msg)
    raise Cs3Error(rc, msg)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _pi(a):
    return None if a is None else a.ctypes.data_as(_i32p)


def _pf(a):
    return None if a is None else a.ctypes.data_as(_f64p)


def device_count():
    return int(lib().cs3_device_count())


def gmres_limits():
    """The constants of the GMRES refinement (cs3_gmres_limits); needs no GPU."""
    out = GmresLimits()
    _check(lib().cs3_gmres_limits(C.byref(out)))
    return out


def refine_xp_limits():
    """The constants of the extra-precise refinement (cs3_refine_xp_limits); needs no GPU."""
    out = RefineXpLimits()
    _check(lib().cs3_refine_xp_limits(C.byref(out)))
    return out


def debug_live_device_buffers():
    """Device blocks the library holds right now, over all handles, plans and calls (process-wide; 0 when all are freed)."""
    return int(lib().cs3_debug_live_device_buffers())


# ------------------------------------------------------ ordering / symbolic --

def csc_amd_f(order, m, n, Ap, Ai):
    """q = amd(A + A') (order 1) or the natural order (order 0)."""
    Ap, Ai = _i32(Ap), _i32(Ai)
    q = np.empty(n, dtype=np.int32)
    _check(lib().cs3_amd(order, m, n, _pi(Ap), _pi(Ai), _pi(q)))
    return q


def csc_etree_f(n, Ap, Ai):
    """Elimination tree of the symmetric matrix whose UPPER triangle is (Ap, Ai)."""
    Ap, Ai = _i32(Ap), _i32(Ai)
    parent = np.empty(n, dtype=np.int32)
    _check(lib().cs3_etree(n, _pi(Ap), _pi(Ai), _pi(parent)))
    return parent


def csc_post_f(n, parent):
    parent = _i32(parent)
    post = np.empty(n, dtype=np.int32)
    _check(lib().cs3_post(n, _pi(parent), _pi(post)))
    return post


def csc_counts_f(n, Ap, Ai, parent, post):
    Ap, Ai, parent, post = _i32(Ap), _i32(Ai), _i32(parent), _i32(post)
    cc = np.empty(n, dtype=np.int32)
    _check(lib().cs3_counts(n, _pi(Ap), _pi(Ai), _pi(parent), _pi(post), _pi(cc)))
    return cc


def match_scale(n, Ap, Ai, Ax):
    """Maximum-product transversal with scalings (MC64 job 5), on the host: -> (rowperm, dr, dc) with
    B[rowinv[i], j] = (dr[i] * A[i, j]) * dc[j], |B| <= 1 and |B[j, j]| = 1; rowperm[j] is the row of A matched to column j.
    SingularMatrix when A has no full transversal (stored zeros count as absent)."""
    Ap, Ai, Ax = _i32(Ap), _i32(Ai), _f64(Ax)
    rowperm = np.empty(n, dtype=np.int32)
    dr, dc = np.empty(n), np.empty(n)
    _check(lib().cs3_match_scale(n, _pi(Ap), _pi(Ai), _pf(Ax), _pi(rowperm), _pf(dr), _pf(dc)))
    return rowperm, dr, dc


# ------------------------------------------------------------------ handle --

class UpdatesInfo:
    """What cs3_updates_info reports: cases, distinct touched rows over all cases, largest rank, tiles."""

    def __init__(self, ncases, nrows_unique, max_rank, ntiles):
        self.ncases, self.nrows_unique, self.max_rank, self.ntiles = ncases, nrows_unique, max_rank, ntiles

    def __repr__(self):
        return "UpdatesInfo(ncases=%d, nrows_unique=%d, max_rank=%d, ntiles=%d)" % (
            self.ncases, self.nrows_unique, self.max_rank, self.ntiles)


def _flat_cases(cases):
    """(cp, ci, cj) from a list of (rows, cols) index arrays per case, or the flat triple itself."""
    if isinstance(cases, tuple) and len(cases) == 3 and np.ndim(cases[0]) == 1 and not isinstance(cases[0], tuple):
        cp, ci, cj = (_i32(a) for a in cases)
        return cp, ci, cj
    rows = [_i32(np.atleast_1d(c[0])) for c in cases]
    cols = [_i32(np.atleast_1d(c[1])) for c in cases]
    for r, c in zip(rows, cols):
        assert r.shape == c.shape and r.ndim == 1, "a case is (rows, cols) of equal length"
    cp = np.zeros(len(rows) + 1, dtype=np.int32)
    np.cumsum([len(r) for r in rows], out=cp[1:])
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, dtype=np.int32)   # noqa: E731
    return cp, cat(rows), cat(cols)


class UpdatesPlan:
    """The pattern of a list of sparse modifications dA_c of a handle's matrix (Factorization.updates_plan): made once on
    the host, used by every solve_updates of that handle, across refactorisations."""

    def __init__(self, factorization, cases):
        self._u = C.c_void_p()
        self.cp, self.ci, self.cj = _flat_cases(cases)
        self.ncases = len(self.cp) - 1
        _check(lib().cs3_updates_plan(factorization._h, self.ncases, _pi(self.cp), _pi(self.ci), _pi(self.cj),
                                      C.byref(self._u)))

    def close(self):
        if self._u:
            lib().cs3_updates_free(self._u)
            self._u = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def info(self):
        out = [I64() for _ in range(4)]
        _check(lib().cs3_updates_info(self._u, *[C.byref(o) for o in out]))
        return UpdatesInfo(*[int(o.value) for o in out])

    def tiles(self):
        """-> int32 [ntiles, 4]: first case, cases, touched rows and solve width of every tile (diagnostic)."""
        nt = self.info.ntiles
        arrs = [np.empty(nt, dtype=np.int32) for _ in range(4)]
        assert lib().cs3_debug_updates_tiles(self._u, *[_pi(a) for a in arrs]) == nt
        return np.stack(arrs, axis=1)


SENS_SIDES = {"auto": 0, "right": 1, "left": 2}


def sens_limits():
    """The constants of the sparse right-hand-side path (cs3_sens_limits); needs no GPU."""
    out = SensLimits()
    _check(lib().cs3_sens_limits(C.byref(out)))
    return out


def selinv_limits():
    """The constants of the selected inversion (cs3_selinv_limits); needs no GPU."""
    out = SelinvLimits()
    _check(lib().cs3_selinv_limits(C.byref(out)))
    return out


def quad_limits():
    """The constants of the bilinear forms on the selected inverse (cs3_quad_limits); needs no GPU."""
    out = QuadLimits()
    _check(lib().cs3_quad_limits(C.byref(out)))
    return out


class QuadPlan:
    """The term map of m bilinear forms t_i = c_i' A^-1 b_i on a handle's selected inverse (Factorization.quad_plan): made
    once on the host from the analysis alone, used by every quad_forms / normalized_residuals of that handle, across
    refactorisations."""

    def __init__(self, factorization, Ct, Bt=None):
        self._u = C.c_void_p()
        self.m, self.ctp, self.cti = int(Ct[0]), _i32(Ct[1]), _i32(Ct[2])
        assert self.ctp.size == self.m + 1, "Ct is (nrows, indptr[nrows + 1], indices)"
        self.btp, self.bti = (None, None) if Bt is None else (_i32(Bt[1]), _i32(Bt[2]))
        assert Bt is None or (int(Bt[0]) == self.m and self.btp.size == self.m + 1), "Bt is (nrows, indptr[nrows + 1], indices), nrows that of Ct"
        self.nnz_c = int(self.ctp[-1])
        self.nnz_b = self.nnz_c if Bt is None else int(self.btp[-1])
        _check(lib().cs3_quad_plan(factorization._h, self.m, _pi(self.ctp), _pi(self.cti), _pi(self.btp), _pi(self.bti),
                                   C.byref(self._u)))

    def close(self):
        if self._u:
            lib().cs3_quad_free(self._u)
            self._u = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def info(self):
        out = QuadInfo()
        _check(lib().cs3_quad_info(self._u, C.byref(out)))
        return out

    def debug_plan(self):
        """Diagnostics -> (row_class [m], term_ptr [m + 1], term_pos [terms]): the class of every row (0 lane, 1 wave,
        2 workgroup) and the offsets in the handle's block of Z of its terms, a-major; needs no GPU."""
        row_class = np.empty(self.m, dtype=np.int32)
        term_ptr = np.empty(self.m + 1, dtype=np.int64)
        term_pos = np.empty(int(self.info.nterms), dtype=np.int64)
        _check(lib().cs3_debug_quad_plan(self._u, _pi(row_class), term_ptr.ctypes.data_as(C.POINTER(I64)),
                                         term_pos.ctypes.data_as(C.POINTER(I64))))
        return row_class, term_ptr, term_pos


class SensPlan:
    """The patterns of B and C' of Y = C op(A)^-1 B on a handle (Factorization.sens_plan): made once on the host, used by
    every sens_solve of that handle, across refactorisations."""

    def __init__(self, factorization, B, Ct=None, side="auto", trans=False):
        self._u = C.c_void_p()
        n = factorization.n
        self.k, self.bp, self.bi = (n, None, None) if B is None else (int(B[0]), _i32(B[1]), _i32(B[2]))
        self.p, self.ctp, self.cti = (n, None, None) if Ct is None else (int(Ct[0]), _i32(Ct[1]), _i32(Ct[2]))
        assert self.bp is None or self.bp.size == self.k + 1, "B is (ncols, indptr[ncols + 1], indices)"
        assert self.ctp is None or self.ctp.size == self.p + 1, "Ct is (ncols, indptr[ncols + 1], indices)"
        _check(lib().cs3_sens_plan(factorization._h, self.k, _pi(self.bp), _pi(self.bi), self.p, _pi(self.ctp), _pi(self.cti),
                                   SENS_SIDES.get(side, side), int(bool(trans)), C.byref(self._u)))

    def close(self):
        if self._u:
            lib().cs3_sens_free(self._u)
            self._u = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def info(self):
        out = SensInfo()
        _check(lib().cs3_sens_info(self._u, C.byref(out)))
        return out


class Factorization:
    """Device-resident factorisation handle: analyze once, (re)factor, solve.

    kind: CS3_LU or CS3_CHOLESKY.  order: ORDER_NATURAL / ORDER_AMD, or pass q.
    batch: number of matrices sharing the pattern (values [batch, nnz]).
    match_values (LU only): values Ax[nnz] of ONE representative matrix; the handle then permutes rows by their
    maximum-product transversal and scales (match_scale) before the analysis and factorises B = P (Dr A Dc), for matrices
    without a strong diagonal (zero diagonals, saddle-point systems, bad scaling).  Values, right-hand sides and solutions
    stay in terms of A; order / q, tol, factors() and ordering() refer to B.  The matching is kept across refactorisations.
    set_perturbation (LU only): pivots smaller than delta are replaced by +delta instead of stopping the factorisation;
    perturbed() counts them and refine() removes the error from a solution.
    schur: indices of the variables that are NOT eliminated (a Schur handle, cs3_analyze_schur).  factor() then factorises
    the interior and holds the dense Schur complement S = A22 - A21 A11^-1 A12 on that set, in the order of the list:
    schur(), schur_forward(), schur_backward().  order / q refer to the interior; slogdet() is that of A11; solve() and
    everything else that would answer for the full matrix raise Cs3Error.  Not together with match_values.
    """

    def __init__(self, m, n, Ap, Ai, kind=CS3_LU, order=ORDER_AMD, q=None, batch=1, match_values=None, schur=None):
        assert m == n, "square matrix required"
        self._h = C.c_void_p()
        self.kind = kind
        self.n = int(n)
        self.batch = int(batch)
        Ap, Ai = _i32(Ap), _i32(Ai)
        self.nnz = int(Ap[n])
        qa = None
        if q is not None:
            qa = _i32(q)
            order = ORDER_GIVEN
        self.matched = match_values is not None
        self.perturbation = 0.0
        self.ns = 0
        if schur is not None:
            assert not self.matched, "a Schur set and a matching exclude each other"
            idx = _i32(schur).reshape(-1)
            _check(lib().cs3_analyze_schur(kind, order, n, _pi(Ap), _pi(Ai), _pi(qa), batch, idx.size, _pi(idx), C.byref(self._h)))
            self.ns = int(idx.size)
        elif self.matched:
            assert kind == CS3_LU, "matching is for LU handles"
            mv = _f64(match_values).reshape(-1)
            assert mv.size >= self.nnz
            _check(lib().cs3_analyze_matched(order, n, _pi(Ap), _pi(Ai), _pf(mv), _pi(qa), batch, C.byref(self._h)))
        else:
            _check(lib().cs3_analyze(kind, order, n, _pi(Ap), _pi(Ai), _pi(qa), batch, C.byref(self._h)))

    _borrowed = False                 # a handle lent by a plan that owns it (PowerFlowPlan.factorization): never freed here

    @classmethod
    def _borrow(cls, handle, n, nnz, batch):
        self = cls.__new__(cls)
        self._h = C.c_void_p(handle)
        self._borrowed = True
        self.kind, self.n, self.nnz, self.batch = CS3_LU, int(n), int(nnz), int(batch)
        self.matched, self.perturbation, self.ns = False, 0.0, 0
        return self

    def close(self):
        if self._h:
            if not self._borrowed:
                lib().cs3_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def info(self):
        out = Cs3Info()
        _check(lib().cs3_get_info(self._h, C.byref(out)))
        return out

    def ordering(self):
        """-> dict(q_amd, parent, post, colcount, q, pinv), all int32[n]."""
        names = ("q_amd", "parent", "post", "colcount", "q", "pinv")
        arrs = [np.empty(self.n, dtype=np.int32) for _ in names]
        _check(lib().cs3_get_ordering(self._h, *[_pi(a) for a in arrs]))
        return dict(zip(names, arrs))

    def matching(self):
        """-> (rowperm, dr, dc) of a matched handle, as match_scale returns them (Cs3Error on a plain handle)."""
        rowperm = np.empty(self.n, dtype=np.int32)
        dr, dc = np.empty(self.n), np.empty(self.n)
        _check(lib().cs3_get_matching(self._h, _pi(rowperm), _pf(dr), _pf(dc), None))
        return rowperm, dr, dc

    @property
    def match_time(self):
        """Host seconds the matching took (next to info.t_order_s)."""
        t = C.c_double(0.0)
        _check(lib().cs3_get_matching(self._h, None, None, None, C.byref(t)))
        return float(t.value)

    def supernodes(self):
        ns = int(self.info.nsuper)
        sn_ptr = np.empty(ns + 1, dtype=np.int32)
        sn_parent = np.empty(ns, dtype=np.int32)
        sn_level = np.empty(ns, dtype=np.int32)
        _check(lib().cs3_get_supernodes(self._h, _pi(sn_ptr), _pi(sn_parent), _pi(sn_level)))
        return sn_ptr, sn_parent, sn_level

    # -- Schur complements (a handle made with schur=...)
    def schur_info(self):
        """-> int32[ns]: the Schur set in the order of S's rows and columns (Cs3Error on a plain handle)."""
        ns = I64()
        _check(lib().cs3_schur_info(self._h, C.byref(ns), None))
        idx = np.empty(int(ns.value), dtype=np.int32)
        _check(lib().cs3_schur_info(self._h, None, _pi(idx)))
        return idx

    def schur(self):
        """The Schur complement of the last factorisation: [ns, ns], or [batch, ns, ns]; S[i, j] belongs to
        (schur_idx[i], schur_idx[j]).  Cholesky: the full symmetric matrix."""
        S = np.empty((self.batch, self.ns, self.ns))
        _check(lib().cs3_schur_get(self._h, _pf(S)))
        return S[0] if self.batch == 1 else S

    def schur_dev(self, s_ptr, stream=0):
        """schur() into device memory [batch][ns, ns], asynchronous on `stream`."""
        _check(lib().cs3_schur_get_dev(self._h, C.c_void_p(s_ptr), C.c_void_p(stream)))

    def schur_forward(self, b):
        """b: [n], [n, k] or [batch, n, k] in A's rows.  -> a new array whose Schur rows hold b2 - A21 A11^-1 b1 (the
        right-hand side of S x2 = g); the interior rows are the half-solved interior, to be passed on to schur_backward."""
        return self._sweep(lib().cs3_schur_fwd, b)

    def schur_backward(self, y):
        """y: what schur_forward returned, with the Schur rows replaced by x2.  -> the solution of A x = b."""
        return self._sweep(lib().cs3_schur_bwd, y)

    def schur_forward_dev(self, x_ptr, k=1, stream=0):
        _check(lib().cs3_schur_fwd_dev(self._h, C.c_void_p(x_ptr), k, C.c_void_p(stream)))

    def schur_backward_dev(self, x_ptr, k=1, stream=0):
        _check(lib().cs3_schur_bwd_dev(self._h, C.c_void_p(x_ptr), k, C.c_void_p(stream)))

    # -- static pivot perturbation
    def set_perturbation(self, delta):
        """LU pivots with |p| < delta become +delta from the next factorisation on (0: off, the default).  On a matched
        handle delta refers to B, where |B| <= 1.  The factors are then those of A(q, q) + diag(E): solutions need
        refine(), and slogdet / condest describe the perturbed matrix."""
        _check(lib().cs3_set_pivot_perturbation(self._h, float(delta)))
        self.perturbation = float(delta)
        return self

    def perturbed(self, stream=0):
        """-> int64[batch]: the pivots the last factorisation replaced, per matrix (synchronises `stream`)."""
        count = np.zeros(self.batch, dtype=np.int64)
        _check(lib().cs3_get_perturbed(self._h, count.ctypes.data_as(C.POINTER(I64)), C.c_void_p(stream)))
        return count

    # -- numeric, host arrays
    def factor(self, Ax, tol=0.0):
        Ax = _f64(Ax)
        assert Ax.size >= self.batch * self.nnz
        _check(lib().cs3_factor(self._h, _pf(Ax), tol))
        return self

    def solve(self, b, trans=False):
        """Solve A x = b (trans: A' x = b, on the same factors).  b: [n], [n, k] or [batch, n, k]; returns a new array."""
        x = np.array(b, dtype=np.float64, order="C", copy=True)
        per = self.batch * self.n
        assert x.size % per == 0, "right-hand side does not match [batch,] n [, k]"
        _check((lib().cs3_solve_t if trans else lib().cs3_solve)(self._h, _pf(x), x.size // per))
        return x

    def refine(self, Ax, b, x, steps=1):
        """`steps` rounds of x += A \\ (b - A x) with the held factors and the values Ax (host arrays; the bits of
        refine_dev).  -> (the refined x, a new array; max |dx| of the last round)."""
        Ax, b = _f64(Ax), _f64(b)
        x = np.array(x, dtype=np.float64, order="C", copy=True)
        per = self.batch * self.n
        assert Ax.size >= self.batch * self.nnz and x.size % per == 0 and b.size == x.size
        out = C.c_double(0.0)
        _check(lib().cs3_refine(self._h, _pf(Ax), _pf(b), _pf(x), x.size // per, steps, C.byref(out)))
        return x, float(out.value)

    def gmres(self, Ax, b, x0=None, rtol=1e-12, restart=30, max_iters=100, trans=False):
        """Restarted GMRES(restart) on A x = b (trans: A' x = b) with the values Ax, right-preconditioned with the held
        factors: converges where refine() diverges (factors of an earlier iterate, a large perturbation).  b: [n], [n, k]
        or [batch, n, k]; every column is a system of its own.  x0=None starts from solve(b, trans).
        -> (x, iters int32[batch * k], relres float64[batch * k]: the true final ||b - A x|| / ||b|| of every system)."""
        Ax, b = _f64(Ax), _f64(b)
        x = self.solve(b, trans) if x0 is None else np.array(x0, dtype=np.float64, order="C", copy=True)
        per = self.batch * self.n
        assert Ax.size >= self.batch * self.nnz and x.size % per == 0 and b.size == x.size
        k = x.size // per
        iters = np.zeros(self.batch * k, dtype=np.int32)
        relres = np.zeros(self.batch * k)
        _check(lib().cs3_gmres(self._h, _pf(Ax), _pf(b), _pf(x), k, restart, max_iters, rtol, 1 if trans else 0,
                               _pi(iters), _pf(relres)))
        return x, iters, relres

    def gmres_dev(self, ax_ptr, b_ptr, x_ptr, k=1, rtol=1e-12, restart=30, max_iters=100, stream=0, trans=False):
        """gmres on device pointers: X at x_ptr holds x0 on entry and the solution on exit.  Host-driven: synchronises
        `stream` after every iteration (one 4-byte read).  The same bits as gmres().  -> (iters, relres)."""
        iters = np.zeros(self.batch * k, dtype=np.int32)
        relres = np.zeros(self.batch * k)
        _check(lib().cs3_gmres_dev(self._h, C.c_void_p(ax_ptr), C.c_void_p(b_ptr), C.c_void_p(x_ptr), k, restart, max_iters,
                                   rtol, 1 if trans else 0, _pi(iters), _pf(relres), C.c_void_p(stream)))
        return iters, relres

    def debug_gmres_estimates(self, count):
        """The recurrence's residual estimate every system of the last gmres call ended its last cycle with (diagnostic)."""
        est = np.zeros(count)
        _check(lib().cs3_debug_gmres_estimates(self._h, _pf(est), count))
        return est

    def debug_gmres_basis(self, nvec, k):
        """The first nvec <= restart + 1 basis vectors as the last gmres call (with k right-hand sides) left them
        (diagnostic) -> [nvec, batch, n, k].  Vector 0 is what the call's closing residual check left."""
        V = np.zeros((nvec, self.batch, self.n, k))
        _check(lib().cs3_debug_gmres_basis(self._h, _pf(V), nvec))
        return V

    def residual_xp(self, Ax, b, x, xt=None, trans=False):
        """r = b - A (x + xt) (trans: with A') accumulated in doubled precision and rounded once, and
        s = |b| + |A| |x|, on host arrays (cs3_residual_xp; needs the analysis only).  -> (r, s), shaped like b."""
        Ax, b, x = _f64(Ax), _f64(b), _f64(x)
        xt = None if xt is None else _f64(xt)
        per = self.batch * self.n
        assert Ax.size >= self.batch * self.nnz and b.size % per == 0 and x.size == b.size
        assert xt is None or xt.size == b.size
        r, s = np.empty_like(b), np.empty_like(b)
        _check(lib().cs3_residual_xp(self._h, _pf(Ax), _pf(b), _pf(x), _pf(xt), _pf(r), _pf(s), b.size // per,
                                     1 if trans else 0))
        return r, s

    def refine_xp(self, Ax, b, x=None, max_iters=10, trans=False, want_tail=False):
        """Extra-precise refinement of A x = b (trans: A' x = b) with the values Ax on the held factors: residuals in
        doubled precision, x carried as a head and a tail (LAPACK's xGERFSX).  b: [n], [n, k] or [batch, n, k]; every
        column is a system of its own.  x=None starts from solve(b, trans).
        -> (x, info): info["iters"], ["flag"] (0 still iterating after max_iters, 1 converged, 2 stalled, 3 non-finite),
        ["ferr"] (bound on the normwise relative error, infinity norm), ["berr"] (componentwise backward error of x) and
        ["rate"], [batch * k] each; with want_tail info["xt"], x + xt being the solution in doubled precision."""
        Ax, b = _f64(Ax), _f64(b)
        x = self.solve(b, trans) if x is None else np.array(x, dtype=np.float64, order="C", copy=True)
        per = self.batch * self.n
        assert Ax.size >= self.batch * self.nnz and x.size % per == 0 and b.size == x.size
        k = x.size // per
        info = self._xp_info(k)
        xt = np.zeros_like(x) if want_tail else None
        _check(lib().cs3_refine_xp(self._h, _pf(Ax), _pf(b), _pf(x), _pf(xt), k, max_iters, 1 if trans else 0,
                                   _pi(info["iters"]), _pi(info["flag"]), _pf(info["ferr"]), _pf(info["berr"]), _pf(info["rate"])))
        if want_tail:
            info["xt"] = xt
        return x, info

    def refine_xp_dev(self, ax_ptr, b_ptr, x_ptr, k=1, max_iters=10, xt_ptr=0, stream=0, trans=False):
        """refine_xp on device pointers: X at x_ptr holds x0 on entry and the refined head on exit, xt_ptr (optional)
        receives the tail.  Host-driven: synchronises `stream` after every pass (one 4-byte read).  The same bits as
        refine_xp().  -> info."""
        info = self._xp_info(k)
        _check(lib().cs3_refine_xp_dev(self._h, C.c_void_p(ax_ptr), C.c_void_p(b_ptr), C.c_void_p(x_ptr),
                                       C.c_void_p(xt_ptr) if xt_ptr else None, k, max_iters, 1 if trans else 0,
                                       _pi(info["iters"]), _pi(info["flag"]), _pf(info["ferr"]), _pf(info["berr"]),
                                       _pf(info["rate"]), C.c_void_p(stream)))
        return info

    def residual_xp_dev(self, ax_ptr, b_ptr, x_ptr, r_ptr, s_ptr=0, xt_ptr=0, k=1, stream=0, trans=False):
        """residual_xp on device pointers, asynchronous on `stream` (s_ptr, xt_ptr optional)."""
        _check(lib().cs3_residual_xp_dev(self._h, C.c_void_p(ax_ptr), C.c_void_p(b_ptr), C.c_void_p(x_ptr),
                                         C.c_void_p(xt_ptr) if xt_ptr else None, C.c_void_p(r_ptr),
                                         C.c_void_p(s_ptr) if s_ptr else None, k, 1 if trans else 0, C.c_void_p(stream)))

    def _xp_info(self, k):
        nsys = self.batch * k
        return {"iters": np.zeros(nsys, dtype=np.int32), "flag": np.zeros(nsys, dtype=np.int32), "ferr": np.zeros(nsys),
                "berr": np.zeros(nsys), "rate": np.zeros(nsys)}

    def solve_refined(self, Ax, b, max_refine=10, refine="stationary"):
        """solve(b), then -- when the factorisation replaced pivots -- refinement.  refine="stationary": one round at a
        time until the correction no longer falls below half of the one before, at most max_refine rounds (a round whose
        correction GREW is dropped).  refine="gmres": gmres() from solve(b) with max_iters = max_refine, which also
        converges when the perturbation is too large for the stationary rounds.
        Without replaced pivots these two are solve(b), bit for bit.
        refine="extra": solve(b), then refine_xp() with max_iters = max_refine, with or without replaced pivots."""
        assert refine in ("stationary", "gmres", "extra")
        if refine == "extra":
            return self.refine_xp(Ax, b, max_iters=max_refine)[0]
        x = self.solve(b)
        if not self.perturbed().any():
            return x
        if refine == "gmres":
            return self.gmres(Ax, b, x0=x, max_iters=max_refine)[0]
        prev = np.inf
        for _ in range(max_refine):
            x_new, corr = self.refine(Ax, b, x, 1)
            if not corr <= prev:
                break
            x = x_new
            if not corr < 0.5 * prev:
                break
            prev = corr
        return x

    def _sweep(self, fn, x):
        x = np.array(x, dtype=np.float64, order="C", copy=True)
        per = self.batch * self.n
        assert x.size % per == 0
        _check(fn(self._h, _pf(x), x.size // per))
        return x

    def lsolve(self, x):
        """x = L \\ x in pivot order (cs_lsolve on this factorisation's L)."""
        return self._sweep(lib().cs3_lsolve, x)

    def usolve(self, x):
        """x = U \\ x in pivot order (cs_usolve; L' for Cholesky, i.e. cs_ltsolve)."""
        return self._sweep(lib().cs3_usolve, x)

    def ltsolve(self, x):
        """x = L' \\ x in pivot order (cs_ltsolve; unit diagonal for LU, the same as usolve for Cholesky)."""
        return self._sweep(lib().cs3_ltsolve, x)

    def utsolve(self, x):
        """x = U' \\ x in pivot order (cs_utsolve; Cs3Error on a Cholesky handle)."""
        return self._sweep(lib().cs3_utsolve, x)

    # -- numeric, device pointers (e.g. torch.Tensor.data_ptr()) on a HIP stream
    def factor_dev(self, ax_ptr, tol=0.0, stream=0):
        _check(lib().cs3_factor_dev(self._h, C.c_void_p(ax_ptr), tol, C.c_void_p(stream)))

    def factor_solve_dev(self, ax_ptr, x_ptr, k=1, tol=0.0, stream=0):
        """(Re)factorise and solve in one call (cs_lusol on resident data); X is overwritten."""
        _check(lib().cs3_factor_solve_dev(self._h, C.c_void_p(ax_ptr), tol, C.c_void_p(x_ptr), k, C.c_void_p(stream)))

    def factor_solve_bx_dev(self, ax_ptr, b_ptr, x_ptr, k=1, tol=0.0, stream=0):
        """The same out of place: right-hand sides at b_ptr stay as they are, solutions go to x_ptr."""
        _check(lib().cs3_factor_solve_bx_dev(self._h, C.c_void_p(ax_ptr), tol, C.c_void_p(b_ptr), C.c_void_p(x_ptr), k, C.c_void_p(stream)))

    def factor_status(self, stream=0):
        _check(lib().cs3_factor_status(self._h, C.c_void_p(stream)))

    def solve_dev(self, x_ptr, k=1, stream=0, trans=False):
        fn = lib().cs3_solve_t_dev if trans else lib().cs3_solve_dev
        _check(fn(self._h, C.c_void_p(x_ptr), k, C.c_void_p(stream)))

    def lsolve_dev(self, x_ptr, k=1, stream=0):
        _check(lib().cs3_lsolve_dev(self._h, C.c_void_p(x_ptr), k, C.c_void_p(stream)))

    def usolve_dev(self, x_ptr, k=1, stream=0):
        _check(lib().cs3_usolve_dev(self._h, C.c_void_p(x_ptr), k, C.c_void_p(stream)))

    def ltsolve_dev(self, x_ptr, k=1, stream=0):
        _check(lib().cs3_ltsolve_dev(self._h, C.c_void_p(x_ptr), k, C.c_void_p(stream)))

    def utsolve_dev(self, x_ptr, k=1, stream=0):
        _check(lib().cs3_utsolve_dev(self._h, C.c_void_p(x_ptr), k, C.c_void_p(stream)))

    def residual_dev(self, ax_ptr, b_ptr, x_ptr, r_ptr, k=1, stream=0, trans=False):
        """R = B - A X (trans: B - A' X) on resident data (A's values at ax_ptr, the analysed pattern); csc_mat_vec_ff's
        summation order."""
        fn = lib().cs3_residual_t_dev if trans else lib().cs3_residual_dev
        _check(fn(self._h, C.c_void_p(ax_ptr), C.c_void_p(b_ptr), C.c_void_p(x_ptr), C.c_void_p(r_ptr), k, C.c_void_p(stream)))

    def matvec_dev(self, ax_ptr, x_ptr, y_ptr, k=1, stream=0, trans=False):
        """Y = A X (trans: A' X) on resident data (the analysed pattern, values at ax_ptr), summed as csc_mat_vec_ff sums."""
        fn = lib().cs3_matvec_t_dev if trans else lib().cs3_matvec_dev
        _check(fn(self._h, C.c_void_p(ax_ptr), C.c_void_p(x_ptr), C.c_void_p(y_ptr), k, C.c_void_p(stream)))

    def refine_dev(self, ax_ptr, b_ptr, x_ptr, k=1, steps=1, stream=0, want_correction=True, trans=False):
        """`steps` rounds of x += A \\ (b - A x) (trans: x += A^-T (b - A' x)) with the factors at hand; returns max |dx|
        of the last round."""
        out = C.c_double(0.0)
        fn = lib().cs3_refine_t_dev if trans else lib().cs3_refine_dev
        _check(fn(self._h, C.c_void_p(ax_ptr), C.c_void_p(b_ptr), C.c_void_p(x_ptr), k, steps,
                  C.byref(out) if want_correction else None, C.c_void_p(stream)))
        return float(out.value)

    # -- reliability of the held factors
    def condest(self, Ax):
        """1-norm condition estimates of every matrix of the batch from the held factors (LAPACK dlacn2, ITMAX 5):
        -> (cond, inv_norm), float64[batch] each.  inv_norm estimates ||A^-1||_1; cond = ||A||_1 * inv_norm with ||A||_1
        summed from Ax ([batch, nnz] in the analysed entry order) as csc_norm sums it.  Runs only the solves some matrix
        still needs, synchronising after each."""
        Ax = _f64(Ax)
        assert Ax.size >= self.batch * self.nnz
        cond = np.empty(self.batch)
        inv_norm = np.empty(self.batch)
        _check(lib().cs3_condest(self._h, _pf(Ax), _pf(cond), _pf(inv_norm)))
        return cond, inv_norm

    def condest_dev(self, ax_ptr, cond_ptr, inv_norm_ptr=0, stream=0):
        """condest on device pointers, asynchronous on `stream` (a fixed sequence of 11 solves, no synchronisation); the
        same bits as condest().  inv_norm_ptr = 0: not written."""
        _check(lib().cs3_condest_dev(self._h, C.c_void_p(ax_ptr), C.c_void_p(cond_ptr), C.c_void_p(inv_norm_ptr),
                                     C.c_void_p(stream)))

    def slogdet(self):
        """(sign, log|det A|) of every matrix of the batch from the pivots of the held factors, float64[batch] each
        (numpy.linalg.slogdet's convention: a zero pivot gives (0, -inf))."""
        sign = np.empty(self.batch)
        logabs = np.empty(self.batch)
        _check(lib().cs3_slogdet(self._h, _pf(sign), _pf(logabs)))
        return sign, logabs

    def slogdet_dev(self, sign_ptr, logabs_ptr, stream=0):
        _check(lib().cs3_slogdet_dev(self._h, C.c_void_p(sign_ptr), C.c_void_p(logabs_ptr), C.c_void_p(stream)))

    # -- many low-rank-modified systems on the held factors
    def updates_plan(self, cases):
        """Plan for solving (A + dA_c) x = b for a list of sparse modifications: `cases` is a list of (rows, cols) index
        arrays (the positions of each case's triplets; duplicates add) or the flat (cp, ci, cj).  Needs no GPU.
        -> UpdatesPlan (.info, .close(), context manager)."""
        return UpdatesPlan(self, cases)

    def solve_updates(self, plan, cx, b, sing_tol=0.0):
        """x_c = (A + dA_c)^-1 b for every case of `plan` from the held factors (Sherman-Morrison-Woodbury, no
        refactorisation): cx the values of all triplets in the plan's order, b [n].  -> (X [n, ncases], rpiv [ncases]);
        rpiv is the smallest pivot of the case's capacitance matrix relative to its largest entry, and a case with
        rpiv <= sing_tol (A + dA_c singular) has a NaN column."""
        cx, b = _f64(cx).reshape(-1), _f64(b).reshape(-1)
        assert cx.size == int(plan.cp[-1]) and b.size == self.n
        X = np.empty((self.n, plan.ncases))
        rpiv = np.empty(plan.ncases)
        _check(lib().cs3_updates_solve(self._h, plan._u, _pf(cx), _pf(b), sing_tol, _pf(X), _pf(rpiv)))
        return X, rpiv

    def solve_updates_dev(self, plan, cx_ptr, b_ptr, x_ptr, rpiv_ptr=0, sing_tol=0.0, stream=0):
        """solve_updates on device pointers, asynchronous on `stream`; X [n, ncases] row-major.  After the first call
        with a plan nothing is allocated and nothing synchronises.  The same bits as solve_updates()."""
        _check(lib().cs3_updates_solve_dev(self._h, plan._u, C.c_void_p(cx_ptr), C.c_void_p(b_ptr), sing_tol,
                                           C.c_void_p(x_ptr), C.c_void_p(rpiv_ptr), C.c_void_p(stream)))

    # -- sparse right-hand sides on the held factors
    def sens_plan(self, B, Ct=None, side="auto", trans=False):
        """Plan for Y = C op(A)^-1 B with sparse B (n x k) and C (p x n): `B` = (k, indptr, indices) by columns, `Ct` =
        (p, indptr, indices) the CSC pattern of C' (C by rows); None is the identity (not both).  side "auto" solves
        for the fewer of k and p columns, "right" for columns of B, "left" for rows of C.  Needs no GPU.
        -> SensPlan (.info, .close(), context manager)."""
        return SensPlan(self, B, Ct, side, trans)

    def sens_solve(self, plan, Bx, Ctx):
        """Y [p, k] = C op(A)^-1 B from the held factors: Bx / Ctx the values in the plan's entry order (None for an
        identity operand)."""
        Bx = None if plan.bp is None else _f64(Bx).reshape(-1)
        Ctx = None if plan.ctp is None else _f64(Ctx).reshape(-1)
        assert Bx is None or Bx.size == int(plan.bp[-1])
        assert Ctx is None or Ctx.size == int(plan.ctp[-1])
        Y = np.empty((plan.p, plan.k))
        _check(lib().cs3_sens_solve(self._h, plan._u, _pf(Bx), _pf(Ctx), _pf(Y)))
        return Y

    def sens_solve_dev(self, plan, bx_ptr, ctx_ptr, y_ptr, stream=0):
        """sens_solve on device pointers, asynchronous on `stream`; Y [p, k] row-major.  After the first call with a plan
        nothing is allocated and nothing synchronises.  The same bits as sens_solve()."""
        _check(lib().cs3_sens_solve_dev(self._h, plan._u, C.c_void_p(bx_ptr), C.c_void_p(ctx_ptr), C.c_void_p(y_ptr),
                                        C.c_void_p(stream)))

    def debug_sens_parts(self, plan, parts, bx_ptr, ctx_ptr, y_ptr, stream=0):
        """Diagnostics, for timing: the steps of sens_solve_dev in the mask `parts` (1 scatter, 2 solves, 4 combine)."""
        _check(lib().cs3_debug_sens_parts(self._h, plan._u, parts, C.c_void_p(bx_ptr), C.c_void_p(ctx_ptr), C.c_void_p(y_ptr),
                                          C.c_void_p(stream)))

    def debug_sens_tile(self, shape, write=None):
        """Diagnostics, for tests: the front of the tile buffer of the sens paths as an array of `shape` (synchronises); with
        `write` that array goes INTO the buffer instead."""
        a = np.empty(shape) if write is None else np.ascontiguousarray(write, dtype=np.float64).reshape(shape)
        _check(lib().cs3_debug_sens_tile(self._h, 0 if write is None else 1, _pf(a), a.size))
        return a

    # -- selected inversion: A^-1 on the pattern of L + U from the held factors
    def selinv(self, stream=0):
        """Compute Z = A^-1 on the pattern of L + U into memory the handle owns, asynchronously on `stream` (one pass over
        the assembly tree, parents first).  Any later factorisation invalidates it."""
        _check(lib().cs3_selinv_dev(self._h, C.c_void_p(stream or 0)))

    def selinv_info(self):
        """-> SelinvInfo: sizes of the plan of the selected inversion; needs no GPU."""
        out = SelinvInfo()
        _check(lib().cs3_selinv_info(self._h, C.byref(out)))
        return out

    def selinv_plan(self):
        """Diagnostics -> (front, launch, entry_map, diag_map): supernodes in the order they are computed, the launch of
        each, the offset in Z of A^-1(Ai[p], j) per entry of A and of A^-1(i, i) per i; needs no GPU."""
        ns = int(self.info.nsuper)
        front, launch = np.empty(ns, dtype=np.int32), np.empty(ns, dtype=np.int32)
        emap, dmap = np.empty(self.nnz, dtype=np.int64), np.empty(self.n, dtype=np.int64)
        got = lib().cs3_debug_selinv_plan(self._h, _pi(front), _pi(launch), emap.ctypes.data_as(C.POINTER(I64)),
                                          dmap.ctypes.data_as(C.POINTER(I64)))
        if got < 0:
            _check(CS3_ERR_ARG)
        assert got == ns
        return front, launch, emap, dmap

    def inverse_entries(self, trans=False):
        """A^-1 at the stored positions of A: [batch, nnz] (1-D for one matrix), entry p of column j = A^-1(Ai[p], j), with
        `trans` A^-1(j, Ai[p]).  Runs selinv() first when the handle holds no inverse of the current factors."""
        Zx = np.empty((self.batch, self.nnz))
        _check(lib().cs3_selinv_entries(self._h, 1 if trans else 0, _pf(Zx)))
        return Zx[0] if self.batch == 1 else Zx

    def inverse_diagonal(self):
        """diag(A^-1) in the caller's labels: [batch, n] (1-D for one matrix); computes like inverse_entries."""
        d = np.empty((self.batch, self.n))
        _check(lib().cs3_selinv_diag(self._h, _pf(d)))
        return d[0] if self.batch == 1 else d

    def inverse_on_factors(self, b=0):
        """-> (Zl, Zu): Z = (Q' A Q)^-1 of matrix b at the positions of factors()' (Lp, Li) and (Up, Ui), in their labels
        (Zu None for Cholesky); computes like inverse_entries."""
        inf = self.info
        Zl = np.empty(inf.nnz_l)
        Zu = np.empty(inf.nnz_u) if self.kind == CS3_LU else None
        _check(lib().cs3_selinv_factors(self._h, b, _pf(Zl), _pf(Zu)))
        return Zl, Zu

    # -- bilinear forms on the selected inverse: t_i = c_i' A^-1 b_i, the bad-data test of a state estimate
    def quad_plan(self, Ct, Bt=None):
        """Plan for t_i = c_i' A^-1 b_i, i < m: `Ct` = (m, indptr, indices) the CSC pattern of C' (C by rows), `Bt` the same
        for B; None: B = C, pattern and values.  Every pair of a row's columns must lie on the pattern of L + U (the pairs
        of one row of H always do for A = H' W H).  Needs no GPU.  -> QuadPlan (.info, .close(), context manager)."""
        return QuadPlan(self, Ct, Bt)

    def _quad_values(self, a, count):
        a = _f64(a).reshape(self.batch, -1)
        assert a.shape[1] == count, "values are [batch, %d] in the plan's entry order" % count
        return a

    def quad_forms(self, plan, Cx, Bx=None):
        """t [batch, m] (1-D for one matrix) from the held selected inverse: Cx / Bx the values [batch, nnz] in the plan's
        entry order (Bx is ignored for a plan with B = C).  Runs selinv() first when the handle holds no inverse of the
        current factors."""
        Cx = self._quad_values(Cx, plan.nnz_c)
        Bx = None if plan.btp is None else self._quad_values(Bx, plan.nnz_b)
        t = np.empty((self.batch, plan.m))
        _check(lib().cs3_quad(self._h, plan._u, _pf(Cx), _pf(Bx), _pf(t)))
        return t[0] if self.batch == 1 else t

    def quad_forms_dev(self, plan, cx_ptr, bx_ptr, t_ptr, stream=0):
        """quad_forms on device pointers, asynchronous on `stream`, after selinv(); t [batch, m].  After the first call with
        a plan nothing is allocated and nothing synchronises.  The same bits as quad_forms()."""
        _check(lib().cs3_quad_dev(self._h, plan._u, C.c_void_p(cx_ptr), C.c_void_p(bx_ptr or 0), C.c_void_p(t_ptr),
                                  C.c_void_p(stream or 0)))

    def normalized_residuals(self, plan, Hx, w, r, crit_tol=1e-8):
        """The largest-normalised-residual test on a handle that holds the factors of G = H' W H, `plan` made from the
        rows of H (B = C): t_i = h_i' G^-1 h_i, omega_i = 1/w_i - t_i, rn_i = |r_i| / sqrt(omega_i), and rn_i = 0 for a
        critical measurement (1 - w_i t_i <= crit_tol).  Hx [batch, nnz], w and r [batch, m].
        -> (rn, info), info = {"omega", "t", "worst", "worst_row", "J", "critical"}; J = sum w r^2.  Arrays are 1-D and the
        others scalars for one matrix, [batch, ...] otherwise.  Ties take the lowest row; a NaN rn ranks first."""
        Hx = self._quad_values(Hx, plan.nnz_c)
        w, r = self._quad_values(w, plan.m), self._quad_values(r, plan.m)
        t, omega, rn = (np.empty((self.batch, plan.m)) for _ in range(3))
        summary = np.empty((self.batch, 4))
        _check(lib().cs3_quad_normres(self._h, plan._u, _pf(Hx), _pf(w), _pf(r), float(crit_tol), _pf(t), _pf(omega), _pf(rn),
                                      _pf(summary)))
        info = {"omega": omega, "t": t, "worst": summary[:, 0].copy(), "worst_row": summary[:, 1].astype(np.int64),
                "J": summary[:, 2].copy(), "critical": summary[:, 3].astype(np.int64)}
        if self.batch == 1:
            rn = rn[0]
            info = {k: (v[0] if v.ndim == 2 else v[0].item()) for k, v in info.items()}
        return rn, info

    def normalized_residuals_dev(self, plan, hx_ptr, w_ptr, r_ptr, crit_tol, summary_ptr, t_ptr=0, omega_ptr=0, rn_ptr=0, stream=0):
        """normalized_residuals on device pointers, asynchronous on `stream`, after selinv(): summary [batch, 4] = (worst,
        worst_row, J, critical) as doubles; t, omega, rn [batch, m] are written where a pointer is given.  The same bits."""
        _check(lib().cs3_quad_normres_dev(self._h, plan._u, C.c_void_p(hx_ptr), C.c_void_p(w_ptr), C.c_void_p(r_ptr), float(crit_tol),
                                          C.c_void_p(t_ptr or 0), C.c_void_p(omega_ptr or 0), C.c_void_p(rn_ptr or 0),
                                          C.c_void_p(summary_ptr), C.c_void_p(stream or 0)))

    def debug_alloc_counters(self):
        """(device allocations incl. graph instantiations, host synchronisations) the handle's solves have made so far."""
        a, s = I64(), I64()
        _check(lib().cs3_debug_alloc_counters(self._h, C.byref(a), C.byref(s)))
        return int(a.value), int(s.value)

    def export_factor_dev(self, dst_ptr, stream=0):
        """Copy the factor panels (info.factor_bytes per matrix) into an HBM buffer."""
        _check(lib().cs3_export_factor_dev(self._h, C.c_void_p(dst_ptr), C.c_void_p(stream)))

    def import_factor_dev(self, src_ptr, stream=0):
        """Install factor panels produced by another handle with the same analysis."""
        _check(lib().cs3_import_factor_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(stream)))

    def factors(self, b=0, values=True):
        """-> (Lp, Li, Lx, Up, Ui, Ux) in CSparse form (U parts None for Cholesky)."""
        inf = self.info
        n = self.n
        Lp = np.empty(n + 1, dtype=np.int32)
        Li = np.empty(inf.nnz_l, dtype=np.int32)
        Lx = np.empty(inf.nnz_l, dtype=np.float64) if values else None
        if self.kind == CS3_LU:
            Up = np.empty(n + 1, dtype=np.int32)
            Ui = np.empty(inf.nnz_u, dtype=np.int32)
            Ux = np.empty(inf.nnz_u, dtype=np.float64) if values else None
        else:
            Up = Ui = Ux = None
        _check(lib().cs3_get_factors(self._h, b, _pi(Lp), _pi(Li), _pf(Lx), _pi(Up), _pi(Ui), _pf(Ux)))
        return Lp, Li, Lx, Up, Ui, Ux


# ---------------------------------------------- flat functions, reference style --

def csc_lu_f(m, n, Ap, Ai, Ax, tol=0.0, order=ORDER_AMD, q=None):
    """LU with static diagonal pivots in a fill-reducing order: P A Q = L U.

    -> (Lp, Li, Lx, Up, Ui, Ux, pinv, q).  L unit lower with the diagonal
    first in each column, U upper with the diagonal last (cs_lu's layout).
    """
    with Factorization(m, n, Ap, Ai, CS3_LU, order, q) as F:
        F.factor(Ax, tol)
        Lp, Li, Lx, Up, Ui, Ux = F.factors()
        o = F.ordering()
    return Lp, Li, Lx, Up, Ui, Ux, o["pinv"], o["q"]


def csc_chol_f(m, n, Ap, Ai, Ax, order=ORDER_AMD, q=None):
    """Cholesky P A P' = L L'.  -> (Lp, Li, Lx, pinv)."""
    with Factorization(m, n, Ap, Ai, CS3_CHOLESKY, order, q) as F:
        F.factor(Ax)
        Lp, Li, Lx, _, _, _ = F.factors()
        o = F.ordering()
    return Lp, Li, Lx, o["pinv"]


def _tri(fn, n, Gp, Gi, Gx, x):
    Gp, Gi, Gx = _i32(Gp), _i32(Gi), _f64(Gx)
    assert isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous
    assert x.shape[0] == n
    k = 1 if x.ndim == 1 else x.shape[1]
    _check(fn(n, _pi(Gp), _pi(Gi), _pf(Gx), _pf(x), k))


def csc_lsolve_f(n, Lp, Li, Lx, x):
    """x = L \\ x in place; L lower triangular CSC, diagonal first per column."""
    _tri(lib().cs3_csc_lsolve, n, Lp, Li, Lx, x)


def csc_usolve_f(n, Up, Ui, Ux, x):
    """x = U \\ x in place; U upper triangular CSC, diagonal last per column."""
    _tri(lib().cs3_csc_usolve, n, Up, Ui, Ux, x)


def csc_ltsolve_f(n, Lp, Li, Lx, x):
    """x = L' \\ x in place; L lower triangular CSC, diagonal first per column (cs_ltsolve)."""
    _tri(lib().cs3_csc_ltsolve, n, Lp, Li, Lx, x)


def csc_utsolve_f(n, Up, Ui, Ux, x):
    """x = U' \\ x in place; U upper triangular CSC, diagonal last per column (cs_utsolve)."""
    _tri(lib().cs3_csc_utsolve, n, Up, Ui, Ux, x)


def perturbation_delta(perturb, Ax, match):
    """The delta behind a `perturb` argument: True means sqrt(eps), times max |Ax| unless the handle is matched (B is
    scaled to |B| <= 1); a number is taken as it is; False / 0: off."""
    if perturb is True:
        scale = 1.0 if match else float(np.abs(_f64(Ax)).max(initial=0.0))
        return float(np.sqrt(np.finfo(np.float64).eps)) * scale
    return float(perturb or 0.0)


def csc_lusol_f(order, m, n, Ap, Ai, Ax, b, tol=0.0, match=False, perturb=0.0, max_refine=10, refine="stationary"):
    """x = A \\ b by LU (cs_lusol).  match: rows permuted and scaled by the maximum-product transversal first (matrices
    without a strong diagonal).  perturb: pivots below delta are replaced instead of rejected (perturbation_delta), and
    the solution is refined (Factorization.solve_refined, at most max_refine rounds; refine="gmres": GMRES on the held
    factors instead of the stationary rounds).  refine="extra": the solve is followed by the extra-precise refinement
    (Factorization.refine_xp, at most max_refine corrections), with or without perturb."""
    with Factorization(m, n, Ap, Ai, CS3_LU, order, match_values=Ax if match else None) as F:
        delta = perturbation_delta(perturb, Ax, match)
        if delta == 0.0:
            F.factor(Ax, tol)
            return F.solve_refined(Ax, b, max_refine, refine) if refine == "extra" else F.solve(b)
        return F.set_perturbation(delta).factor(Ax, tol).solve_refined(Ax, b, max_refine, refine)


def csc_cholsol_f(order, m, n, Ap, Ai, Ax, b):
    """x = A \\ b by Cholesky (cs_cholsol)."""
    with Factorization(m, n, Ap, Ai, CS3_CHOLESKY, order) as F:
        return F.factor(Ax).solve(b)


def csc_mat_vec_ff(m, n, Ap, Ai, Ax, x):
    """y = A x on the device (csc_numba.py:309-328); x [n] or [n, k] row-major."""
    Ap, Ai, Ax, x = _i32(Ap), _i32(Ai), _f64(Ax), _f64(x)
    assert x.shape[0] == n
    k = 1 if x.ndim == 1 else x.shape[1]
    y = np.empty((m,) if x.ndim == 1 else (m, k), dtype=np.float64)
    _check(lib().cs3_csc_matvec(m, n, _pi(Ap), _pi(Ai), _pf(Ax), _pf(x), _pf(y), k))
    return y


def csc_stack_4_by_4_ff(am, an, Ai, Ap, Ax, bm, bn, Bi, Bp, Bx, cm, cn, Ci, Cp, Cx, dm, dn, Di, Dp, Dx):
    """[[A, B], [C, D]] on the device; argument and return order (m, n, indices, indptr, data) as the
    reference's csc_stack_4_by_4_ff (csc_numba.py:640-720)."""
    assert am == bm and cm == dm and an == cn and bn == dn          # csc_numba.py:679-682
    a = [_i32(Ai), _i32(Ap), _f64(Ax), _i32(Bi), _i32(Bp), _f64(Bx), _i32(Ci), _i32(Cp), _f64(Cx), _i32(Di), _i32(Dp), _f64(Dx)]
    nnz = int(a[1][an]) + int(a[4][bn]) + int(a[7][cn]) + int(a[10][dn])
    Pi = np.empty(nnz, dtype=np.int32); Pp = np.empty(an + bn + 1, dtype=np.int32); Px = np.empty(nnz, dtype=np.float64)
    _check(lib().cs3_csc_stack_4_by_4(am, an, _pi(a[0]), _pi(a[1]), _pf(a[2]), bm, bn, _pi(a[3]), _pi(a[4]), _pf(a[5]),
                                      cm, cn, _pi(a[6]), _pi(a[7]), _pf(a[8]), dm, dn, _pi(a[9]), _pi(a[10]), _pf(a[11]),
                                      _pi(Pi), _pi(Pp), _pf(Px)))
    return am + cm, an + bn, Pi, Pp, Px


def csc_stack_4_by_4_dev(blocks, Pi_ptr, Pp_ptr, Px_ptr, map_ptr=0, stream=0):
    """csc_stack_4_by_4_ff on arrays that already live in HBM.  blocks = [(m, n, nnz, indices_ptr, indptr_ptr, data_ptr)] * 4
    for A, B, C, D (device addresses, e.g. torch.Tensor.data_ptr()); outputs are device addresses too.  Asynchronous on
    `stream`; nothing crosses PCIe.  map_ptr (optional, int32[nnz]) receives the restack map for restack_values_dev."""
    args = []
    for (m, n, nnz, pi, pp, px) in blocks:
        args += [m, n, nnz, C.c_void_p(pi), C.c_void_p(pp), C.c_void_p(px)]
    _check(lib().cs3_csc_stack_4_by_4_dev(*args, C.c_void_p(Pi_ptr), C.c_void_p(Pp_ptr), C.c_void_p(Px_ptr),
                                          C.c_void_p(map_ptr), C.c_void_p(stream)))


def restack_values_dev(nnz, map_ptr, nnz_a, nnz_b, nnz_c, ax_ptr, bx_ptr, cx_ptr, dx_ptr, px_ptr, stream=0):
    """Px[p] = (A | B | C | D)[map[p]]: the values-only restack of a Newton iteration (patterns unchanged)."""
    _check(lib().cs3_restack_values_dev(nnz, C.c_void_p(map_ptr), nnz_a, nnz_b, nnz_c, C.c_void_p(ax_ptr), C.c_void_p(bx_ptr),
                                        C.c_void_p(cx_ptr), C.c_void_p(dx_ptr), C.c_void_p(px_ptr), C.c_void_p(stream)))


# ---- format conversions and utilities on the device ------------------------
# Names, argument order and return shapes of the reference's own kernels (csc_numba.py); outputs are
# bit-identical with them, output order included.

def csc_transpose(m, n, Ap, Ai, Ax):
    """C = A' -> (n, m, Cp, Ci, Cx) as csc_transpose (csc_numba.py:400-436): m and n swapped in the result."""
    Ap, Ai, Ax = _i32(Ap), _i32(Ai), _f64(Ax)
    nnz = int(Ap[n])
    Cp = np.empty(m + 1, dtype=np.int32); Ci = np.empty(nnz, dtype=np.int32); Cx = np.empty(nnz, dtype=np.float64)
    _check(lib().cs3_csc_transpose(m, n, _pi(Ap), _pi(Ai), _pf(Ax), _pi(Cp), _pi(Ci), _pf(Cx)))
    return n, m, Cp, Ci, Cx


def csc_to_csr(m, n, Ap, Ai, Ax, Bp, Bi, Bx):
    """CSR arrays of A written into the caller's Bp[m + 1], Bi[nnz], Bx[nnz], as csc_to_csr (csc_numba.py:360-397)."""
    Ap, Ai, Ax = _i32(Ap), _i32(Ai), _f64(Ax)
    for a, t in ((Bp, np.int32), (Bi, np.int32), (Bx, np.float64)):
        assert isinstance(a, np.ndarray) and a.dtype == t and a.flags.c_contiguous
    _check(lib().cs3_csc_transpose(m, n, _pi(Ap), _pi(Ai), _pf(Ax), _pi(Bp), _pi(Bi), _pf(Bx)))


def coo_to_csc(m, n, Ti, Tj, Tx, nz):
    """Triplets -> (m, n, Cp, Ci, Cx); duplicates kept, triplet order inside a column (csc_numba.py:331-357)."""
    Ti, Tj, Tx = _i32(Ti), _i32(Tj), _f64(Tx)
    Cp = np.empty(n + 1, dtype=np.int32); Ci = np.empty(nz, dtype=np.int32); Cx = np.empty(nz, dtype=np.float64)
    _check(lib().cs3_coo_to_csc(m, n, nz, _pi(Ti), _pi(Tj), _pf(Tx), _pi(Cp), _pi(Ci), _pf(Cx)))
    return m, n, Cp, Ci, Cx


def csc_norm(n, Ap, Ax):
    """1-norm (csc_numba.py:723-739)."""
    Ap, Ax = _i32(Ap), _f64(Ax)
    out = C.c_double(0.0)
    _check(lib().cs3_csc_norm(n, _pi(Ap), _pf(Ax), C.byref(out)))
    return float(out.value)


def csc_add_ff(Am, An, Ap, Ai, Ax, Bm, Bn, Bp, Bi, Bx, alpha, beta):
    """C = alpha A + beta B -> (m, n, Cp, Ci, Cx) as csc_add_ff (csc_numba.py:183-219)."""
    assert Am == Bm and An == Bn
    Ap, Ai, Ax, Bp, Bi, Bx = _i32(Ap), _i32(Ai), _f64(Ax), _i32(Bp), _i32(Bi), _f64(Bx)
    cap = int(Ap[An]) + int(Bp[Bn])
    Cp = np.empty(An + 1, dtype=np.int32); Ci = np.empty(max(cap, 1), dtype=np.int32); Cx = np.empty(max(cap, 1), dtype=np.float64)
    _check(lib().cs3_csc_add(Am, An, _pi(Ap), _pi(Ai), _pf(Ax), _pi(Bp), _pi(Bi), _pf(Bx), alpha, beta, _pi(Cp), _pi(Ci), _pf(Cx)))
    nz = int(Cp[An])
    return Am, An, Cp, Ci[:nz].copy(), Cx[:nz].copy()


def spgemm_limits():
    """The constants that separate the paths of the sparse product (cs3_spgemm_limits); needs no GPU."""
    out = SpgemmLimits()
    _check(lib().cs3_spgemm_limits(C.byref(out)))
    return out


class SpgemmPlan:
    """C = A B, or C = A' B with transpose_a, for fixed patterns: the pattern of C and the list of products behind every
    entry are worked out once on the device, values() / values_dev() then refresh Cx as often as the values change
    (cs3_spgemm_plan_create).  Pattern and values are those of the reference's csc_multiply_ff, bit for bit; with
    transpose_a those of csc_transpose followed by csc_multiply_ff, read from A's own value array."""

    def __init__(self, Am, An, Ap, Ai, Bm, Bn, Bp, Bi, transpose_a=False):
        self._p = C.c_void_p()
        Ap, Ai, Bp, Bi = _i32(Ap), _i32(Ai), _i32(Bp), _i32(Bi)
        _check(lib().cs3_spgemm_plan_create(Am, An, _pi(Ap), _pi(Ai), Bm, Bn, _pi(Bp), _pi(Bi), 1 if transpose_a else 0,
                                            C.byref(self._p)))
        inf = self.info
        self.m, self.n, self.nnz = int(inf.m), int(inf.n), int(inf.nnz_c)
        self.nnz_a, self.nnz_b = int(inf.nnz_a), int(inf.nnz_b)

    def close(self):
        if self._p:
            lib().cs3_spgemm_plan_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def info(self):
        out = SpgemmInfo()
        _check(lib().cs3_spgemm_plan_info(self._p, C.byref(out)))
        return out

    def pattern(self):
        """-> (Cp int32[n + 1], Ci int32[nnz]) on the host."""
        Cp = np.empty(self.n + 1, dtype=np.int32)
        Ci = np.empty(self.nnz, dtype=np.int32)
        _check(lib().cs3_spgemm_plan_pattern(self._p, _pi(Cp), _pi(Ci)))
        return Cp, Ci

    def _pattern_dev(self):
        cp, ci = C.c_void_p(), C.c_void_p()
        _check(lib().cs3_spgemm_plan_pattern_dev(self._p, C.byref(cp), C.byref(ci)))
        return cp.value or 0, ci.value or 0

    @property
    def cp_ptr(self):
        """Device address of Cp (int32[n + 1]), valid until close()."""
        return self._pattern_dev()[0]

    @property
    def ci_ptr(self):
        """Device address of Ci (int32[nnz]), valid until close()."""
        return self._pattern_dev()[1]

    def values(self, Ax, Bx):
        """-> Cx float64[nnz] from host value arrays in the patterns' entry order."""
        Ax, Bx = _f64(Ax).reshape(-1), _f64(Bx).reshape(-1)
        assert Ax.size >= self.nnz_a and Bx.size >= self.nnz_b
        Cx = np.empty(self.nnz, dtype=np.float64)
        _check(lib().cs3_spgemm_values(self._p, _pf(Ax), _pf(Bx), _pf(Cx)))
        return Cx

    def values_dev(self, ax_ptr, bx_ptr, cx_ptr, stream=0):
        """Cx at cx_ptr from the values at ax_ptr, bx_ptr (device addresses), asynchronous on `stream`: at most two
        launches, no allocation, no synchronisation.  The same bits as values()."""
        _check(lib().cs3_spgemm_values_dev(self._p, C.c_void_p(ax_ptr), C.c_void_p(bx_ptr), C.c_void_p(cx_ptr),
                                           C.c_void_p(stream)))


def csc_multiply_ff(Am, An, Ap, Ai, Ax, Bm, Bn, Bp, Bi, Bx):
    """C = A B -> (Cm, Cn, Cp, Ci, Cx, Cnzmax) as csc_multiply_ff (csc_numba.py:222-306): rows of a column in order of first
    occurrence, sums in the reference's order, arrays trimmed to nnz.  One SpgemmPlan, used once."""
    assert An == Bm                                      # csc_numba.py:240
    with SpgemmPlan(Am, An, Ap, Ai, Bm, Bn, Bp, Bi) as plan:
        Cp, Ci = plan.pattern()
        Cx = plan.values(Ax, Bx)
    return Am, Bn, Cp, Ci, Cx, int(Cp[Bn])


def union_limits():
    """The constants that shape the launch of the embedding kernel (cs3_union_limits); needs no GPU."""
    out = UnionLimits()
    _check(lib().cs3_union_limits(C.byref(out)))
    return out


class UnionPlan:
    """Matrices of one order n whose patterns differ, for ONE batched handle: the union of the patterns (rows ascending)
    and the place of every member entry in it are worked out once on the host (cs3_union_plan_create, no GPU needed);
    values() / values_dev() then move the members' value arrays into the [nmat, nnz_union] layout that
    Factorization(n, n, Up, Ui, batch=nmat) reads, as often as the values change.  patterns: a sequence of (Ap, Ai);
    rows need not be sorted and may repeat (repeated entries are added up in storage order).  An entry a member does not
    have is +0.0; an entry with one source is copied bit for bit."""

    def __init__(self, n, patterns):
        self._p = C.c_void_p()
        pats = [(_i32(p[0]), _i32(p[1])) for p in patterns]            # (kept alive over the call)
        nmat = len(pats)
        aps = (_i32p * max(nmat, 1))(*[_pi(p[0]) for p in pats])
        ais = (_i32p * max(nmat, 1))(*[_pi(p[1]) for p in pats])
        _check(lib().cs3_union_plan_create(n, nmat, aps, ais, C.byref(self._p)))
        inf = self.info
        self.n, self.nmat, self.nnz = int(inf.n), int(inf.nmat), int(inf.nnz_union)
        self.nnz_total = int(inf.nnz_total)

    def close(self):
        if self._p:
            lib().cs3_union_plan_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def info(self):
        out = UnionInfo()
        _check(lib().cs3_union_plan_info(self._p, C.byref(out)))
        return out

    def pattern(self):
        """-> (Up int32[n + 1], Ui int32[nnz_union]) on the host."""
        Up = np.empty(self.n + 1, dtype=np.int32)
        Ui = np.empty(self.nnz, dtype=np.int32)
        _check(lib().cs3_union_plan_pattern(self._p, _pi(Up), _pi(Ui)))
        return Up, Ui

    def offsets(self):
        """-> int64[nmat + 1]: member b's values start at offsets()[b] of the concatenated value buffer."""
        off = np.empty(self.nmat + 1, dtype=np.int64)
        _check(lib().cs3_union_plan_offsets(self._p, off.ctypes.data_as(C.POINTER(I64))))
        return off

    def slots(self, b):
        """-> int32[nnz_b]: the union entry every entry of member b lands on."""
        off = self.offsets()
        assert 0 <= b < self.nmat
        slot = np.empty(int(off[b + 1] - off[b]), dtype=np.int32)
        _check(lib().cs3_union_plan_slots(self._p, b, _pi(slot)))
        return slot

    def upload(self):
        """Puts the tables on the device now (the first values call does it otherwise; do it before a graph capture)."""
        _check(lib().cs3_union_upload(self._p))
        return self

    def values(self, Ax):
        """Ax: the members' host value arrays, as a list or already concatenated.  -> float64[nmat, nnz_union]."""
        if isinstance(Ax, (list, tuple)):
            Ax = np.concatenate([_f64(a).reshape(-1) for a in Ax]) if len(Ax) else np.empty(0)
        Ax = _f64(Ax).reshape(-1)
        assert Ax.size >= self.nnz_total
        out = np.empty((self.nmat, self.nnz), dtype=np.float64)
        _check(lib().cs3_union_values(self._p, _pf(Ax), _pf(out)))
        return out

    def values_dev(self, cat_ptr, union_ptr, stream=0):
        """[nmat, nnz_union] at union_ptr from the concatenated values at cat_ptr (device addresses), asynchronous on
        `stream`: one launch, no allocation, no synchronisation.  The same bits as values()."""
        _check(lib().cs3_union_values_dev(self._p, C.c_void_p(cat_ptr), C.c_void_p(union_ptr), C.c_void_p(stream)))


# ----------------------------------------------------------- AC power flow --

def pf_limits():
    """The constants that shape the launches of the power-flow kernels (cs3_pf_limits); needs no GPU."""
    out = PfLimits()
    _check(lib().cs3_pf_limits(C.byref(out)))
    return out


class PowerFlowPlan:
    """Newton-Raphson AC power flow on the device (include/csparse3_amd.h, "AC power flow"): from the pattern (Yp, Yi) of
    a bus admittance matrix of order n and the bus lists pv, pq, the pattern of the Jacobian [[H, N], [M, L]] and the
    maps the kernels read (host work, no GPU needed), and a batched LU handle on that pattern, owned by the plan and lent
    out as `factorization`.  batch scenarios advance in lock-step; y_batch is 1 (one Y for all) or batch.
    Host arrays: Yz complex [y_batch, nnz_y], S complex [batch, n], vm and va float64 [batch, n].  The *_dev forms take
    device addresses of the same layouts (complex as interleaved doubles)."""

    def __init__(self, n, Yp, Yi, pv, pq, batch=1, y_batch=1, order=ORDER_AMD):
        self._p = C.c_void_p()
        self._f = None
        Yp, Yi, pv, pq = _i32(Yp), _i32(Yi), _i32(pv).reshape(-1), _i32(pq).reshape(-1)
        _check(lib().cs3_pf_plan_create(n, _pi(Yp), _pi(Yi), pv.size, _pi(pv), pq.size, _pi(pq), batch, y_batch, order,
                                        C.byref(self._p)))
        inf = self.info
        self.n, self.nnz_y, self.nj, self.nnz_j = int(inf.n), int(inf.nnz_y), int(inf.nj), int(inf.nnz_j)
        self.batch, self.y_batch = int(inf.batch), int(inf.y_batch)

    def close(self):
        if self._p:
            if self._f is not None:
                self._f.close()                          # the lent handle goes with the plan: the borrower is left empty
            lib().cs3_pf_plan_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def info(self):
        out = PfInfo()
        _check(lib().cs3_pf_plan_info(self._p, C.byref(out)))
        return out

    @property
    def factorization(self):
        """The plan's LU handle on the Jacobian as a Factorization that BORROWS it: everything a handle offers works on
        the Jacobian of the last factorisation; closing it frees nothing, and closing the plan leaves it empty (every
        call on it then raises Cs3Error).  Closing the borrower ends that loan only: the next access lends the handle again."""
        if self._f is None or not self._f._h:
            h = C.c_void_p()
            _check(lib().cs3_pf_handle(self._p, C.byref(h)))
            self._f = Factorization._borrow(h.value, self.nj, self.nnz_j, self.batch)
        return self._f

    def pattern(self):
        """-> (Jp int32[nj + 1], Ji int32[nnz_j]) on the host."""
        Jp = np.empty(self.nj + 1, dtype=np.int32)
        Ji = np.empty(self.nnz_j, dtype=np.int32)
        _check(lib().cs3_pf_plan_pattern(self._p, _pi(Jp), _pi(Ji)))
        return Jp, Ji

    def maps(self):
        """-> dict(jpos int32[4, nnz_y] (H, N, M, L; -1: none), Rp, Rj, Rpos (Y by rows), upos_a, upos_m int32[n])."""
        out = dict(jpos=np.empty((4, self.nnz_y), dtype=np.int32), Rp=np.empty(self.n + 1, dtype=np.int32),
                   Rj=np.empty(self.nnz_y, dtype=np.int32), Rpos=np.empty(self.nnz_y, dtype=np.int32),
                   upos_a=np.empty(self.n, dtype=np.int32), upos_m=np.empty(self.n, dtype=np.int32))
        _check(lib().cs3_pf_plan_maps(self._p, *[_pi(out[k]) for k in ("jpos", "Rp", "Rj", "Rpos", "upos_a", "upos_m")]))
        return out

    def _yz(self, Yz):
        Yz = _c128(Yz).reshape(-1)
        assert Yz.size == self.y_batch * self.nnz_y, "Yz must be [y_batch, nnz_y]"
        return Yz

    def _bn(self, a, dtype):
        a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
        assert a.size == self.batch * self.n, "expected [batch, n]"
        return a

    def mismatch(self, Yz, S, vm, va):
        """-> (-F float64[batch, nj] in unknown order, max |F| float64[batch])."""
        Yz, S, vm, va = self._yz(Yz), self._bn(S, np.complex128), self._bn(vm, np.float64), self._bn(va, np.float64)
        F = np.empty((self.batch, self.nj)); norm = np.empty(self.batch)
        _check(lib().cs3_pf_mismatch(self._p, _pc(Yz), _pc(S), _pf(vm), _pf(va), _pf(F), _pf(norm)))
        return F, norm

    def jacobian(self, Yz, vm, va):
        """-> Jx float64[batch, nnz_j], the values of pattern()."""
        Yz, vm, va = self._yz(Yz), self._bn(vm, np.float64), self._bn(va, np.float64)
        Jx = np.empty((self.batch, self.nnz_j))
        _check(lib().cs3_pf_jacobian(self._p, _pc(Yz), _pf(vm), _pf(va), _pf(Jx)))
        return Jx

    def _results(self):
        return np.zeros(self.batch, dtype=np.int32), np.zeros(self.batch), np.zeros(self.batch, dtype=np.int32)

    def solve(self, Yz, S, vm, va, tol=1e-8, max_iters=20, refactor_every=1, pivot_tol=1e-3):
        """Newton from (vm, va).  -> (vm, va, dict(iters, norm, flag)); flag 0 converged, 1 out of iterations, 2 not
        finite.  A rejected pivot raises SingularMatrix."""
        Yz, S = self._yz(Yz), self._bn(S, np.complex128)
        vm, va = self._bn(vm, np.float64).copy(), self._bn(va, np.float64).copy()
        iters, norm, flag = self._results()
        _check(lib().cs3_pf_solve(self._p, _pc(Yz), _pc(S), _pf(vm), _pf(va), tol, max_iters, refactor_every, pivot_tol,
                                  _pi(iters), _pf(norm), _pi(flag)))
        return vm.reshape(self.batch, self.n), va.reshape(self.batch, self.n), dict(iters=iters, norm=norm, flag=flag)

    def mismatch_dev(self, yz_ptr, s_ptr, vm_ptr, va_ptr, f_ptr, norm_ptr=0, stream=0):
        vp = C.c_void_p
        _check(lib().cs3_pf_mismatch_dev(self._p, vp(yz_ptr), vp(s_ptr), vp(vm_ptr), vp(va_ptr), vp(f_ptr), vp(norm_ptr), vp(stream)))

    def jacobian_dev(self, yz_ptr, vm_ptr, va_ptr, jx_ptr, stream=0):
        vp = C.c_void_p
        _check(lib().cs3_pf_jacobian_dev(self._p, vp(yz_ptr), vp(vm_ptr), vp(va_ptr), vp(jx_ptr), vp(stream)))

    def solve_dev(self, yz_ptr, s_ptr, vm_ptr, va_ptr, tol=1e-8, max_iters=20, refactor_every=1, pivot_tol=1e-3, stream=0):
        """Newton in place on the device arrays at vm_ptr, va_ptr.  -> dict(iters, norm, flag) (host).  Host-driven: one
        4-byte read per iteration synchronises `stream`."""
        vp = C.c_void_p
        iters, norm, flag = self._results()
        _check(lib().cs3_pf_solve_dev(self._p, vp(yz_ptr), vp(s_ptr), vp(vm_ptr), vp(va_ptr), tol, max_iters, refactor_every,
                                      pivot_tol, _pi(iters), _pf(norm), _pi(flag), vp(stream)))
        return dict(iters=iters, norm=norm, flag=flag)


# ---------------------------------------------------- AC state estimation --

def se_limits():
    """The constants that shape the launches of the state-estimation kernels (cs3_se_limits); needs no GPU."""
    out = SeLimits()
    _check(lib().cs3_se_limits(C.byref(out)))
    return out


class StateEstPlan:
    """Weighted-least-squares AC state estimation on the device (include/csparse3_amd.h, "AC state estimation"): from the
    pattern (Yp, Yi) of a bus admittance matrix of order n, the reference buses, the branch-end table (end_from, end_to)
    and the measurement list (kind, where), the pattern of the measurement Jacobian H by rows and in CSC and the tables
    the kernels read (host work, no GPU needed).  The first solve, bad_data, factorization or gain_pattern() builds the
    solver: the sparse product H' (W H), a Cholesky handle on its pattern (lent out as `factorization`), the bilinear-form
    plan of the rows of H.
    Host arrays: Yz complex [nnz_y], Ye complex [ne, 2] = (yff, yft), z and w float64 [m], vm and va float64 [n].  The
    *_dev forms take device addresses of the same layouts (complex as interleaved doubles)."""

    def __init__(self, n, Yp, Yi, ref, end_from, end_to, kind, where, order=ORDER_AMD):
        self._p = C.c_void_p()
        self._f = None
        Yp, Yi, ref = _i32(Yp), _i32(Yi), _i32(ref).reshape(-1)
        ef, et, kind, where = (_i32(a).reshape(-1) for a in (end_from, end_to, kind, where))
        assert ef.size == et.size and kind.size == where.size
        _check(lib().cs3_se_plan_create(n, _pi(Yp), _pi(Yi), ref.size, _pi(ref), ef.size, _pi(ef), _pi(et), kind.size, _pi(kind),
                                        _pi(where), order, C.byref(self._p)))
        inf = self.info
        self.n, self.nnz_y, self.ns, self.na, self.ne = int(inf.n), int(inf.nnz_y), int(inf.ns), int(inf.na), int(inf.ne)
        self.m, self.nnz_h = int(inf.m), int(inf.nnz_h)

    def close(self):
        if self._p:
            if self._f is not None:
                self._f.close()                          # the lent handle goes with the plan: the borrower is left empty
            lib().cs3_se_plan_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def info(self):
        out = SeInfo()
        _check(lib().cs3_se_plan_info(self._p, C.byref(out)))
        return out

    @property
    def factorization(self):
        """The plan's Cholesky handle on the gain matrix as a Factorization that BORROWS it (the rules of
        PowerFlowPlan.factorization): condest, slogdet, selinv, quad_plan ... work on the gain matrix of the last
        factorisation; closing it frees nothing, and closing the plan leaves it empty.  Builds the solver when needed."""
        if self._f is None or not self._f._h:
            h = C.c_void_p()
            _check(lib().cs3_se_handle(self._p, C.byref(h)))
            self._f = Factorization._borrow(h.value, self.ns, int(self.info.nnz_g), 1)
            self._f.kind = CS3_CHOLESKY
        return self._f

    def pattern(self):
        """-> dict(Hp int32[ns + 1], Hi int32[nnz_h] (CSC), Rp int32[m + 1], Rj int32[nnz_h] (by rows)) on the host."""
        out = dict(Hp=np.empty(self.ns + 1, dtype=np.int32), Hi=np.empty(self.nnz_h, dtype=np.int32),
                   Rp=np.empty(self.m + 1, dtype=np.int32), Rj=np.empty(self.nnz_h, dtype=np.int32))
        _check(lib().cs3_se_plan_pattern(self._p, *[_pi(out[k]) for k in ("Hp", "Hi", "Rp", "Rj")]))
        return out

    def maps(self):
        """-> dict(cpos int32[nnz_h] (row-order entry -> CSC position), upos_a int32[n] (-1: reference), upos_m int32[n])."""
        out = dict(cpos=np.empty(self.nnz_h, dtype=np.int32), upos_a=np.empty(self.n, dtype=np.int32),
                   upos_m=np.empty(self.n, dtype=np.int32))
        _check(lib().cs3_se_plan_maps(self._p, *[_pi(out[k]) for k in ("cpos", "upos_a", "upos_m")]))
        return out

    def gain_pattern(self):
        """-> (Gp int32[ns + 1], Gi int32[nnz_g]) of G = H' W H, rows in the order of the sparse product.  Needs the GPU."""
        _check(lib().cs3_se_gain_pattern(self._p, None, None))
        Gp, Gi = np.empty(self.ns + 1, dtype=np.int32), np.empty(int(self.info.nnz_g), dtype=np.int32)
        _check(lib().cs3_se_gain_pattern(self._p, _pi(Gp), _pi(Gi)))
        return Gp, Gi

    def _host(self, Yz, Ye, vm, va, z=None, w=None):
        Yz, Ye = _c128(Yz).reshape(-1), _c128(Ye).reshape(-1)
        assert Yz.size == self.nnz_y and Ye.size == 2 * self.ne, "Yz must be [nnz_y], Ye [ne, 2]"
        vm, va = _f64(vm).reshape(-1), _f64(va).reshape(-1)
        assert vm.size == self.n and va.size == self.n, "vm and va must be [n]"
        out = [Yz, Ye, vm, va]
        for a in (z, w):
            if a is not None:
                a = _f64(a).reshape(-1)
                assert a.size == self.m, "z and w must be [m]"
            out.append(a)
        return out

    def measure(self, Yz, Ye, z, w, vm, va):
        """-> (r float64[m] = z - h(x), J = sum w r^2)."""
        Yz, Ye, vm, va, z, w = self._host(Yz, Ye, vm, va, z, w)
        r, J = np.empty(self.m), np.empty(1)
        _check(lib().cs3_se_measure(self._p, _pc(Yz), _pc(Ye), _pf(z), _pf(w), _pf(vm), _pf(va), _pf(r), _pf(J)))
        return r, float(J[0])

    def jacobian(self, Yz, Ye, w, vm, va):
        """-> (Hr, Hc, WHc) float64[nnz_h]: H by rows, in CSC, and w_i H_ij in CSC, on pattern()."""
        Yz, Ye, vm, va, _, w = self._host(Yz, Ye, vm, va, None, w)
        Hr, Hc, WHc = (np.empty(self.nnz_h) for _ in range(3))
        _check(lib().cs3_se_jacobian(self._p, _pc(Yz), _pc(Ye), _pf(w), _pf(vm), _pf(va), _pf(Hr), _pf(Hc), _pf(WHc)))
        return Hr, Hc, WHc

    @staticmethod
    def _scalars():
        return C.c_int32(0), C.c_double(0.0), C.c_double(0.0), C.c_int32(0)

    @staticmethod
    def _solve_info(iters, step, J, flag):
        return dict(iters=int(iters.value), step=float(step.value), J=float(J.value), flag=int(flag.value))

    def solve(self, Yz, Ye, z, w, vm, va, tol=1e-8, max_iters=20):
        """Gauss-Newton from (vm, va).  -> (vm, va, dict(iters, step, J, flag)); flag 0 converged (max |dx| <= tol), 1 out
        of iterations, 2 a step that is not finite.  An unobservable state raises NotPositiveDefinite."""
        Yz, Ye, vm, va, z, w = self._host(Yz, Ye, vm, va, z, w)
        vm, va = vm.copy(), va.copy()
        iters, step, J, flag = self._scalars()
        _check(lib().cs3_se_solve(self._p, _pc(Yz), _pc(Ye), _pf(z), _pf(w), _pf(vm), _pf(va), tol, max_iters, C.byref(iters),
                                  C.byref(step), C.byref(J), C.byref(flag)))
        return vm, va, self._solve_info(iters, step, J, flag)

    def bad_data(self, Yz, Ye, z, w, vm, va, crit_tol=1e-8):
        """The largest-normalised-residual test at (vm, va).  -> dict(t, omega, rn float64[m], worst, worst_row, J, critical)."""
        Yz, Ye, vm, va, z, w = self._host(Yz, Ye, vm, va, z, w)
        t, omega, rn, s = np.empty(self.m), np.empty(self.m), np.empty(self.m), np.empty(4)
        _check(lib().cs3_se_baddata(self._p, _pc(Yz), _pc(Ye), _pf(z), _pf(w), _pf(vm), _pf(va), crit_tol, _pf(t), _pf(omega), _pf(rn),
                                    _pf(s)))
        return dict(t=t, omega=omega, rn=rn, worst=float(s[0]), worst_row=int(s[1]), J=float(s[2]), critical=int(s[3]))

    def residuals_dev(self):
        """-> (r_ptr, wr_ptr): device addresses of the plan's r [m] and w r [m] of the last residual pass."""
        r, wr = C.c_void_p(), C.c_void_p()
        _check(lib().cs3_se_residuals_dev(self._p, C.byref(r), C.byref(wr)))
        return r.value, wr.value

    def measure_dev(self, yz_ptr, ye_ptr, z_ptr, w_ptr, vm_ptr, va_ptr, r_ptr=0, j_ptr=0, stream=0):
        vp = C.c_void_p
        _check(lib().cs3_se_measure_dev(self._p, vp(yz_ptr), vp(ye_ptr), vp(z_ptr), vp(w_ptr), vp(vm_ptr), vp(va_ptr), vp(r_ptr),
                                        vp(j_ptr), vp(stream)))

    def jacobian_dev(self, yz_ptr, ye_ptr, w_ptr, vm_ptr, va_ptr, hr_ptr=0, hc_ptr=0, whc_ptr=0, stream=0):
        vp = C.c_void_p
        _check(lib().cs3_se_jacobian_dev(self._p, vp(yz_ptr), vp(ye_ptr), vp(w_ptr), vp(vm_ptr), vp(va_ptr), vp(hr_ptr), vp(hc_ptr),
                                         vp(whc_ptr), vp(stream)))

    def gradient_dev(self, hc_ptr, wr_ptr, g_ptr, stream=0):
        """g [ns] = H' (w r) from Hc [nnz_h] and w r [m], in the fixed order of k_se_gradient."""
        vp = C.c_void_p
        _check(lib().cs3_se_gradient_dev(self._p, vp(hc_ptr), vp(wr_ptr), vp(g_ptr), vp(stream)))

    def solve_dev(self, yz_ptr, ye_ptr, z_ptr, w_ptr, vm_ptr, va_ptr, tol=1e-8, max_iters=20, stream=0):
        """Gauss-Newton in place on the device arrays at vm_ptr, va_ptr.  -> dict(iters, step, J, flag) (host).
        Host-driven: one read per iteration synchronises `stream`."""
        vp = C.c_void_p
        iters, step, J, flag = self._scalars()
        _check(lib().cs3_se_solve_dev(self._p, vp(yz_ptr), vp(ye_ptr), vp(z_ptr), vp(w_ptr), vp(vm_ptr), vp(va_ptr), tol, max_iters,
                                      C.byref(iters), C.byref(step), C.byref(J), C.byref(flag), vp(stream)))
        return self._solve_info(iters, step, J, flag)

    def bad_data_dev(self, yz_ptr, ye_ptr, z_ptr, w_ptr, vm_ptr, va_ptr, crit_tol, summary_ptr, t_ptr=0, omega_ptr=0, rn_ptr=0,
                     stream=0):
        vp = C.c_void_p
        _check(lib().cs3_se_baddata_dev(self._p, vp(yz_ptr), vp(ye_ptr), vp(z_ptr), vp(w_ptr), vp(vm_ptr), vp(va_ptr), crit_tol,
                                        vp(t_ptr), vp(omega_ptr), vp(rn_ptr), vp(summary_ptr), vp(stream)))


# -------------------------------------------------------- complex matrices --

CPLX_N, CPLX_T, CPLX_H = 0, 1, 2
_CPLX_OPS = {"N": CPLX_N, "T": CPLX_T, "H": CPLX_H, False: CPLX_N, True: CPLX_T}


def cplx_op(trans):
    """"N" | "T" | "H" (or False | True for N | T, or the enum itself) -> cs3_cplx_op."""
    if isinstance(trans, str):
        trans = trans.upper()
    assert trans in _CPLX_OPS or trans == CPLX_H, "trans must be 'N', 'T' or 'H'"
    return _CPLX_OPS.get(trans, trans)


def cplx_limits():
    """The constants that shape the launches of the complex glue kernels (cs3_cplx_limits); needs no GPU."""
    out = CplxLimits()
    _check(lib().cs3_cplx_limits(C.byref(out)))
    return out


def _c128(a):
    return np.ascontiguousarray(a, dtype=np.complex128)


def _pc(a):
    return a.ctypes.data_as(_f64p)


class ComplexPlan:
    """A complex CSC pattern of order n for a handle on its real-equivalent form (include/csparse3_amd.h, "complex
    matrices"): every entry w is the block [[Re w, -Im w], [Im w, Re w]] of a real matrix of order 2n, rows and columns
    interleaved.  pattern() and order() are what Factorization(2n, 2n, Rp, Ri, q=q2) analyses (host work, no GPU);
    values / pack / unpack / residual are the device glue, with host-array and `_dev` forms that give the same bits.
    rotate: rows are multiplied by s_i = conj(d_i) / max(|Re d_i|, |Im d_i|) so that the static pivots, the real parts of
    the diagonal, are positive (an admittance matrix has a mostly imaginary diagonal).  Right-hand sides are [n], [n, k] or
    [batch, n, k] complex128, their real forms [2n], [2n, k] or [batch, 2n, k] float64.
    schur: the border of a Kron reduction (cs3_cplx_plan_create_schur): rows that are never rotated (s = 1 there), so that
    the Schur complement of the real form is that of A itself; schur_order() and schur_info() go with it."""

    def __init__(self, n, Ap, Ai, batch=1, rotate=True, schur=None):
        self._p = C.c_void_p()
        Ap, Ai = _i32(Ap), _i32(Ai)
        self.ns = 0
        if schur is None:
            _check(lib().cs3_cplx_plan_create(n, _pi(Ap), _pi(Ai), batch, int(rotate), C.byref(self._p)))
        else:
            idx = _i32(schur).reshape(-1)
            _check(lib().cs3_cplx_plan_create_schur(n, _pi(Ap), _pi(Ai), batch, int(rotate), idx.size, _pi(idx), C.byref(self._p)))
            self.ns = int(idx.size)
        inf = self.info
        self.n, self.nnz, self.batch, self.rotate = int(inf.n), int(inf.nnz), int(inf.batch), bool(inf.rotate)

    def close(self):
        if self._p:
            lib().cs3_cplx_plan_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def info(self):
        out = CplxInfo()
        _check(lib().cs3_cplx_plan_info(self._p, C.byref(out)))
        return out

    def pattern(self):
        """-> (Rp int32[2n + 1], Ri int32[4 nnz]) on the host: the pattern of the real form."""
        Rp = np.empty(2 * self.n + 1, dtype=np.int32)
        Ri = np.empty(4 * self.nnz, dtype=np.int32)
        _check(lib().cs3_cplx_plan_pattern(self._p, _pi(Rp), _pi(Ri)))
        return Rp, Ri

    def order(self, order=ORDER_AMD, q=None):
        """-> q2 int32[2n]: the fill-reducing order of the complex pattern (or q) with every index doubled into its pair."""
        qa = None
        if q is not None:
            qa = _i32(q)
            assert qa.size == self.n
            order = ORDER_GIVEN
        q2 = np.empty(2 * self.n, dtype=np.int32)
        _check(lib().cs3_cplx_plan_order(self._p, order, _pi(qa), _pi(q2)))
        return q2

    def schur_info(self):
        """-> int32[ns]: the border in the order of S's rows and columns (Cs3Error on a plan without one)."""
        ns = I64()
        _check(lib().cs3_cplx_plan_schur_info(self._p, C.byref(ns), None))
        idx = np.empty(int(ns.value), dtype=np.int32)
        _check(lib().cs3_cplx_plan_schur_info(self._p, None, _pi(idx)))
        return idx

    def schur_order(self, order=ORDER_AMD, q=None):
        """-> (q2_interior int32[2 (n - ns)], schur2 int32[2 ns]): the doubled order of the interior (AMD of A11, natural,
        or q, a permutation of the interior) and the doubled border, for Factorization(..., q=q2_interior, schur=schur2)."""
        qa = None
        if q is not None:
            qa = _i32(q)
            assert qa.size == self.n - self.ns
            order = ORDER_GIVEN
        q2 = np.empty(2 * max(self.n - self.ns, 0), dtype=np.int32)
        s2 = np.empty(2 * self.ns, dtype=np.int32)
        _check(lib().cs3_cplx_plan_schur_order(self._p, order, _pi(qa), _pi(q2), _pi(s2)))
        return q2, s2

    def upload(self):
        """Puts the tables on the device now (the first device call does it otherwise; do it before a graph capture)."""
        _check(lib().cs3_cplx_upload(self._p))
        return self

    def _k(self, a):
        per = self.batch * self.n
        assert per > 0 and a.size % per == 0, "array does not match [batch,] n [, k]"
        assert a.ndim == 3 or self.batch == 1, "with batch > 1 arrays are [batch, n, k]"
        return a.size // per

    @staticmethod
    def _scaled(shape, num, den):
        axis = 1 if len(shape) == 3 else 0
        return tuple(s * num // den if a == axis else s for a, s in enumerate(shape))

    def values(self, Az):
        """Az: complex128 [batch, nnz] (or [nnz]).  -> float64 [batch, 4 nnz]: the values of the real form, rotated."""
        Az = _c128(Az).reshape(-1)
        assert Az.size >= self.batch * self.nnz
        out = np.empty((self.batch, 4 * self.nnz), dtype=np.float64)
        _check(lib().cs3_cplx_values(self._p, _pc(Az), _pf(out)))
        return out

    def rotation(self):
        """-> complex128 [batch, n]: s of the last values call."""
        s = np.empty((self.batch, self.n), dtype=np.complex128)
        _check(lib().cs3_cplx_rotation(self._p, _pc(s)))
        return s

    def pack(self, Z, trans="N"):
        """The real right-hand side of op(A) x = z for the handle (op N: rotated; T: conjugated; H: as it is)."""
        Z = _c128(Z)
        k = self._k(Z)
        Y = np.empty(self._scaled(Z.shape, 2, 1), dtype=np.float64)
        _check(lib().cs3_cplx_pack(self._p, cplx_op(trans), _pc(Z), _pf(Y), k))
        return Y

    def unpack(self, Y, trans="N", into=None):
        """The complex solution from the handle's real one.  into: a complex array the result is ADDED to (a new array
        comes back; `into` stays)."""
        Y = _f64(Y)
        per = 2 * self.batch * self.n
        assert per > 0 and Y.size % per == 0, "array does not match [batch,] 2n [, k]"
        k = Y.size // per
        if into is None:
            Z = np.empty(self._scaled(Y.shape, 1, 2), dtype=np.complex128)
        else:
            Z = np.array(into, dtype=np.complex128, order="C", copy=True)
            assert Z.size * 2 == Y.size
        _check(lib().cs3_cplx_unpack(self._p, cplx_op(trans), _pf(Y), _pc(Z), k, 0 if into is None else 1))
        return Z

    def residual(self, Az, b, x, trans="N"):
        """R = b - op(A) x with the caller's values Az (complex128 [batch, nnz]), not the rotated ones."""
        Az, b, x = _c128(Az).reshape(-1), _c128(b), _c128(x)
        assert Az.size >= self.batch * self.nnz and b.shape == x.shape
        R = np.empty_like(b)
        _check(lib().cs3_cplx_residual(self._p, cplx_op(trans), _pc(Az), _pc(b), _pc(x), _pc(R), self._k(b)))
        return R

    # -- device pointers on a HIP stream: one or two launches each, nothing allocated after the first call
    def values_dev(self, az_ptr, rx_ptr, stream=0):
        _check(lib().cs3_cplx_values_dev(self._p, C.c_void_p(az_ptr), C.c_void_p(rx_ptr), C.c_void_p(stream)))

    def pack_dev(self, z_ptr, y_ptr, k=1, trans="N", stream=0):
        _check(lib().cs3_cplx_pack_dev(self._p, cplx_op(trans), C.c_void_p(z_ptr), C.c_void_p(y_ptr), k, C.c_void_p(stream)))

    def unpack_dev(self, y_ptr, z_ptr, k=1, trans="N", accumulate=False, stream=0):
        _check(lib().cs3_cplx_unpack_dev(self._p, cplx_op(trans), C.c_void_p(y_ptr), C.c_void_p(z_ptr), k, int(bool(accumulate)),
                                         C.c_void_p(stream)))

    def residual_dev(self, az_ptr, b_ptr, x_ptr, r_ptr, k=1, trans="N", stream=0):
        _check(lib().cs3_cplx_residual_dev(self._p, cplx_op(trans), C.c_void_p(az_ptr), C.c_void_p(b_ptr), C.c_void_p(x_ptr),
                                           C.c_void_p(r_ptr), k, C.c_void_p(stream)))

    def rotation_dev(self):
        """The device address of s [batch, n] complex."""
        out = C.c_void_p()
        _check(lib().cs3_cplx_rotation_dev(self._p, C.byref(out)))
        return int(out.value or 0)

    def workspace_dev(self, slot, count):
        """The device address of a block of `count` doubles that the plan owns (slot 0, 1 or 2; grown only when needed)."""
        out = C.c_void_p()
        _check(lib().cs3_cplx_workspace_dev(self._p, slot, count, C.byref(out)))
        return int(out.value or 0)


class ComplexFactorization:
    """A z = b for a complex CSC matrix: a ComplexPlan and a Factorization (`.real`: condest, slogdet, info, ... stay
    reachable there) on the plan's real-equivalent pattern and doubled order.  Values are complex128 [batch, nnz],
    right-hand sides [n], [n, k] or [batch, n, k].  trans: "N" A x = b, "T" A^T x = b (no conjugate), "H" A^H x = b, all on
    the same factors.  rotate (LU only): see ComplexPlan; with it the factors are those of diag(s) A.
    schur: the boundary buses of a Kron reduction, not eliminated (a Schur handle on the real form).  factor() then holds
    the complex S = A22 - A21 A11^-1 A12 in the order of the list: schur(), schur_forward(), schur_backward(); order / q refer
    to the interior; solve() raises Cs3Error, as on every Schur handle.
    sens_plan / sens_solve: Y = C op(A)^-1 B with sparse B and C (entries of Z-bus), see ComplexSensPlan.
    updates_plan / solve_updates: (A + dA_c) x = b for many sparse complex dA_c (outages, faults), see ComplexUpdatesPlan.
    selinv / inverse_entries / inverse_diagonal / thevenin: A^-1 on the pattern of A from the selected inverse of the real
    form (diag(Z-bus), the Thevenin impedance of every branch)."""

    def __init__(self, n, Ap, Ai, kind=CS3_LU, order=ORDER_AMD, q=None, batch=1, rotate=True, schur=None):
        assert not (rotate and kind == CS3_CHOLESKY), "rotate scales rows, which breaks the symmetry Cholesky needs: pass rotate=False"
        self.kind, self.n, self.batch = kind, int(n), int(batch)
        self.plan = self.real = None
        self._ws = (0, None)
        self.plan = ComplexPlan(n, Ap, Ai, batch, rotate, schur=schur)
        self.nnz, self.ns = self.plan.nnz, self.plan.ns
        Rp, Ri = self.plan.pattern()
        if schur is None:
            self.real = Factorization(2 * self.n, 2 * self.n, Rp, Ri, kind=kind, q=self.plan.order(order, q), batch=batch)
        else:
            q2, s2 = self.plan.schur_order(order, q)
            self.real = Factorization(2 * self.n, 2 * self.n, Rp, Ri, kind=kind, q=q2, batch=batch, schur=s2)

    def close(self):
        if self.real is not None:
            self.real.close()
        if self.plan is not None:
            self.plan.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- host arrays
    def factor(self, Az, tol=0.0):
        self.real.factor(self.plan.values(Az), tol)
        return self

    def solve(self, b, trans="N"):
        """Solve op(A) x = b; returns a new complex array of b's shape."""
        op = cplx_op(trans)
        return self.plan.unpack(self.real.solve(self.plan.pack(b, op), trans=op != CPLX_N), op)

    def residual(self, Az, b, x, trans="N"):
        return self.plan.residual(Az, b, x, trans)

    def refine(self, Az, b, x, steps=1, trans="N"):
        """`steps` rounds of x += op(A) \\ (b - op(A) x) with the held factors and the values Az.  -> the refined x."""
        op = cplx_op(trans)
        x = _c128(x)
        for _ in range(steps):
            r = self.plan.residual(Az, b, x, op)
            x = self.plan.unpack(self.real.solve(self.plan.pack(r, op), trans=op != CPLX_N), op, into=x)
        return x

    # -- device pointers on a HIP stream
    def _workspace(self, k):
        """(Rx, Y, X2) in the plan's workspace, for k right-hand sides: asks the plan only when k grows."""
        if self._ws[1] is None or k > self._ws[0]:
            per = 2 * self.batch * self.n * k
            self._ws = (k, (self.plan.workspace_dev(0, 4 * self.batch * self.nnz), self.plan.workspace_dev(1, per),
                            self.plan.workspace_dev(2, per)))
        return self._ws[1]

    def factor_solve_dev(self, az_ptr, b_ptr, x_ptr, k=1, tol=0.0, stream=0):
        """(Re)factorise Az and solve A X = B: values -> pack -> the handle's fused factor + solve -> unpack, all on
        `stream`; B [batch][n, k] complex stays, X gets the solutions.  The bits of factor() + solve().  Status through
        factor_status()."""
        rx, y, x2 = self._workspace(k)
        self.plan.values_dev(az_ptr, rx, stream)
        self.plan.pack_dev(b_ptr, y, k, CPLX_N, stream)
        self.real.factor_solve_bx_dev(rx, y, x2, k, tol, stream)
        self.plan.unpack_dev(x2, x_ptr, k, CPLX_N, False, stream)

    def solve_dev(self, b_ptr, x_ptr, k=1, stream=0, trans="N"):
        """op(A) X = B on the held factors; B stays, X gets the solutions (they may be the same array)."""
        op = cplx_op(trans)
        _, y, _ = self._workspace(k)
        self.plan.pack_dev(b_ptr, y, k, op, stream)
        self.real.solve_dev(y, k, stream, trans=op != CPLX_N)
        self.plan.unpack_dev(y, x_ptr, k, op, False, stream)

    def factor_status(self, stream=0):
        self.real.factor_status(stream)

    # -- Kron reduction (a factorisation made with schur=...)
    def schur_info(self):
        return self.plan.schur_info()

    def schur(self):
        """The complex Schur complement of the last factorisation: [ns, ns], or [batch, ns, ns]; S[i, j] belongs to
        (schur[i], schur[j]).  A Cholesky handle gives a Hermitian S."""
        S = np.empty((self.batch, self.ns, self.ns), dtype=np.complex128)
        _check(lib().cs3_cplx_schur_get(self.plan._p, self.real._h, _pc(S)))
        return S[0] if self.batch == 1 else S

    def schur_dev(self, s_ptr, stream=0):
        """schur() into device memory [batch][ns, ns] complex, one launch on `stream`."""
        _check(lib().cs3_cplx_schur_get_dev(self.plan._p, self.real._h, C.c_void_p(s_ptr), C.c_void_p(stream)))

    def schur_forward(self, b):
        """b: [n], [n, k] or [batch, n, k] complex.  -> a new array whose border rows hold b2 - A21 A11^-1 b1 (the right-hand
        side of S x2 = g); the interior rows are the half-solved interior, to be passed on to schur_backward."""
        return self.plan.unpack(self.real.schur_forward(self.plan.pack(b, CPLX_N)), CPLX_N)

    def schur_backward(self, y):
        """y: what schur_forward returned, with the border rows replaced by x2.  -> the solution of A x = b."""
        return self.plan.unpack(self.real.schur_backward(self.plan.pack(y, CPLX_H)), CPLX_N)

    def schur_forward_dev(self, b_ptr, y_ptr, k=1, stream=0):
        """schur_forward on device pointers: B [batch][n, k] complex stays, Y gets the result (they may be the same)."""
        _, x2, _ = self._workspace(k)
        self.plan.pack_dev(b_ptr, x2, k, CPLX_N, stream)
        self.real.schur_forward_dev(x2, k, stream)
        self.plan.unpack_dev(x2, y_ptr, k, CPLX_N, False, stream)

    def schur_backward_dev(self, y_ptr, x_ptr, k=1, stream=0):
        """schur_backward on device pointers: Y stays, X gets the solution (they may be the same)."""
        _, x2, _ = self._workspace(k)
        self.plan.pack_dev(y_ptr, x2, k, CPLX_H, stream)
        self.real.schur_backward_dev(x2, k, stream)
        self.plan.unpack_dev(x2, x_ptr, k, CPLX_N, False, stream)

    # -- sparse right-hand sides: entries of Z-bus
    def sens_plan(self, B, Ct=None, side="auto", trans="N"):
        """A ComplexSensPlan for Y = C op(A)^-1 B: B = (k, indptr, indices) by columns or None for I; Ct the same for the
        ROWS of C or None for I; indices of the complex matrix."""
        return ComplexSensPlan(self, B, Ct, side, trans)

    def sens_solve(self, plan, Bz, Ctz):
        """Y [p, k] complex128 = C op(A)^-1 B with the values Bz, Ctz (complex, in the plan's entry order; None for an
        identity operand) on the factors at hand."""
        Bz = _c128(Bz if Bz is not None else []).reshape(-1)
        Ctz = _c128(Ctz if Ctz is not None else []).reshape(-1)
        assert plan.bp is None or Bz.size >= int(plan.bp[-1])
        assert plan.ctp is None or Ctz.size >= int(plan.ctp[-1])
        Y = np.empty((plan.p, plan.k), dtype=np.complex128)
        _check(lib().cs3_cplx_sens_solve(self.plan._p, self.real._h, plan._u, _pc(Bz), _pc(Ctz), _pc(Y)))
        return Y

    def sens_solve_dev(self, plan, bz_ptr, ctz_ptr, y_ptr, stream=0):
        """sens_solve on device pointers, asynchronous on `stream`; Y [p, k] complex row-major.  After the first call with a
        plan nothing is allocated and nothing synchronises.  The same bits as sens_solve()."""
        _check(lib().cs3_cplx_sens_solve_dev(self.plan._p, self.real._h, plan._u, C.c_void_p(bz_ptr), C.c_void_p(ctz_ptr),
                                             C.c_void_p(y_ptr), C.c_void_p(stream)))

    def debug_sens_parts(self, plan, parts, bz_ptr, ctz_ptr, y_ptr, stream=0):
        """Diagnostics: the steps of sens_solve_dev in the mask `parts` (1 scatter, 2 solves, 4 combine)."""
        _check(lib().cs3_debug_cplx_sens_parts(self.plan._p, self.real._h, plan._u, parts, C.c_void_p(bz_ptr), C.c_void_p(ctz_ptr),
                                               C.c_void_p(y_ptr), C.c_void_p(stream)))


    # -- low-rank-modified systems: outages, faults and switching on an admittance matrix
    def updates_plan(self, cases):
        """A ComplexUpdatesPlan for a list of modifications of A: `cases` is a list of (rows, cols) index arrays, one pair per
        case, in the indices of the complex matrix (or the flat triple (cp, ci, cj)); at most 16 distinct rows and 16
        distinct columns per case."""
        return ComplexUpdatesPlan(self, cases)

    def solve_updates(self, plan, cz, b, sing_tol=0.0):
        """x_c = (A + dA_c)^-1 b for every case of `plan` on the factors at hand; cz holds the complex values of all
        triplets in the plan's order.  -> (X [n, ncases] complex128, rpiv [ncases]).  A case with rpiv[c] <= sing_tol
        (sing_tol > 0), an exactly zero pivot or a NaN has a (NaN, NaN) column in X; the others are unaffected."""
        cz, b = _c128(cz).reshape(-1), _c128(b).reshape(-1)
        assert cz.size >= int(plan.cp[-1]) and b.size == self.n
        X = np.empty((self.n, plan.ncases), dtype=np.complex128)
        rpiv = np.empty(plan.ncases, dtype=np.float64)
        _check(lib().cs3_cplx_updates_solve(self.plan._p, self.real._h, plan._u, _pc(cz), _pc(b), sing_tol, _pc(X), _pf(rpiv)))
        return X, rpiv

    def solve_updates_dev(self, plan, cz_ptr, b_ptr, x_ptr, rpiv_ptr=0, sing_tol=0.0, stream=0):
        """solve_updates on device pointers, asynchronous on `stream`; X [n, ncases] complex row-major.  After the first
        call with a plan nothing is allocated and nothing synchronises.  The same bits as solve_updates()."""
        _check(lib().cs3_cplx_updates_solve_dev(self.plan._p, self.real._h, plan._u, C.c_void_p(cz_ptr), C.c_void_p(b_ptr), sing_tol,
                                                C.c_void_p(x_ptr), C.c_void_p(rpiv_ptr), C.c_void_p(stream)))

    def debug_updates_parts(self, plan, parts, cz_ptr, b_ptr, x_ptr, rpiv_ptr=0, sing_tol=0.0, stream=0):
        """Diagnostics: the steps of solve_updates_dev in the mask `parts` (1 x0 and units, 2 solves, 4 capacitance + apply)."""
        _check(lib().cs3_debug_cplx_updates_parts(self.plan._p, self.real._h, plan._u, parts, C.c_void_p(cz_ptr), C.c_void_p(b_ptr),
                                                  sing_tol, C.c_void_p(x_ptr), C.c_void_p(rpiv_ptr), C.c_void_p(stream)))

    # -- selected inversion: Z = A^-1 on the pattern of A, diag(Z-bus), the Thevenin table of the branches
    def selinv(self, stream=0):
        """The selected inverse of the real form on the factors at hand (Factorization.selinv), asynchronously on `stream`;
        the `_dev` getters below read it."""
        self.real.selinv(stream)
        return self

    def selinv_maps(self):
        """-> (entry int64 [nnz, 2], entry_t [nnz, 2], diag [n, 2]): where the getters read the real selected inverse, as
        offsets in the handle's block of Z per matrix (diagnostic; from the analysis alone, needs no GPU)."""
        entry, entry_t = (np.empty((self.nnz, 2), dtype=np.int64) for _ in range(2))
        diag = np.empty((self.n, 2), dtype=np.int64)
        p64 = C.POINTER(I64)
        _check(lib().cs3_debug_cplx_selinv_maps(self.plan._p, self.real._h, entry.ctypes.data_as(p64), entry_t.ctypes.data_as(p64),
                                                diag.ctypes.data_as(p64)))
        return entry, entry_t, diag

    def _zshape(self, count):
        return (count,) if self.batch == 1 else (self.batch, count)

    def inverse_entries(self, trans=False):
        """-> complex128 [nnz] (or [batch, nnz]): A^-1(Ai[e], j) for every stored entry e of column j; with `trans`
        A^-1(j, Ai[e]).  Runs selinv() first when the handle holds no inverse of the current factors."""
        Zz = np.empty(self._zshape(self.nnz), dtype=np.complex128)
        _check(lib().cs3_cplx_selinv_entries(self.plan._p, self.real._h, 1 if trans else 0, _pc(Zz)))
        return Zz

    def inverse_diagonal(self):
        """-> complex128 [n] (or [batch, n]): A^-1(i, i), the driving-point impedances of an admittance matrix."""
        d = np.empty(self._zshape(self.n), dtype=np.complex128)
        _check(lib().cs3_cplx_selinv_diag(self.plan._p, self.real._h, _pc(d)))
        return d

    def thevenin(self):
        """-> complex128 [nnz] (or [batch, nnz]): ((Z_ii + Z_jj) - Z_ij) - Z_ji of Z = A^-1 for every stored entry (i, j),
        the Thevenin impedance between the ends of a branch."""
        T = np.empty(self._zshape(self.nnz), dtype=np.complex128)
        _check(lib().cs3_cplx_selinv_thevenin(self.plan._p, self.real._h, _pc(T)))
        return T

    def inverse_entries_dev(self, z_ptr, trans=False, stream=0):
        """inverse_entries into device memory [batch][nnz] complex (16-byte aligned), one launch on `stream`, after
        selinv().  After the first call nothing is allocated and nothing synchronises.  The same bits."""
        _check(lib().cs3_cplx_selinv_entries_dev(self.plan._p, self.real._h, 1 if trans else 0, C.c_void_p(z_ptr), C.c_void_p(stream)))

    def inverse_diagonal_dev(self, d_ptr, stream=0):
        """inverse_diagonal into device memory [batch][n] complex, as inverse_entries_dev."""
        _check(lib().cs3_cplx_selinv_diag_dev(self.plan._p, self.real._h, C.c_void_p(d_ptr), C.c_void_p(stream)))

    def thevenin_dev(self, t_ptr, stream=0):
        """thevenin into device memory [batch][nnz] complex, as inverse_entries_dev."""
        _check(lib().cs3_cplx_selinv_thevenin_dev(self.plan._p, self.real._h, C.c_void_p(t_ptr), C.c_void_p(stream)))


def cplx_selinv_limits():
    """The constants of the complex selected-inverse getters (cs3_cplx_selinv_limits); needs no GPU."""
    out = CplxSelinvLimits()
    _check(lib().cs3_cplx_selinv_limits(C.byref(out)))
    return out


def cplx_updates_limits():
    """The constants of the complex low-rank-modified solves (cs3_cplx_updates_limits); needs no GPU."""
    out = CplxUpdatesLimits()
    _check(lib().cs3_cplx_updates_limits(C.byref(out)))
    return out


class ComplexUpdatesPlan:
    """The pattern of a list of sparse complex modifications dA_c (ComplexFactorization.updates_plan): made once on the
    host, used by every solve_updates, across refactorisations.  One touched bus is one real column of the handle's tile."""

    def __init__(self, factorization, cases):
        self._u = C.c_void_p()
        self.cp, self.ci, self.cj = _flat_cases(cases)
        self.ncases = len(self.cp) - 1
        _check(lib().cs3_cplx_updates_plan(factorization.plan._p, factorization.real._h, self.ncases, _pi(self.cp), _pi(self.ci),
                                           _pi(self.cj), C.byref(self._u)))

    def close(self):
        if self._u:
            lib().cs3_cplx_updates_free(self._u)
            self._u = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def info(self):
        out = [I64() for _ in range(4)]
        _check(lib().cs3_cplx_updates_info(self._u, *[C.byref(o) for o in out]))
        return UpdatesInfo(*[int(o.value) for o in out])

    def tiles(self):
        """-> int32 [ntiles, 4]: first case, cases, touched rows and solve width of every tile (diagnostic)."""
        nt = self.info.ntiles
        arrs = [np.empty(nt, dtype=np.int32) for _ in range(4)]
        assert lib().cs3_debug_cplx_updates_tiles(self._u, *[_pi(a) for a in arrs]) == nt
        return np.stack(arrs, axis=1)


def cplx_sens_limits():
    """The constants of the complex sparse right-hand-side kernels (cs3_cplx_sens_limits); needs no GPU."""
    out = SensLimits()
    _check(lib().cs3_cplx_sens_limits(C.byref(out)))
    return out


class ComplexSensPlan:
    """The patterns of B and C' of Y = C op(A)^-1 B on a ComplexFactorization (its sens_plan): made once on the host, used
    by every sens_solve, across refactorisations.  trans: "N", "T" or "H".  One complex solved-for column is one real
    column of the handle's tile: side left with p rows of C plans p solves."""

    def __init__(self, factorization, B, Ct=None, side="auto", trans="N"):
        self._u = C.c_void_p()
        n = factorization.n
        self.k, self.bp, self.bi = (n, None, None) if B is None else (int(B[0]), _i32(B[1]), _i32(B[2]))
        self.p, self.ctp, self.cti = (n, None, None) if Ct is None else (int(Ct[0]), _i32(Ct[1]), _i32(Ct[2]))
        assert self.bp is None or self.bp.size == self.k + 1, "B is (ncols, indptr[ncols + 1], indices)"
        assert self.ctp is None or self.ctp.size == self.p + 1, "Ct is (ncols, indptr[ncols + 1], indices)"
        _check(lib().cs3_cplx_sens_plan(factorization.plan._p, factorization.real._h, self.k, _pi(self.bp), _pi(self.bi), self.p,
                                        _pi(self.ctp), _pi(self.cti), SENS_SIDES.get(side, side), cplx_op(trans), C.byref(self._u)))

    def close(self):
        if self._u:
            lib().cs3_cplx_sens_free(self._u)
            self._u = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def info(self):
        out = SensInfo()
        _check(lib().cs3_cplx_sens_info(self._u, C.byref(out)))
        return out


def csc_sub_matrix(Am, Anz, Ap, Ai, Ax, rows, cols):
    """A[rows, cols] -> (nnz, Bp, Bi, Bx) exactly as csc_sub_matrix computes it (csc_numba.py:464-502): the new row
    index is that function's running match counter, not the position of the row in `rows`."""
    Ap, Ai, Ax, rows, cols = _i32(Ap), _i32(Ai), _f64(Ax), _i32(rows), _i32(cols)
    n = len(Ap) - 1
    cap = max(Anz, 1)                                    # what the reference allocates (csc_numba.py:476-478)
    Bp = np.empty(len(cols) + 1, dtype=np.int32); Bi = np.empty(cap, dtype=np.int32); Bx = np.zeros(cap, dtype=np.float64)
    _check(lib().cs3_csc_sub_matrix(n, _pi(Ap), _pi(Ai), _pf(Ax), _pi(rows), len(rows), _pi(cols), len(cols), _pi(Bp), _pi(Bi), _pf(Bx), cap))
    nz = int(Bp[len(cols)])
    return nz, Bp, Bi[:nz].copy(), Bx[:nz].copy()


def find_islands(node_number, indptr, indices):
    """Islands of the pattern as find_islands / CscMat.islands give them (csc_numba.py:744-808, csc.py:515-521):
    a list of islands ordered by their smallest node, each a sorted int32 array."""
    Ap, Ai = _i32(indptr), _i32(indices)
    label = np.empty(node_number, dtype=np.int32)
    _check(lib().cs3_find_islands(node_number, _pi(Ap), _pi(Ai), _pi(label)))
    order = np.argsort(label, kind="stable")
    cuts = np.flatnonzero(np.diff(label[order])) + 1
    return [g.astype(np.int32) for g in np.split(order, cuts)] if node_number else []

