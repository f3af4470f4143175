"""ctypes view of libmi_hypre.so for tests/ and bench.py.

This is plumbing, not the product: the host side of the product is the C++
driver in host/ (HypreSystem + main, mirroring /root/reference/src).  Everything
here goes through the C ABI declared in include/*.h.  There is no fallback: if
the shared library is missing, or no HIP device is present at HYPRE_Init, this
raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MI_HYPRE_LIB: another build of the same library (A/B timing of kernel variants on one box); never a fallback
LIB_PATH = os.environ.get("MI_HYPRE_LIB") or os.path.join(_HERE, "libmi_hypre.so")

HYPRE_PARCSR = 5555
HYPRE_MEMORY_DEVICE = 1
HYPRE_EXEC_DEVICE = 1
HYPRE_ERROR_GENERIC = 1
HYPRE_ERROR_ARG = 4
HYPRE_ERROR_CONV = 256

c_big = C.c_longlong
c_int = C.c_int
c_dbl = C.c_double
vp = C.c_void_p

PROF_SPMV_L0, PROF_RELAX_L0, PROF_DOT, PROF_AXPY = 0, 1, 2, 3
PROF_LEVELS = 16
PROF_LVL_RESID, PROF_LVL_RELAX, PROF_LVL_RESTRICT, PROF_LVL_PROLONG = 4, 4 + 16, 4 + 32, 4 + 48
PROF_LVL_RELAX0 = 4 + 64  # first sweep on a zero guess (runs on the level's zero-guess sub-operator)
PROF_LVL_RELAX_MC = 4 + 80  # colour passes of relax types 40 / 41 / 42 (one launch per (block, colour) range)

ALLREDUCE_FN = C.CFUNCTYPE(None, vp, vp, C.c_size_t, c_int, c_int)
ALLGATHER_FN = C.CFUNCTYPE(None, vp, vp, vp, C.c_size_t)
EXCHANGE_FN = C.CFUNCTYPE(None, vp, c_int, C.POINTER(c_int), C.POINTER(vp), C.POINTER(C.c_size_t), c_int,
                          C.POINTER(c_int), C.POINTER(vp), C.POINTER(C.c_size_t))


class HypreError(RuntimeError):
    pass


_lib = None


def lib():
    """Load the shared library (no compute happens here, so this works without a GPU)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HypreError(
                f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                "(make -C hypre-mini-app_amd). There is no CPU fallback.")
        _lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        _lib.HYPRE_MI_LastErrorMessage.restype = C.c_char_p
        _lib.hypre_MAlloc.restype = vp
        _lib.hypre_MAlloc.argtypes = [C.c_size_t, c_int]
        _lib.hypre_Free.argtypes = [vp, c_int]
        _lib.hypre_Memcpy.argtypes = [vp, vp, C.c_size_t, c_int, c_int]
        _lib.HYPRE_MI_Free.argtypes = [vp]
    return _lib


def _conv(a):
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(vp)
    if isinstance(a, float):
        return c_dbl(a)
    if isinstance(a, (int, np.integer)):
        return a
    return a


def call(name, *args, allow=()):
    """Call an ABI entry point; raise on a non-zero HYPRE_Int unless allowed."""
    fn = getattr(lib(), name)
    rc = fn(*[_conv(a) for a in args])
    if rc != 0 and rc not in allow:
        msg = lib().HYPRE_MI_LastErrorMessage()
        raise HypreError(f"{name} returned {rc}: {msg.decode() if msg else ''}")
    return rc


def init():
    call("HYPRE_Init")
    call("HYPRE_SetMemoryLocation", HYPRE_MEMORY_DEVICE)
    call("HYPRE_SetExecutionPolicy", HYPRE_EXEC_DEVICE)


def finalize():
    call("HYPRE_Finalize")


def big(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def dbl(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def row_partition(total_rows, nproc, iproc):
    """init_row_decomposition, /root/reference/src/HypreSystem.cpp:525-544 (inclusive bounds)."""
    per, rem = divmod(total_rows, nproc)
    ilower = per * iproc + min(iproc, rem)
    iupper = per * (iproc + 1) + min(iproc + 1, rem) - 1
    return ilower, iupper


class IJMatrix:
    def __init__(self, ilower, iupper, jlower=None, jupper=None):
        jlower = ilower if jlower is None else jlower
        jupper = iupper if jupper is None else jupper
        self.h = vp()
        self.ilower, self.iupper = ilower, iupper
        call("HYPRE_IJMatrixCreate", 0, c_big(ilower), c_big(iupper), c_big(jlower), c_big(jupper), C.byref(self.h))
        call("HYPRE_IJMatrixSetObjectType", self.h, HYPRE_PARCSR)
        call("HYPRE_IJMatrixInitialize", self.h)
        self.par = vp()
        call("HYPRE_IJMatrixGetObject", self.h, C.byref(self.par))

    def set_values_coo(self, rows, cols, vals, add=False):
        """One entry per 'row', ncols == NULL -- the shape the driver uses (HypreSystem.cpp:942)."""
        n = len(vals) if not isinstance(vals, int) else None
        fn = "HYPRE_IJMatrixAddToValues2" if add else "HYPRE_IJMatrixSetValues2"
        if isinstance(rows, np.ndarray):
            rows, cols, vals = big(rows), big(cols), dbl(vals)
            # HYPRE_Int nrows: split calls that would overflow int32
            step = 1 << 30
            for s in range(0, len(vals), step):
                e = min(len(vals), s + step)
                call(fn, self.h, e - s, None, rows[s:e], None, cols[s:e], vals[s:e])
        else:
            raise TypeError("numpy arrays expected")
        return n

    def set_values_ptr(self, n, rows_ptr, cols_ptr, vals_ptr, add=False):
        fn = "HYPRE_IJMatrixAddToValues2" if add else "HYPRE_IJMatrixSetValues2"
        step = 1 << 30
        for s in range(0, n, step):
            e = min(n, s + step)
            call(fn, self.h, e - s, None, vp(rows_ptr + 8 * s), None, vp(cols_ptr + 8 * s), vp(vals_ptr + 8 * s))

    def set_values_rows_ptr(self, nrows, ncols_ptr, rows_ptr, row_indexes_ptr, cols_ptr, vals_ptr, add=False):
        """The ncols / row_indexes form: row rows[i] gets ncols[i] entries that start at row_indexes[i] of cols / vals
        (row_indexes_ptr None or 0: packed one row after the other).  Pointers are host or device addresses."""
        fn = "HYPRE_IJMatrixAddToValues2" if add else "HYPRE_IJMatrixSetValues2"
        call(fn, self.h, nrows, vp(ncols_ptr), vp(rows_ptr), vp(row_indexes_ptr) if row_indexes_ptr else None,
             vp(cols_ptr), vp(vals_ptr))

    def initialize(self):
        """On an assembled matrix: opens an update round; the stored values stay."""
        call("HYPRE_IJMatrixInitialize", self.h)

    def set_constant_values(self, v):
        call("HYPRE_IJMatrixSetConstantValues", self.h, c_dbl(v))

    def assemble(self):
        """The first call builds the matrix; a later one closes an update round (set / add calls after the first
        assemble change values of the frozen pattern) and is a no-op when no round is open."""
        call("HYPRE_IJMatrixAssemble", self.h)
        call("HYPRE_IJMatrixGetObject", self.h, C.byref(self.par))

    def destroy(self):
        if self.h:
            call("HYPRE_IJMatrixDestroy", self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class IJVector:
    def __init__(self, jlower, jupper, values=None, ncomp=1):
        """ncomp > 1: a multivector as init_system builds it for non-segregated solves
        (/root/reference/src/HypreSystem.cpp:567-571); values then has shape (ncomp, n)."""
        self.h = vp()
        self.jlower, self.jupper = jlower, jupper
        self.n = jupper - jlower + 1
        self.ncomp = ncomp
        call("HYPRE_IJVectorCreate", 0, c_big(jlower), c_big(jupper), C.byref(self.h))
        call("HYPRE_IJVectorSetObjectType", self.h, HYPRE_PARCSR)
        if ncomp != 1:
            call("HYPRE_IJVectorSetNumComponents", self.h, ncomp)
        call("HYPRE_IJVectorInitialize", self.h)
        self.par = vp()
        call("HYPRE_IJVectorGetObject", self.h, C.byref(self.par))
        if values is not None:
            if ncomp == 1:
                self.set(values)
            else:
                for c in range(ncomp):
                    self.set_component(c)
                    self.set(values[c])
        call("HYPRE_IJVectorAssemble", self.h)

    def set_component(self, c):
        """HYPRE_IJVectorSetComponent, /root/reference/src/HypreSystem.cpp:967"""
        call("HYPRE_IJVectorSetComponent", self.h, c)

    def get_all(self):
        out = np.empty((self.ncomp, self.n))
        for c in range(self.ncomp):
            self.set_component(c)
            out[c] = self.get()
        return out

    def set(self, values):
        values = dbl(values)
        idx = np.arange(self.jlower, self.jupper + 1, dtype=np.int64)
        call("HYPRE_IJVectorSetValues", self.h, self.n, idx, values)

    def fill(self, v):
        call("HYPRE_ParVectorSetConstantValues", self.par, float(v))

    def get(self):
        out = np.empty(self.n)
        if self.n:
            call("HYPRE_IJVectorGetValues", self.h, self.n, None, out)
        return out

    def destroy(self):
        if self.h:
            call("HYPRE_IJVectorDestroy", self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# YAML keys of boomeramg_settings with the app's defaults (HypreSystem.cpp:119-159)
APP_AMG_DEFAULTS = dict(print_level=1, debug_flag=1, coarsen_type=8, cycle_type=1, relax_type=8, num_sweeps=1,
                        smooth_num_sweeps=1, tolerance=0.0, max_iterations=1, relax_order=1, max_levels=20,
                        strong_threshold=0.57)


class BoomerAMG:
    """setup_boomeramg_precond, /root/reference/src/HypreSystem.cpp:119-326, same YAML keys."""

    def __init__(self, **node):
        cfg = dict(APP_AMG_DEFAULTS)
        cfg.update(node)
        self.cfg = cfg
        self.h = vp()
        call("HYPRE_BoomerAMGCreate", C.byref(self.h))
        s = self.h
        call("HYPRE_BoomerAMGSetPrintLevel", s, cfg["print_level"])
        call("HYPRE_BoomerAMGSetDebugFlag", s, cfg["debug_flag"])
        call("HYPRE_BoomerAMGSetCoarsenType", s, cfg["coarsen_type"])
        call("HYPRE_BoomerAMGSetCycleType", s, cfg["cycle_type"])
        if all(k in cfg for k in ("down_relax_type", "up_relax_type", "coarse_relax_type")):
            call("HYPRE_BoomerAMGSetCycleRelaxType", s, cfg["down_relax_type"], 1)
            call("HYPRE_BoomerAMGSetCycleRelaxType", s, cfg["up_relax_type"], 2)
            call("HYPRE_BoomerAMGSetCycleRelaxType", s, cfg["coarse_relax_type"], 3)
        else:
            call("HYPRE_BoomerAMGSetRelaxType", s, cfg["relax_type"])
        if all(k in cfg for k in ("num_down_sweeps", "num_up_sweeps", "num_coarse_sweeps")):
            call("HYPRE_BoomerAMGSetCycleNumSweeps", s, cfg["num_down_sweeps"], 1)
            call("HYPRE_BoomerAMGSetCycleNumSweeps", s, cfg["num_up_sweeps"], 2)
            call("HYPRE_BoomerAMGSetCycleNumSweeps", s, cfg["num_coarse_sweeps"], 3)
        else:
            call("HYPRE_BoomerAMGSetNumSweeps", s, cfg["num_sweeps"])
        call("HYPRE_BoomerAMGSetSmoothNumSweeps", s, cfg["smooth_num_sweeps"])
        call("HYPRE_BoomerAMGSetTol", s, float(cfg["tolerance"]))
        call("HYPRE_BoomerAMGSetMaxIter", s, cfg["max_iterations"])
        call("HYPRE_BoomerAMGSetRelaxOrder", s, cfg["relax_order"])
        call("HYPRE_BoomerAMGSetMaxLevels", s, cfg["max_levels"])
        call("HYPRE_BoomerAMGSetStrongThreshold", s, float(cfg["strong_threshold"]))
        for key, fn, conv in (("interp_type", "HYPRE_BoomerAMGSetInterpType", int),
                              ("num_functions", "HYPRE_BoomerAMGSetNumFunctions", int),  # unknown-based systems AMG
                              ("max_row_sum", "HYPRE_BoomerAMGSetMaxRowSum", float),
                              ("relax_weight", "HYPRE_BoomerAMGSetRelaxWt", float),
                              ("outer_weight", "HYPRE_BoomerAMGSetOuterWt", float),
                              ("min_coarse_size", "HYPRE_BoomerAMGSetMinCoarseSize", int),
                              ("max_coarse_size", "HYPRE_BoomerAMGSetMaxCoarseSize", int),
                              ("seq_threshold", "HYPRE_BoomerAMGSetSeqThreshold", int),
                              ("agg_num_levels", "HYPRE_BoomerAMGSetAggNumLevels", int),
                              ("agg_interp_type", "HYPRE_BoomerAMGSetAggInterpType", int),
                              ("agg_pmax_elmts", "HYPRE_BoomerAMGSetAggPMaxElmts", int),
                              ("pmax_elmts", "HYPRE_BoomerAMGSetAggPMaxElmts", int),  # sic, HypreSystem.cpp:210-213
                              ("agg_trunc_factor", "HYPRE_BoomerAMGSetAggTruncFactor", float),
                              ("agg_p12_max_elmts", "HYPRE_BoomerAMGSetAggP12MaxElmts", int),
                              ("agg_p12_trunc_factor", "HYPRE_BoomerAMGSetAggP12TruncFactor", float),
                              ("trunc_factor", "HYPRE_BoomerAMGSetTruncFactor", float),
                              # restriction 0 = P^T, 1 = approximate ideal restriction
                              ("restriction", "HYPRE_BoomerAMGSetRestriction", int),
                              ("strong_threshold_r", "HYPRE_BoomerAMGSetStrongThresholdR", float),
                              ("filter_threshold_r", "HYPRE_BoomerAMGSetFilterThresholdR", float),
                              ("keep_transpose", "HYPRE_BoomerAMGSetKeepTranspose", int),
                              ("rap2", "HYPRE_BoomerAMGSetRAP2", int),
                              ("smooth_type", "HYPRE_BoomerAMGSetSmoothType", int),  # HypreSystem.cpp:235-320
                              ("smooth_num_sweeps", "HYPRE_BoomerAMGSetSmoothNumSweeps", int),
                              ("smooth_num_levels", "HYPRE_BoomerAMGSetSmoothNumLevels", int),
                              ("ilu_type", "HYPRE_BoomerAMGSetILUType", int),
                              ("ilu_level", "HYPRE_BoomerAMGSetILULevel", int),
                              ("ilu_max_iter", "HYPRE_BoomerAMGSetILUMaxIter", int),
                              ("ilu_tri_solve", "HYPRE_BoomerAMGSetILUTriSolve", int),
                              ("ilu_reordering_type", "HYPRE_BoomerAMGSetILULocalReordering", int),  # 2 = multicolour
                              ("ilu_lower_jacobi_iters", "HYPRE_BoomerAMGSetILULowerJacobiIters", int),
                              ("ilu_upper_jacobi_iters", "HYPRE_BoomerAMGSetILUUpperJacobiIters", int),
                              ("iterative_ilu_algorithm_type", "HYPRE_BoomerAMGSetILUIterSetupType", int),
                              ("iterative_ilu_setup_option", "HYPRE_BoomerAMGSetILUIterSetupOption", int),
                              ("iterative_ilu_max_iterations", "HYPRE_BoomerAMGSetILUIterSetupMaxIter", int),
                              ("iterative_ilu_tolerance", "HYPRE_BoomerAMGSetILUIterSetupTolerance", float),
                              ("fsai_algo_type", "HYPRE_BoomerAMGSetFSAIAlgoType", int),
                              ("fsai_local_solve_type", "HYPRE_BoomerAMGSetFSAILocalSolveType", int),
                              ("fsai_num_levels", "HYPRE_BoomerAMGSetFSAINumLevels", int),
                              ("fsai_threshold", "HYPRE_BoomerAMGSetFSAIThreshold", float),
                              ("fsai_eig_max_iters", "HYPRE_BoomerAMGSetFSAIEigMaxIters", int),
                              ("fsai_max_steps", "HYPRE_BoomerAMGSetFSAIMaxSteps", int),
                              ("fsai_max_step_size", "HYPRE_BoomerAMGSetFSAIMaxStepSize", int),
                              ("fsai_max_nnz_row", "HYPRE_BoomerAMGSetFSAIMaxNnzRow", int),
                              ("fsai_kap_tolerance", "HYPRE_BoomerAMGSetFSAIKapTolerance", float),
                              ("cheby_order", "HYPRE_BoomerAMGSetChebyOrder", int),  # relax type 16
                              ("cheby_fraction", "HYPRE_BoomerAMGSetChebyFraction", float),
                              ("cheby_eig_est", "HYPRE_BoomerAMGSetChebyEigEst", int),
                              ("cheby_variant", "HYPRE_BoomerAMGSetChebyVariant", int),
                              ("cheby_scale", "HYPRE_BoomerAMGSetChebyScale", int),
                              ("true_pmax_elmts", "HYPRE_BoomerAMGSetPMaxElmts", int)):
            if key in cfg:
                call(fn, s, conv(cfg[key]))
        # dof_func: the unknown of every local row (int32 array; default global row mod num_functions).  The library
        # reads it at Setup and never frees it: this object keeps the array alive
        self.dof_func = None
        if cfg.get("dof_func") is not None:
            self.dof_func = np.ascontiguousarray(cfg["dof_func"], dtype=np.int32)
            call("HYPRE_BoomerAMGSetDofFunc", s, self.dof_func)
        # this library's keys: value storage of the levels >= mi_value_storage_first_level (0 fp64, 1 fp32, 2 fp64
        # holding fp32-rounded values); absent keys leave the solver's defaults (MI_HYPRE_VALUE_STORAGE*)
        if "mi_value_storage" in cfg or "mi_value_storage_first_level" in cfg:
            env = os.environ.get
            call("HYPRE_MI_BoomerAMGSetValueStorage", s,
                 int(cfg.get("mi_value_storage", env("MI_HYPRE_VALUE_STORAGE", 0))),
                 int(cfg.get("mi_value_storage_first_level", env("MI_HYPRE_VALUE_STORAGE_FIRST_LEVEL", 1))))
        # setup reuse (0 = every Setup builds from scratch, 1 = refresh the values on the kept structure); the driver's
        # key mi_setup_reuse means the same
        reuse = cfg.get("setup_reuse", cfg.get("mi_setup_reuse"))
        if reuse is not None:
            self.set_setup_reuse(int(reuse))
        if cfg.get("keep_agg_markers"):  # test hook: level_agg_markers() after a setup with agg_interp_type 5
            call("HYPRE_MI_BoomerAMGSetKeepAggMarkers", s, 1)
        # non_galerkin_tol + non_galerkin_level_tols {levels, tolerances}, HypreSystem.cpp:161-176
        if "non_galerkin_tol" in cfg:
            call("HYPRE_BoomerAMGSetNonGalerkinTol", s, float(cfg["non_galerkin_tol"]))
            lt = cfg.get("non_galerkin_level_tols")
            if lt:
                for lev, tol in zip(lt["levels"], lt["tolerances"]):
                    call("HYPRE_BoomerAMGSetLevelNonGalerkinTol", s, float(tol), int(lev))

    def setup(self, A):
        call("HYPRE_BoomerAMGSetup", self.h, A.par, None, None)

    def solve(self, A, b, x):
        call("HYPRE_BoomerAMGSolve", self.h, A.par, b.par, x.par)

    def set_setup_reuse(self, mode):
        """0: every Setup builds from scratch; 1: a Setup on a finished hierarchy of the same matrix and pattern
        refreshes the values and keeps the structure (setup_kind() tells which happened)."""
        call("HYPRE_MI_BoomerAMGSetSetupReuse", self.h, int(mode))

    def setup_kind(self):
        """(kind, reason) of the last Setup: kind 0 never set up, 1 built from scratch, 2 refreshed; reason (kind 1):
        0 reuse off, 1 first Setup or the previous one failed, 2 another matrix or pattern, 3 a structural setting
        changed, 4 a setting the refresh does not cover, 5 more than one rank, 6 the other entry point built it."""
        kind, reason = c_int(), c_int()
        call("HYPRE_MI_BoomerAMGGetSetupKind", self.h, C.byref(kind), C.byref(reason))
        return kind.value, reason.value

    @property
    def num_levels(self):
        n = c_int()
        call("HYPRE_MI_BoomerAMGGetNumLevels", self.h, C.byref(n))
        return n.value

    @property
    def operator_complexity(self):
        v = c_dbl()
        call("HYPRE_MI_BoomerAMGGetOperatorComplexity", self.h, C.byref(v))
        return v.value

    @property
    def setup_seconds(self):
        v = c_dbl()
        call("HYPRE_MI_BoomerAMGGetSetupSeconds", self.h, C.byref(v))
        return v.value

    def level_csr(self, level, which):
        """which: 0 A diag, 1 A offd, 2 P diag, 3 R diag, 4 P offd, 5 R offd -> (ia int64, ja int32, a f64, shape)."""
        nr, nc, nnz = c_int(), c_int(), c_big()
        call("HYPRE_MI_BoomerAMGGetLevelCSRSize", self.h, level, which, C.byref(nr), C.byref(nc), C.byref(nnz))
        ia = np.zeros(nr.value + 1, dtype=np.int64)
        ja = np.zeros(max(nnz.value, 1), dtype=np.int32)
        a = np.zeros(max(nnz.value, 1), dtype=np.float64)
        call("HYPRE_MI_BoomerAMGGetLevelCSR", self.h, level, which, ia, ja, a)
        return ia, ja[: nnz.value], a[: nnz.value], (nr.value, nc.value)

    def level_value_storage(self, level, which):
        """(kind, value_bytes) of an operator after setup; which as in level_csr, or 6 / 8 for the zero-guess
        sub-operators.  kind: 0 fp64, 1 fp32, 2 fp64 holding fp32-rounded values, 8 value dictionary."""
        kind, nbytes = c_int(), c_big()
        call("HYPRE_MI_BoomerAMGGetLevelValueStorage", self.h, level, which, C.byref(kind), C.byref(nbytes))
        return kind.value, nbytes.value

    def level_cf(self, level):
        nr, nc, nnz = c_int(), c_int(), c_big()
        call("HYPRE_MI_BoomerAMGGetLevelCSRSize", self.h, level, 0, C.byref(nr), C.byref(nc), C.byref(nnz))
        cf = np.zeros(nr.value, dtype=np.int32)
        call("HYPRE_MI_BoomerAMGGetLevelCF", self.h, level, cf)
        return cf

    @property
    def num_functions(self):
        k = c_int()
        call("HYPRE_BoomerAMGGetNumFunctions", self.h, C.byref(k))
        return k.value

    def level_dof_func(self, level):
        """The unknown of every row of a level built with num_functions > 1, level_cf's rows."""
        nr, nc, nnz = c_int(), c_int(), c_big()
        call("HYPRE_MI_BoomerAMGGetLevelCSRSize", self.h, level, 0, C.byref(nr), C.byref(nc), C.byref(nnz))
        dof = np.zeros(nr.value, dtype=np.int32)
        call("HYPRE_MI_BoomerAMGGetLevelDofFunc", self.h, level, dof)
        return dof

    def level_colours(self, level):
        """The colouring of a level set up with relax type 40 / 41 / 42 in some slot: (info, colour) with info =
        (colours, colouring rounds, (block, colour) ranges in the C block, ranges in the F block) and colour the colour
        of every row, level_csr's rows."""
        nr, nc, nnz = c_int(), c_int(), c_big()
        call("HYPRE_MI_BoomerAMGGetLevelCSRSize", self.h, level, 0, C.byref(nr), C.byref(nc), C.byref(nnz))
        info = np.zeros(4, dtype=np.int32)
        colour = np.zeros(nr.value, dtype=np.int32)
        call("HYPRE_MI_BoomerAMGGetLevelColours", self.h, level, info, colour)
        return tuple(int(v) for v in info), colour

    def level_norms(self, level):
        """(diagonal, signed l1 norm of the hybrid-GS chunks, signed full l1 norm) of a level, level_csr's rows."""
        nr, nc, nnz = c_int(), c_int(), c_big()
        call("HYPRE_MI_BoomerAMGGetLevelCSRSize", self.h, level, 0, C.byref(nr), C.byref(nc), C.byref(nnz))
        out = [np.zeros(nr.value, dtype=np.float64) for _ in range(3)]
        call("HYPRE_MI_BoomerAMGGetLevelNorms", self.h, level, *out)
        return tuple(out)

    def level_agg_markers(self, level):
        """(stage-1 marker, stage-2 marker) of an aggressive level built with agg_interp_type 5, level_csr's rows."""
        nr, nc, nnz = c_int(), c_int(), c_big()
        call("HYPRE_MI_BoomerAMGGetLevelCSRSize", self.h, level, 0, C.byref(nr), C.byref(nc), C.byref(nnz))
        m1 = np.zeros(nr.value, dtype=np.int32)
        m2 = np.zeros(nr.value, dtype=np.int32)
        call("HYPRE_MI_BoomerAMGGetLevelAggMarkers", self.h, level, m1, m2)
        return m1, m2

    def interp_census(self, level):
        """What the device interpolation kernel ran for the level's P: rows per instantiation, the largest bound and
        the flags fell_back (a bound above 1024: host routine) / host (the kernel was not asked)."""
        out = np.zeros(8, dtype=np.int32)
        call("HYPRE_MI_BoomerAMGGetInterpCensus", self.h, level, out)
        names = ("cap16", "cap32", "try32_kept", "try32_retried", "cap512", "cap1024", "max_bound")
        d = {k: int(v) for k, v in zip(names, out)}
        d["fell_back"], d["host"] = bool(out[7] & 1), bool(out[7] & 2)
        return d

    def restriction_info(self, level):
        """How the level's R was made: kind 0 the transpose of P / 1 approximate ideal restriction built by the device /
        2 by the host routine, the largest F-neighbourhood, the C rows with an empty one, the entries the filter dropped."""
        out = np.zeros(4, dtype=np.int32)
        call("HYPRE_MI_BoomerAMGGetRestrictionInfo", self.h, level, out)
        return {k: int(v) for k, v in zip(("kind", "max_m", "zero_rows", "dropped"), out)}

    def level_perm(self, level):
        """perm[new local row] = old local row of the level's C-first ordering."""
        nr, nc, nnz = c_int(), c_int(), c_big()
        call("HYPRE_MI_BoomerAMGGetLevelCSRSize", self.h, level, 0, C.byref(nr), C.byref(nc), C.byref(nnz))
        perm = np.zeros(nr.value, dtype=np.int32)
        call("HYPRE_MI_BoomerAMGGetLevelPerm", self.h, level, perm)
        return perm

    def input_ordering(self):
        """(applied, order): the internal locality numbering of the input, order[new] = caller's local row."""
        nr, nc, nnz = c_int(), c_int(), c_big()
        call("HYPRE_MI_BoomerAMGGetLevelCSRSize", self.h, 0, 0, C.byref(nr), C.byref(nc), C.byref(nnz))
        applied = c_int()
        order = np.zeros(nr.value, dtype=np.int32)
        call("HYPRE_MI_BoomerAMGGetInputOrdering", self.h, C.byref(applied), order)
        return bool(applied.value), order

    def level_colmap(self, level):
        nr, nc, nnz = c_int(), c_int(), c_big()
        call("HYPRE_MI_BoomerAMGGetLevelCSRSize", self.h, level, 1, C.byref(nr), C.byref(nc), C.byref(nnz))
        cm = np.zeros(max(nc.value, 1), dtype=np.int64)
        rs = c_big()
        call("HYPRE_MI_BoomerAMGGetLevelColMap", self.h, level, cm, C.byref(rs))
        return cm[: nc.value], rs.value

    def level_offd_colmap(self, level, which):
        """sorted global column ids of an offd block (which: 1 A, 4 P, 5 R)."""
        nr, nc, nnz = c_int(), c_int(), c_big()
        call("HYPRE_MI_BoomerAMGGetLevelCSRSize", self.h, level, which, C.byref(nr), C.byref(nc), C.byref(nnz))
        cm = np.zeros(max(nc.value, 1), dtype=np.int64)
        call("HYPRE_MI_BoomerAMGGetLevelOffdColMap", self.h, level, which, cm)
        return cm[: nc.value]

    def relax_level(self, level, relax_type, points, f, u):
        """One relaxation call of the level on host arrays (relax types 40 / 41 / 42 take points 0)."""
        f = dbl(f)
        u = np.array(u, dtype=np.float64)
        call("HYPRE_MI_BoomerAMGRelaxLevel", self.h, level, relax_type, points, f, u)
        return u

    def relax_pair_level(self, level, relax_type, first, f, u=None):
        """A C/F pair of hybrid-GS passes of the level on host arrays (first +1: C then F); u None = zero guess."""
        f = dbl(f)
        zero = u is None
        u = np.zeros_like(f) if zero else np.array(u, dtype=np.float64)
        call("HYPRE_MI_BoomerAMGRelaxPairLevel", self.h, level, relax_type, first, 1 if zero else 0, f, u)
        return u

    def relax_level_multi(self, level, relax_type, points, f, u):
        """relax_level on nvec = 2 .. 4 vectors at once, as a batched cycle does: f and u of shape (nvec, n)."""
        f = dbl(f)
        u = np.array(u, dtype=np.float64)
        assert f.ndim == 2 and f.shape == u.shape
        call("HYPRE_MI_BoomerAMGRelaxLevelMulti", self.h, level, relax_type, points, f.shape[0], f, u)
        return u

    def relax_pair_level_multi(self, level, relax_type, first, f, u=None):
        """relax_pair_level on nvec = 2 .. 4 vectors at once: f (and u) of shape (nvec, n); u None = zero guess."""
        f = dbl(f)
        assert f.ndim == 2
        zero = u is None
        u = np.zeros_like(f) if zero else np.array(u, dtype=np.float64)
        assert u.shape == f.shape
        call("HYPRE_MI_BoomerAMGRelaxPairLevelMulti", self.h, level, relax_type, first, 1 if zero else 0, f.shape[0], f, u)
        return u

    # ---- cycle trace (test hooks)
    TRACE_STEPS = ("f_in", "u_in", "u_down", "resid", "u_sub", "u_prolong", "u_up", "u_coarse", "u_collapsed", "u_sweep")
    TRACE_COMPOSITE, TRACE_FILL_SKIPPED, TRACE_DENSE, TRACE_SWEPT, TRACE_COLLAPSED, TRACE_ZERO_GUESS, TRACE_SWEEP_ZERO = \
        1, 2, 4, 8, 16, 32, 64

    def trace_cycle(self, level, f, u0=None, nvec=1, collapse=True):
        """One cycle(level, zero guess iff u0 is None) on host arrays in level_csr's numbering, every step recorded where
        the cycle runs it.  nvec 2 .. 4: f (and u0) of shape (nvec, n), run as a batched cycle.  collapse False: the
        collapsed level cycles like any other.  Returns records (level, visit, step name, values, flags), values of
        shape (n_level,) or (nvec, n_level); a u_sweep record's flags carry which leg (bits 8-9) and sweep (bits 10..)."""
        f = dbl(f)
        assert f.shape[0] == nvec if nvec > 1 else f.ndim == 1
        if u0 is not None:
            u0 = dbl(u0)
            assert u0.shape == f.shape
        nrec = c_int()
        call("HYPRE_MI_BoomerAMGTraceCycle", self.h, level, nvec, 1 if collapse else 0, f, u0, C.byref(nrec))
        out = []
        for i in range(nrec.value):
            info = np.zeros(5, dtype=np.int32)
            call("HYPRE_MI_BoomerAMGGetTraceRecord", self.h, i, info, None)
            vals = np.zeros(max(int(info[4]), 1), dtype=np.float64)
            call("HYPRE_MI_BoomerAMGGetTraceRecord", self.h, i, info, vals)
            vals = vals[: int(info[4])]
            if nvec > 1:
                vals = vals.reshape(nvec, -1)
            out.append((int(info[0]), int(info[1]), self.TRACE_STEPS[int(info[2])], vals, int(info[3])))
        return out

    def level_cycle_info(self, level):
        """dict(r_row_mapped, t_from, has_Ar, has_Az, nc, collapsed_level): the state of a level the cycle's steps
        depend on."""
        out = np.zeros(6, dtype=np.int32)
        call("HYPRE_MI_BoomerAMGGetLevelCycleInfo", self.h, level, out)
        return dict(r_row_mapped=bool(out[0]), t_from=int(out[1]), has_Ar=bool(out[2]), has_Az=bool(out[3]),
                    nc=int(out[4]), collapsed_level=int(out[5]))

    def collapsed_tail(self):
        """(level, B): the tabulated map u = B f of the collapsed coarse tail (n x n, level's numbering); (-1, None)
        without one."""
        level, n = c_int(), c_int()
        call("HYPRE_MI_BoomerAMGGetCollapsedTail", self.h, C.byref(level), C.byref(n), None)
        if level.value < 0:
            return -1, None
        Bt = np.zeros((n.value, n.value), dtype=np.float64)
        call("HYPRE_MI_BoomerAMGGetCollapsedTail", self.h, C.byref(level), C.byref(n), Bt)
        return level.value, np.ascontiguousarray(Bt.T)

    def c_row_handover_census(self, level=0):
        """dict(tiles, listed, handed, flagged_c_rows, w_upto): the tiles of the level's operator, those the mat-vec
        after a C-row hand-over still runs, the handed-over ones, the C rows with an off-diagonal C column, and the row
        at which the last handed-over tile ends."""
        out = np.zeros(5, dtype=np.int64)
        call("HYPRE_MI_BoomerAMGGetCRowHandoverCensus", self.h, level, out)
        return dict(zip(("tiles", "listed", "handed", "flagged_c_rows", "w_upto"), (int(v) for v in out)))

    def cycle_then_matvec(self, f):
        """(z, w, w_full, raised): one cycle from a zero guess on f with the hand-over target set, w = A z by the path
        the current mode takes, w_full by the full mat-vec; arrays in level 0's ordering (level_csr(0, 0)'s rows)."""
        f = dbl(f)
        z, w, wf = np.zeros_like(f), np.zeros_like(f), np.zeros_like(f)
        raised = c_int()
        call("HYPRE_MI_BoomerAMGCycleThenMatvec", self.h, f, z, w, wf, C.byref(raised))
        return z, w, wf, bool(raised.value)

    def gs_sweep_paths(self, level, points, zero_guess=False):
        """Host-side census of the tile GS kernel's sweep branches for one pass: None when the pass does not run on
        the tile kernel, else dict(waves, idle, diagonal, zero, general)."""
        on = c_int()
        counts = np.zeros(5, dtype=np.int64)
        call("HYPRE_MI_BoomerAMGGetGSSweepPaths", self.h, level, points, 1 if zero_guess else 0, C.byref(on), counts)
        if not on.value:
            return None
        return dict(zip(("waves", "idle", "diagonal", "zero", "general"), (int(c) for c in counts)))

    def set_fsai(self, **kw):
        """Change FSAI smoother parameters (fsai_* keys of the constructor), also after setup."""
        names = {"fsai_algo_type": ("HYPRE_BoomerAMGSetFSAIAlgoType", int),
                 "fsai_num_levels": ("HYPRE_BoomerAMGSetFSAINumLevels", int),
                 "fsai_threshold": ("HYPRE_BoomerAMGSetFSAIThreshold", float),
                 "fsai_eig_max_iters": ("HYPRE_BoomerAMGSetFSAIEigMaxIters", int),
                 "fsai_max_steps": ("HYPRE_BoomerAMGSetFSAIMaxSteps", int),
                 "fsai_max_step_size": ("HYPRE_BoomerAMGSetFSAIMaxStepSize", int),
                 "fsai_kap_tolerance": ("HYPRE_BoomerAMGSetFSAIKapTolerance", float)}
        for k, v in kw.items():
            fn, conv = names[k]
            call(fn, self.h, conv(v))
            self.cfg[k] = v

    def set_cheby(self, **kw):
        """Change Chebyshev parameters (cheby_* keys of the constructor), also after setup."""
        names = {"cheby_order": ("HYPRE_BoomerAMGSetChebyOrder", int),
                 "cheby_fraction": ("HYPRE_BoomerAMGSetChebyFraction", float),
                 "cheby_eig_est": ("HYPRE_BoomerAMGSetChebyEigEst", int),
                 "cheby_variant": ("HYPRE_BoomerAMGSetChebyVariant", int),
                 "cheby_scale": ("HYPRE_BoomerAMGSetChebyScale", int)}
        for k, v in kw.items():
            fn, conv = names[k]
            call(fn, self.h, conv(v))
            self.cfg[k] = v

    def level_cheby(self, level):
        """Chebyshev data of a level set up with relax type 16 in some slot: dict(eig_min, eig_max, lower, upper,
        theta, delta) of D^-1 A; raises when the level has none."""
        out = np.zeros(6, dtype=np.float64)
        call("HYPRE_MI_BoomerAMGGetLevelCheby", self.h, level, out)
        return dict(zip(("eig_min", "eig_max", "lower", "upper", "theta", "delta"), (float(v) for v in out)))

    def level_fsai(self, level):
        """(ia int64, ja int32, a f64, omega) of the level's FSAI factor G (GetLevelCSR numbering); None without one."""
        nr, nnz = c_int(), c_big()
        call("HYPRE_MI_BoomerAMGGetLevelFSAISize", self.h, level, C.byref(nr), C.byref(nnz))
        if nr.value == 0 and nnz.value == 0:
            return None
        ia = np.zeros(nr.value + 1, dtype=np.int64)
        ja = np.zeros(max(nnz.value, 1), dtype=np.int32)
        a = np.zeros(max(nnz.value, 1), dtype=np.float64)
        om = c_dbl()
        call("HYPRE_MI_BoomerAMGGetLevelFSAI", self.h, level, ia, ja, a, C.byref(om))
        return ia, ja[: nnz.value], a[: nnz.value], om.value

    def level_fsai_info(self, level):
        """How the level's FSAI factor was built (HYPRE_MI_BoomerAMGGetLevelFSAIInfo): dict with FSAI_INFO_NAMES."""
        out = np.full(8, -2, dtype=np.int32)
        call("HYPRE_MI_BoomerAMGGetLevelFSAIInfo", self.h, level, out)
        return {k: int(v) for k, v in zip(FSAI_INFO_NAMES, out)}

    def level_ilu_ordering(self, level):
        """ILU.ordering() of the level's ILU smoother (smooth_type 5), rows in level_csr's numbering; raises without
        one."""
        nr, nc, nnz = c_int(), c_int(), c_big()
        call("HYPRE_MI_BoomerAMGGetLevelCSRSize", self.h, level, 0, C.byref(nr), C.byref(nc), C.byref(nnz))
        return _ilu_ordering("HYPRE_MI_BoomerAMGGetLevelILUOrdering", nr.value, self.h, level)

    def smooth_level(self, level, f, u=None):
        """One complex-smoother step of the level on host arrays; u None = zero guess."""
        f = dbl(f)
        zero = u is None
        u = np.zeros_like(f) if zero else np.array(u, dtype=np.float64)
        call("HYPRE_MI_BoomerAMGSmoothLevel", self.h, level, 1 if zero else 0, f, u)
        return u

    def destroy(self):
        if self.h:
            call("HYPRE_BoomerAMGDestroy", self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


ILU_ORDERING_NAMES = ("reordering", "colours", "rounds", "lower_levels", "upper_levels")


def _ilu_ordering(fn, n, *handle):
    """dict with ILU_ORDERING_NAMES, perm and colour (int32, n entries: by block row / by the caller's local row; None
    when no ordering is in force) from HYPRE_MI_ILUGetOrdering or its per-level counterpart."""
    info = np.zeros(5, dtype=np.int32)
    perm = np.zeros(max(n, 1), dtype=np.int32)
    colour = np.zeros(max(n, 1), dtype=np.int32)
    call(fn, *handle, info, perm, colour)
    out = {k: int(v) for k, v in zip(ILU_ORDERING_NAMES, info)}
    on = out["reordering"] != 0
    out["perm"], out["colour"] = (perm[:n], colour[:n]) if on else (None, None)
    return out


class ILU:
    """HYPRE_ILU: block-Jacobi ILU(k) (type 0); usable as a preconditioner (set_precond) or a solver.
    iterative_algorithm_type 1-4 (fill 0): the factors come from fixed-point sweeps."""

    def __init__(self, max_iterations=1, tolerance=0.0, trisolve=1, lower_jacobi_iters=5, upper_jacobi_iters=5,
                 print_level=0, ilu_type=0, fill=0, iterative_algorithm_type=0, iterative_setup_option=0,
                 iterative_max_iterations=100, iterative_tolerance=1e-3, local_reordering=0):
        self.h = vp()
        call("HYPRE_ILUCreate", C.byref(self.h))
        call("HYPRE_ILUSetType", self.h, ilu_type)
        call("HYPRE_ILUSetLocalReordering", self.h, int(local_reordering))  # 2 = multicolour ordering
        call("HYPRE_ILUSetLevelOfFill", self.h, fill)
        call("HYPRE_ILUSetIterativeSetupType", self.h, int(iterative_algorithm_type))
        call("HYPRE_ILUSetIterativeSetupOption", self.h, int(iterative_setup_option))
        call("HYPRE_ILUSetIterativeSetupMaxIter", self.h, int(iterative_max_iterations))
        call("HYPRE_ILUSetIterativeSetupTolerance", self.h, float(iterative_tolerance))
        call("HYPRE_ILUSetMaxIter", self.h, max_iterations)
        call("HYPRE_ILUSetTol", self.h, float(tolerance))
        call("HYPRE_ILUSetTriSolve", self.h, trisolve)
        call("HYPRE_ILUSetLowerJacobiIters", self.h, lower_jacobi_iters)
        call("HYPRE_ILUSetUpperJacobiIters", self.h, upper_jacobi_iters)
        call("HYPRE_ILUSetPrintLevel", self.h, print_level)
        self.solve_fn, self.setup_fn = "HYPRE_ILUSolve", "HYPRE_ILUSetup"

    def setup(self, A):
        call("HYPRE_ILUSetup", self.h, A.par, None, None)

    def solve(self, A, b, x):
        return call("HYPRE_ILUSolve", self.h, A.par, b.par, x.par)

    @property
    def num_iterations(self):
        n = c_int()
        call("HYPRE_ILUGetNumIterations", self.h, C.byref(n))
        return n.value

    @property
    def final_rel_res(self):
        v = c_dbl()
        call("HYPRE_ILUGetFinalRelativeResidualNorm", self.h, C.byref(v))
        return v.value

    def iterative_setup_info(self):
        """(sweeps, last correction, last residual) of the last iterative setup on this rank; -1 = norm not computed."""
        n, c, r = c_int(), c_dbl(), c_dbl()
        call("HYPRE_MI_ILUGetIterativeSetupInfo", self.h, C.byref(n), C.byref(c), C.byref(r))
        return n.value, c.value, r.value

    def iterative_setup_history(self):
        """(corrections, residuals) kept by option bit 16, one entry per sweep for each norm that was computed."""
        nc, nr = c_int(), c_int()
        call("HYPRE_MI_ILUGetIterativeSetupHistory", self.h, C.byref(nc), None, C.byref(nr), None)
        c = np.zeros(max(nc.value, 1))
        r = np.zeros(max(nr.value, 1))
        call("HYPRE_MI_ILUGetIterativeSetupHistory", self.h, C.byref(nc), c, C.byref(nr), r)
        return c[: nc.value], r[: nr.value]

    def ordering(self):
        """dict(reordering, colours, rounds, lower_levels, upper_levels, perm, colour) of the last setup; perm and
        colour (int32, by block row / by the caller's local row) are None when no ordering is in force."""
        nr, nnz = c_int(), c_big()
        call("HYPRE_MI_ILUGetFactorsSize", self.h, C.byref(nr), C.byref(nnz))
        return _ilu_ordering("HYPRE_MI_ILUGetOrdering", nr.value, self.h)

    def factors(self):
        """(ia int64, ja int32, a f64): L (unit diagonal not stored) and U of this rank's block as one CSR -- of the
        reordered block P D P^T when local_reordering 2 is in force (ordering())."""
        nr, nnz = c_int(), c_big()
        call("HYPRE_MI_ILUGetFactorsSize", self.h, C.byref(nr), C.byref(nnz))
        ia = np.zeros(nr.value + 1, dtype=np.int64)
        ja = np.zeros(max(nnz.value, 1), dtype=np.int32)
        a = np.zeros(max(nnz.value, 1), dtype=np.float64)
        call("HYPRE_MI_ILUGetFactors", self.h, ia, ja, a)
        return ia, ja[: nnz.value], a[: nnz.value]

    def destroy(self):
        if self.h:
            call("HYPRE_ILUDestroy", self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:  # noqa: BLE001
            pass


class FSAI:
    """HYPRE_FSAI, static pattern (algo type 3; num_levels, threshold) or adaptive pattern (algo type 4; max_steps,
    max_step_size, kap_tolerance): x += omega G^T G (b - A x); a preconditioner (set_precond) or a solver."""

    def __init__(self, max_iterations=1, tolerance=0.0, zero_guess=1, algo_type=3, num_levels=1, threshold=0.01,
                 eig_max_iters=5, omega=None, print_level=0, max_steps=None, max_step_size=None, kap_tolerance=None):
        self.h = vp()
        call("HYPRE_FSAICreate", C.byref(self.h))
        call("HYPRE_FSAISetAlgoType", self.h, int(algo_type))
        if max_steps is not None:
            call("HYPRE_FSAISetMaxSteps", self.h, int(max_steps))
        if max_step_size is not None:
            call("HYPRE_FSAISetMaxStepSize", self.h, int(max_step_size))
        if kap_tolerance is not None:
            call("HYPRE_FSAISetKapTolerance", self.h, float(kap_tolerance))
        call("HYPRE_FSAISetNumLevels", self.h, int(num_levels))
        call("HYPRE_FSAISetThreshold", self.h, float(threshold))
        call("HYPRE_FSAISetEigMaxIters", self.h, int(eig_max_iters))
        if omega is not None:
            call("HYPRE_FSAISetOmega", self.h, float(omega))
        call("HYPRE_FSAISetMaxIterations", self.h, int(max_iterations))
        call("HYPRE_FSAISetTolerance", self.h, float(tolerance))
        call("HYPRE_FSAISetZeroGuess", self.h, int(zero_guess))
        call("HYPRE_FSAISetPrintLevel", self.h, int(print_level))
        self.solve_fn, self.setup_fn = "HYPRE_FSAISolve", "HYPRE_FSAISetup"

    def setup(self, A):
        call("HYPRE_FSAISetup", self.h, A.par, None, None)

    def solve(self, A, b, x):
        return call("HYPRE_FSAISolve", self.h, A.par, b.par, x.par)

    def setup_info(self):
        """How G was built (HYPRE_MI_FSAIGetSetupInfo): dict with FSAI_INFO_NAMES."""
        out = np.full(8, -2, dtype=np.int32)
        call("HYPRE_MI_FSAIGetSetupInfo", self.h, out)
        return {k: int(v) for k, v in zip(FSAI_INFO_NAMES, out)}

    def destroy(self):
        if self.h:
            call("HYPRE_FSAIDestroy", self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:  # noqa: BLE001
            pass


class _Krylov:
    prefix = None

    def __init__(self, tolerance=1e-5, max_iterations=1000, kspace=10, print_level=4, absolute_tol=None,
                 min_iterations=None):
        """setup_gmres / setup_bicg, /root/reference/src/HypreSystem.cpp:390-404, :423-438 (same defaults);
        absolute_tol / min_iterations: SetAbsoluteTol / SetMinIter when given (the driver never calls them)."""
        self.h = vp()
        call(f"{self.prefix}Create", 0, C.byref(self.h))
        call(f"{self.prefix}SetTol", self.h, float(tolerance))
        call(f"{self.prefix}SetMaxIter", self.h, int(max_iterations))
        if self.prefix.endswith("GMRES"):
            call(f"{self.prefix}SetKDim", self.h, int(kspace))
        call(f"{self.prefix}SetPrintLevel", self.h, int(print_level))
        if absolute_tol is not None:
            call(f"{self.prefix}SetAbsoluteTol", self.h, float(absolute_tol))
        if min_iterations is not None:
            call(f"{self.prefix}SetMinIter", self.h, int(min_iterations))
        self.precond = None

    def set_precond(self, amg):
        """solverPrecondPtr_(solver_, precondSolvePtr_, precondSetupPtr_, precond_), HypreSystem.cpp:687."""
        L = lib()
        solve_fn = getattr(amg, "solve_fn", "HYPRE_BoomerAMGSolve")
        setup_fn = getattr(amg, "setup_fn", "HYPRE_BoomerAMGSetup")
        call(f"{self.prefix}SetPrecond", self.h, C.cast(getattr(L, solve_fn), vp), C.cast(getattr(L, setup_fn), vp), amg.h)
        self.precond = amg

    def setup(self, A, b, x):
        call(f"{self.prefix}Setup", self.h, A.par, b.par, x.par)

    def solve(self, A, b, x, allow_generic=False):
        """0, or HYPRE_ERROR_CONV (256) when max_iterations ended the solve.  allow_generic: also hand out 1
        (HYPRE_ERROR_GENERIC: a NaN ended the solve) instead of raising, with the error flag cleared."""
        allow = (HYPRE_ERROR_CONV, HYPRE_ERROR_GENERIC) if allow_generic else (HYPRE_ERROR_CONV,)
        rc = call(f"{self.prefix}Solve", self.h, A.par, b.par, x.par, allow=allow)
        if rc == HYPRE_ERROR_GENERIC:
            call("HYPRE_ClearAllErrors")
        return rc

    @property
    def num_iterations(self):
        n = c_int()
        call(f"{self.prefix}GetNumIterations", self.h, C.byref(n))
        return n.value

    @property
    def final_rel_res(self):
        v = c_dbl()
        call(f"{self.prefix}GetFinalRelativeResidualNorm", self.h, C.byref(v))
        return v.value

    @property
    def solve_seconds(self):
        v = c_dbl()
        call("HYPRE_MI_KrylovGetSolveSeconds", self.h, C.byref(v))
        return v.value

    def residual_history(self):
        n = c_int()
        buf = np.zeros(4096)
        call("HYPRE_MI_KrylovGetResidualHistory", self.h, buf, len(buf), C.byref(n))
        return buf[: min(n.value, len(buf))].copy()

    def destroy(self):
        if self.h:
            call(f"{self.prefix}Destroy", self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class GMRES(_Krylov):
    prefix = "HYPRE_ParCSRGMRES"


class BiCGSTAB(_Krylov):
    prefix = "HYPRE_ParCSRBiCGSTAB"


class FlexGMRES(_Krylov):
    prefix = "HYPRE_ParCSRFlexGMRES"


class PCG(_Krylov):
    prefix = "HYPRE_ParCSRPCG"

    def __init__(self, *args, two_norm=None, **kw):
        """two_norm 1: the convergence measure is <r, r> / <b, b> instead of <C r, r> / <C b, b>"""
        super().__init__(*args, **kw)
        if two_norm is not None:
            call("HYPRE_ParCSRPCGSetTwoNorm", self.h, int(two_norm))


class COGMRES(_Krylov):
    prefix = "HYPRE_ParCSRCOGMRES"

    def __init__(self, *args, cgs=None, **kw):
        """cgs <= 1: one classical Gram-Schmidt pass per Arnoldi step (the default), cgs >= 2: two"""
        super().__init__(*args, **kw)
        if cgs is not None:
            call("HYPRE_ParCSRCOGMRESSetCGS", self.h, int(cgs))


def laplace3d(nx, ny, nz, stencil, ilower, iupper):
    """Synthetic COO triples + rhs for global rows [ilower, iupper] (library-side generator)."""
    nnz = c_big()
    rows, cols, vals, rhs = vp(), vp(), vp(), vp()
    call("HYPRE_MI_Laplace3D", nx, ny, nz, stencil, c_big(ilower), c_big(iupper), C.byref(nnz), C.byref(rows),
         C.byref(cols), C.byref(vals), C.byref(rhs))
    return dict(nnz=nnz.value, rows=rows.value, cols=cols.value, vals=vals.value, rhs=rhs.value,
                nloc=iupper - ilower + 1)


def laplace3d_free(g):
    for k in ("rows", "cols", "vals", "rhs"):
        if g.get(k):
            lib().HYPRE_MI_Free(vp(g[k]))
            g[k] = None


def laplace3d_device(nx, ny, nz, stencil, ilower, iupper):
    """laplace3d with the arrays generated into device memory (addresses of device arrays; laplace3d_device_free)."""
    nnz = c_big()
    rows, cols, vals, rhs = vp(), vp(), vp(), vp()
    call("HYPRE_MI_Laplace3DDevice", nx, ny, nz, stencil, c_big(ilower), c_big(iupper), C.byref(nnz), C.byref(rows),
         C.byref(cols), C.byref(vals), C.byref(rhs))
    return dict(nnz=nnz.value, rows=rows.value, cols=cols.value, vals=vals.value, rhs=rhs.value,
                nloc=iupper - ilower + 1)


def laplace3d_device_free(g):
    lib().HYPRE_MI_FreeDevice.argtypes = [vp]
    lib().HYPRE_MI_FreeDevice.restype = None
    for k in ("rows", "cols", "vals", "rhs"):
        if g.get(k):
            lib().HYPRE_MI_FreeDevice(vp(g[k]))
            g[k] = None


def counter(name):
    v = C.c_longlong()
    call("HYPRE_MI_GetCounter", name.encode(), C.byref(v))
    return v.value


def assembly_stamp(A):
    """unique per assembly and per closed update round of an IJ matrix"""
    par = A.par if hasattr(A, "par") else A
    v = C.c_ulonglong()
    call("HYPRE_MI_ParCSRGetAssemblyStamp", par, C.byref(v))
    return v.value


def set_value_dictionary(on):
    """value dictionary on / off for the operators placed from now on (process-wide; on by default)"""
    call("HYPRE_MI_SetValueDictionary", 1 if on else 0)


def set_multivector_batch(width):
    """components of a multivector that share one pass over an operator (mat-vecs, BoomerAMG cycles; one rank): 1 =
    component by component, 2 .. 4 = at most that many; process-wide.  The results are the same bits for every width."""
    call("HYPRE_MI_SetMultivectorBatch", int(width))


def multivector_batch():
    v = c_int()
    call("HYPRE_MI_GetMultivectorBatch", C.byref(v))
    return v.value


def parcsr_matvec_multi(alpha, A, x, beta, y):
    """y_c = alpha A x_c + beta y_c for every component of the multivectors x and y (IJVector with ncomp > 1)"""
    call("HYPRE_MI_ParCSRMatrixMatvecMulti", float(alpha), A.par if hasattr(A, "par") else A, x.par, float(beta), y.par)


def set_gmres_keep_directions(on):
    """GMRES / COGMRES behind BoomerAMG update x from the kept directions z_j (on, the default) or apply the
    preconditioner once more, as gmres.c does (off); process-wide, for the solves started afterwards"""
    call("HYPRE_MI_SetGmresKeepDirections", 1 if on else 0)


def set_basis_storage(mode):
    """how GMRES / COGMRES / FlexGMRES store their Krylov basis: 0 fp64 (default), 1 float, 2 fp64 vectors of the
    float-rounded values (mode 1's bit-exact reference); process-wide, for the solves started afterwards, one rank.
    Another mode raises (HYPRE_ERROR_ARG) and leaves the setting."""
    call("HYPRE_MI_SetKrylovBasisStorage", int(mode))


def get_basis_storage():
    v = c_int()
    call("HYPRE_MI_GetKrylovBasisStorage", C.byref(v))
    return v.value


def set_c_row_handover(mode):
    """C-row hand-over of the Krylov loops in BoomerAMG's level ordering: 0 off, 1 (default) when at least 10 % of level
    0's tiles are handed over, 2 whenever one is; process-wide, for the solves started afterwards"""
    call("HYPRE_MI_SetCRowHandover", int(mode))


def parcsr_value_kind(A):
    """0: the device diag block streams plain fp64 values, 8: through a value dictionary"""
    par = A.par if hasattr(A, "par") else A
    v = c_int()
    call("HYPRE_MI_ParCSRGetValueKind", par, C.byref(v))
    return v.value


def parcsr_csr(A, which):
    """A block of an assembled matrix: which 0 host diag, 1 host offd (compressed columns), 2 the diag block as the
    device solve format holds it -> (ia int64, ja int32, a f64, shape)."""
    par = A.par if hasattr(A, "par") else A
    nr, nc, nnz = c_int(), c_int(), c_big()
    call("HYPRE_MI_ParCSRGetCSRSize", par, which, C.byref(nr), C.byref(nc), C.byref(nnz))
    ia = np.zeros(nr.value + 1, dtype=np.int64)
    ja = np.zeros(max(nnz.value, 1), dtype=np.int32)
    a = np.zeros(max(nnz.value, 1), dtype=np.float64)
    call("HYPRE_MI_ParCSRGetCSR", par, which, ia, ja, a)
    return ia, ja[: nnz.value], a[: nnz.value], (nr.value, nc.value)


def parcsr_colmap(A):
    """sorted global column ids of the offd block's compressed columns"""
    par = A.par if hasattr(A, "par") else A
    nr, nc, nnz = c_int(), c_int(), c_big()
    call("HYPRE_MI_ParCSRGetCSRSize", par, 1, C.byref(nr), C.byref(nc), C.byref(nnz))
    cm = np.zeros(max(nc.value, 1), dtype=np.int64)
    call("HYPRE_MI_ParCSRGetColMapOffd", par, cm)
    return cm[: nc.value]


def build_laplace_system(nx, ny, nz, stencil=7, rank=0, size=1):
    """IJ matrix + rhs + zero x for this rank's block rows of the n^3 Laplacian."""
    N = nx * ny * nz
    ilower, iupper = row_partition(N, size, rank)
    A = IJMatrix(ilower, iupper)  # (created before the entries are generated, as the reference's driver does: the library
    g = laplace3d(nx, ny, nz, stencil, ilower, iupper)  # starts mapping device memory as soon as it knows the row count)
    A.set_values_ptr(g["nnz"], g["rows"], g["cols"], g["vals"])
    A.assemble()
    rhs = np.ctypeslib.as_array(C.cast(g["rhs"], C.POINTER(c_dbl)), shape=(g["nloc"],)).copy()
    laplace3d_free(g)
    b = IJVector(ilower, iupper, rhs)
    x = IJVector(ilower, iupper)
    x.fill(0.0)
    return A, b, x, rhs


def profile_enable(pid, capacity=4096):
    call("HYPRE_MI_ProfileEnable", pid, capacity)


def profile_reset():
    call("HYPRE_MI_ProfileReset")


def profile_kernel_name(pid):
    """instantiation (template flags included) of the kernel last launched under the class."""
    buf = C.create_string_buffer(128)
    call("HYPRE_MI_ProfileKernelName", pid, buf, 128)
    return buf.value.decode()


def solve_kernel_choice(family, xcache=False, tile_entries=2048, fp32=False, dictionary=False, epilogue=0, level0=False,
                        chunk=8, tiles=False, nnz=0, nrows=1, rowlen_p95=0):
    """instantiation the library launches for an operator with these properties (no device needed).  family 0: SpMV /
    Jacobi (epilogue 1) / the in-place colour pass of relax types 40 - 42 (epilogue 3), family 1: hybrid Gauss-Seidel."""
    buf = C.create_string_buffer(128)
    call("HYPRE_MI_SolveKernelChoice", family, int(xcache), tile_entries, int(fp32), int(dictionary), epilogue, int(level0),
         chunk, int(tiles), c_big(nnz), nrows, rowlen_p95, buf, 128)
    return buf.value.decode()


def solve_kernel_choice_multi(nvec, family, xcache=False, tile_entries=2048, fp32=False, dictionary=False, epilogue=0,
                              level0=False, chunk=8, tiles=False, nnz=0, nrows=1, rowlen_p95=0):
    """(name, batched): solve_kernel_choice for a pass that serves nvec components of a multivector; batched False = the
    single-vector instantiation, run once per component"""
    buf = C.create_string_buffer(128)
    batched = c_int(-1)
    call("HYPRE_MI_SolveKernelChoiceMulti", nvec, family, int(xcache), tile_entries, int(fp32), int(dictionary), epilogue,
         int(level0), chunk, int(tiles), c_big(nnz), nrows, rowlen_p95, buf, 128, C.byref(batched))
    return buf.value.decode(), bool(batched.value)


def cheby_kernel_choice(xcache=False, tile_entries=2048, fp32=False, dictionary=False):
    """instantiation the library launches for a Chebyshev step (relax type 16) on such an operator (no device needed)."""
    buf = C.create_string_buffer(128)
    call("HYPRE_MI_ChebyKernelChoice", int(xcache), tile_entries, int(fp32), int(dictionary), buf, 128)
    return buf.value.decode()


def profile_get(pid):
    n, tot, mn = C.c_longlong(), c_dbl(), c_dbl()
    call("HYPRE_MI_ProfileGet", pid, C.byref(n), C.byref(tot), C.byref(mn))
    return n.value, tot.value, mn.value


# ---------------------------------------------------------------------------
# torch.distributed transport for the callback communicator (tests only: gloo,
# host buffers).  The benchmark path uses the library's own RCCL communicator.
_comm_keep = []


def init_comm_torch(dist, device=None):
    """Bind the library's communicator to a torch.distributed process group through
    host-buffer callbacks (several ranks may share one GPU this way).  With a gloo group
    the buffers travel as CPU tensors; with an nccl group pass device="cuda" and they are
    staged through device tensors (bench.py's loud fallback when the library's own RCCL
    communicator cannot be created)."""
    import torch

    rank, size = dist.get_rank(), dist.get_world_size()
    np_dt = {0: np.float64, 1: np.int64, 2: np.int32, 3: np.uint8}
    ops = {0: dist.ReduceOp.SUM, 1: dist.ReduceOp.MIN, 2: dist.ReduceOp.MAX}

    def _view(ptr, nbytes, dtype=np.uint8):
        buf = (C.c_char * nbytes).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype)

    def _to(t):
        return t.to(device) if device else t

    def allreduce(ctx, buf, count, dtype, op):
        dt = np_dt[dtype]
        a = _view(buf, count * np.dtype(dt).itemsize, dt)
        if device:
            t = torch.from_numpy(a.copy()).to(device)
            dist.all_reduce(t, op=ops[op])
            a[:] = t.cpu().numpy()
        else:
            dist.all_reduce(torch.from_numpy(a), op=ops[op])

    def allgather(ctx, send, recv, nbytes):
        s = _to(torch.from_numpy(_view(send, nbytes).copy()))
        out = [_to(torch.empty(nbytes, dtype=torch.uint8)) for _ in range(size)]
        dist.all_gather(out, s)
        r = _view(recv, nbytes * size)
        for i, o in enumerate(out):
            r[i * nbytes:(i + 1) * nbytes] = o.cpu().numpy()

    def exchange(ctx, nsend, speers, sptrs, sbytes, nrecv, rpeers, rptrs, rbytes):
        ops_, rbufs = [], []
        for i in range(nrecv):
            t = _to(torch.empty(rbytes[i], dtype=torch.uint8))
            rbufs.append(t)
            ops_.append(dist.P2POp(dist.irecv, t, rpeers[i]))
        keep = []
        for i in range(nsend):
            t = _to(torch.from_numpy(_view(sptrs[i], sbytes[i]).copy()))
            keep.append(t)
            ops_.append(dist.P2POp(dist.isend, t, speers[i]))
        if ops_:
            for r in dist.batch_isend_irecv(ops_):
                r.wait()
        for i in range(nrecv):
            _view(rptrs[i], rbytes[i])[:] = rbufs[i].cpu().numpy()

    cbs = (ALLREDUCE_FN(allreduce), ALLGATHER_FN(allgather), EXCHANGE_FN(exchange))
    _comm_keep.append(cbs)
    call("HYPRE_MI_CommInitCallbacks", None, cbs[0], cbs[1], cbs[2], rank, size)
    return rank, size


def build_laplace_system_host(nx, ny, nz, stencil, rank, size):
    """IJ matrix of this rank's rows, assembled on the HOST only (no device)."""
    N = nx * ny * nz
    ilower, iupper = row_partition(N, size, rank)
    g = laplace3d(nx, ny, nz, stencil, ilower, iupper)
    A = IJMatrix.__new__(IJMatrix)
    A.h = vp()
    A.ilower, A.iupper = ilower, iupper
    call("HYPRE_IJMatrixCreate", 0, c_big(ilower), c_big(iupper), c_big(ilower), c_big(iupper), C.byref(A.h))
    call("HYPRE_IJMatrixSetObjectType", A.h, HYPRE_PARCSR)
    A.par = vp()
    call("HYPRE_IJMatrixGetObject", A.h, C.byref(A.par))
    A.set_values_ptr(g["nnz"], g["rows"], g["cols"], g["vals"])
    call("HYPRE_MI_IJMatrixAssembleHostOnly", A.h)
    rhs = np.ctypeslib.as_array(C.cast(g["rhs"], C.POINTER(c_dbl)), shape=(g["nloc"],)).copy()
    laplace3d_free(g)
    return A, rhs


def halo_plan(A):
    ns, nr = c_int(), c_int()
    call("HYPRE_MI_ParCSRGetHaloPlan", A.par, C.byref(ns), None, None, None, C.byref(nr), None, None, None)
    sp = np.zeros(max(ns.value, 1), dtype=np.int32)
    ss = np.zeros(ns.value + 1, dtype=np.int32)
    rp = np.zeros(max(nr.value, 1), dtype=np.int32)
    rs = np.zeros(nr.value + 1, dtype=np.int32)
    call("HYPRE_MI_ParCSRGetHaloPlan", A.par, C.byref(ns), sp, ss, None, C.byref(nr), rp, rs)
    sm = np.zeros(max(int(ss[-1]), 1), dtype=np.int32)
    call("HYPRE_MI_ParCSRGetHaloPlan", A.par, C.byref(ns), sp, ss, sm, C.byref(nr), rp, rs)
    return dict(send_peers=sp[: ns.value], send_starts=ss, send_map=sm[: int(ss[-1])], recv_peers=rp[: nr.value],
                recv_starts=rs)


def matrix_from_scipy(M, ilower=0, iupper=None):
    """IJ matrix of rows [ilower, iupper] of a scipy sparse matrix (global column ids)."""
    M = M.tocsr()
    iupper = M.shape[0] - 1 if iupper is None else iupper
    coo = M[ilower:iupper + 1].tocoo()
    A = IJMatrix(ilower, iupper)
    A.set_values_coo(coo.row.astype(np.int64) + ilower, coo.col.astype(np.int64), coo.data)
    A.assemble()
    return A


def csr_device_op(op, A, B=None, perm=None, colpos=None):
    """Setup-phase device kernels on scipy CSR matrices: op 0 A@B, 1 A.T, 2 rows of A in perm order with
    columns mapped through colpos.  Returns (ia int64, ja int32, a f64, shape) exactly as the library stores it."""
    def parts(M):
        return (np.ascontiguousarray(M.indptr, dtype=np.int64), np.ascontiguousarray(M.indices, dtype=np.int32),
                np.ascontiguousarray(M.data, dtype=np.float64))
    aia, aja, aa = parts(A)
    if B is not None:
        bia, bja, ba = parts(B)
        bn, bm = B.shape
    else:
        bia = bja = ba = None
        bn = bm = 0
    pp = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
    cp = None if colpos is None else np.ascontiguousarray(colpos, dtype=np.int32)
    nr, nc = c_int(), c_int()
    cia, cja, ca = vp(), vp(), vp()
    call("HYPRE_MI_CSRDeviceOp", op, A.shape[0], A.shape[1], aia, aja, aa, bn, bm, bia, bja, ba, pp, cp,
         C.byref(nr), C.byref(nc), C.byref(cia), C.byref(cja), C.byref(ca))
    ia = np.ctypeslib.as_array(C.cast(cia, C.POINTER(c_big)), shape=(nr.value + 1,)).copy()
    nnz = int(ia[-1])
    ja = np.ctypeslib.as_array(C.cast(cja, C.POINTER(c_int)), shape=(max(nnz, 1),)).copy()[:nnz]
    a = np.ctypeslib.as_array(C.cast(ca, C.POINTER(c_dbl)), shape=(max(nnz, 1),)).copy()[:nnz]
    for ptr in (cia, cja, ca):
        lib().HYPRE_MI_Free(ptr)
    return ia, ja, a, (nr.value, nc.value)


def csr_reuse_op(op, A, pattern, P=None, rowmap=None, colmap=None, lanes=0):
    """The setup-reuse kernels on scipy CSR matrices (ascending columns).  op 0: the values of P^T (A P) on the stored
    entries of `pattern`, in the refresh's order contract; op 1: pattern[r, c] = A[rowmap[r], colmap[c]].  Returns the
    value array of `pattern`; raises HypreError (and leaves the array untouched: the exception's `values`) when a row
    does not fit."""
    def parts(M):
        return (np.ascontiguousarray(M.indptr, dtype=np.int64), np.ascontiguousarray(M.indices, dtype=np.int32),
                np.ascontiguousarray(M.data, dtype=np.float64))
    aia, aja, aa = parts(A)
    cia, cja, _ = parts(pattern)
    if P is not None:
        bia, bja, ba = parts(P)
        bn, bm = P.shape
    else:
        bia = bja = ba = None
        bn = bm = 0
    rm = None if rowmap is None else np.ascontiguousarray(rowmap, dtype=np.int32)
    cm = None if colmap is None else np.ascontiguousarray(colmap, dtype=np.int32)
    out = np.full(max(int(cia[-1]), 1), np.nan)
    bad = c_int(-2)
    try:
        call("HYPRE_MI_CSRReuseOp", op, A.shape[0], A.shape[1], aia, aja, aa, bn, bm, bia, bja, ba, rm, cm, int(lanes),
             pattern.shape[0], pattern.shape[1], cia, cja, out, C.byref(bad))
    except HypreError as e:
        e.values, e.bad_row = out[: int(cia[-1])], bad.value
        raise
    return out[: int(cia[-1])]


def mm_interp_op(interp_type, A, S, cf, trunc_factor=0.0, pmax=0, lanes=0):
    """The device routine of interp_type 16 / 17 (HYPRE_MI_MMInterpOp) on a scipy CSR operator A (ascending columns), the
    pattern of the scipy CSR strength graph S and the marker cf (+1 C, -1 F, -3 special F).  Returns P as
    (ia int64, ja int32, a f64, shape) exactly as the library stores it (a scipy constructor could drop nothing here,
    but the arrays are what the bit comparisons want).  Raises HypreError with `bad_row` set when a row has a zero
    denominator and a non-empty numerator."""
    n = A.shape[0]
    aia = np.ascontiguousarray(A.indptr, dtype=np.int64)
    aja = np.ascontiguousarray(A.indices, dtype=np.int32)
    aa = np.ascontiguousarray(A.data, dtype=np.float64)
    sia = np.ascontiguousarray(S.indptr, dtype=np.int64)
    sja = np.ascontiguousarray(S.indices, dtype=np.int32)
    m = np.ascontiguousarray(cf, dtype=np.int32)
    nc, bad = c_int(), c_int(-2)
    pia, pja, pa = vp(), vp(), vp()
    try:
        call("HYPRE_MI_MMInterpOp", int(interp_type), n, aia, aja, aa, sia, sja, m, float(trunc_factor), int(pmax),
             int(lanes), C.byref(nc), C.byref(pia), C.byref(pja), C.byref(pa), C.byref(bad))
    except HypreError as e:
        e.bad_row = bad.value
        raise
    ia = np.ctypeslib.as_array(C.cast(pia, C.POINTER(c_big)), shape=(n + 1,)).copy()
    nnz = int(ia[-1])
    ja = np.ctypeslib.as_array(C.cast(pja, C.POINTER(c_int)), shape=(max(nnz, 1),)).copy()[:nnz]
    a = np.ctypeslib.as_array(C.cast(pa, C.POINTER(c_dbl)), shape=(max(nnz, 1),)).copy()[:nnz]
    for ptr in (pia, pja, pa):
        lib().HYPRE_MI_Free(ptr)
    return ia, ja, a, (n, nc.value)


def _csr_from_caller(nrows, pia, pja, pa):
    """Copies of malloc'ed CSR arrays (released here): (ia int64, ja int32, a f64)."""
    ia = np.ctypeslib.as_array(C.cast(pia, C.POINTER(c_big)), shape=(nrows + 1,)).copy()
    nnz = int(ia[-1])
    ja = np.ctypeslib.as_array(C.cast(pja, C.POINTER(c_int)), shape=(max(nnz, 1),)).copy()[:nnz]
    a = np.ctypeslib.as_array(C.cast(pa, C.POINTER(c_dbl)), shape=(max(nnz, 1),)).copy()[:nnz]
    for ptr in (pia, pja, pa):
        lib().HYPRE_MI_Free(ptr)
    return ia, ja, a


AIR_INFO_NAMES = ("status", "max_m", "zero_rows", "dropped", "rows16", "rows32", "rows64", "bad_row")


def air_restriction_op(A, cf, strong_threshold_r=0.25, filter_threshold_r=0.0, host=False):
    """The approximate ideal restriction (HYPRE_MI_AIRRestrictionOp) of a scipy CSR operator A (ascending columns) with
    the marker cf (+1 C, -1 F), by the device routine or -- host=True, no GPU needed -- the host routine.  Returns
    (R, info): R = (ia int64, ja int32, a f64, shape) exactly as the library stores it, or None when the device routine
    did not build it (info["status"] == 1: a neighbourhood above 64 entries).  Raises HypreError with `info` set when a
    local system is singular."""
    n = A.shape[0]
    aia = np.ascontiguousarray(A.indptr, dtype=np.int64)
    aja = np.ascontiguousarray(A.indices, dtype=np.int32)
    aa = np.ascontiguousarray(A.data, dtype=np.float64)
    m = np.ascontiguousarray(cf, dtype=np.int32)
    nr = c_int()
    out = np.full(8, -2, dtype=np.int32)
    pia, pja, pa = vp(), vp(), vp()
    try:
        call("HYPRE_MI_AIRRestrictionOp", int(bool(host)), n, aia, aja, aa, m, float(strong_threshold_r),
             float(filter_threshold_r), C.byref(nr), C.byref(pia), C.byref(pja), C.byref(pa), out)
    except HypreError as e:
        e.info = {k: int(v) for k, v in zip(AIR_INFO_NAMES, out)}
        raise
    info = {k: int(v) for k, v in zip(AIR_INFO_NAMES, out)}
    if info["status"] != 0:
        return None, info
    return _csr_from_caller(nr.value, pia, pja, pa) + ((nr.value, n),), info


FSAI_INFO_NAMES = ("status", "max_row", "max_candidates", "overflow_rows", "stop_tolerance", "stop_no_candidate",
                   "stop_max_steps", "bad_row")


def fsai_adaptive_op(B, max_steps=3, max_step_size=5, kap_tolerance=1e-3, table_slots=0, host=False):
    """FSAI with the adaptive pattern (HYPRE_MI_FSAIAdaptiveOp, fsai_algo_type 4) of a scipy CSR block B (ascending
    columns), by the device routine or -- host=True, no GPU needed -- the host routine.  table_slots: 0 = the library's
    LDS table, a small power of two forces rows through the table in global memory (same result).  Returns (G, info):
    G = (ia int64, ja int32, a f64, shape) exactly as the library stores it.  Raises HypreError with `info` set when a
    row fails."""
    n = B.shape[0]
    bia = np.ascontiguousarray(B.indptr, dtype=np.int64)
    bja = np.ascontiguousarray(B.indices, dtype=np.int32)
    ba = np.ascontiguousarray(B.data, dtype=np.float64)
    out = np.full(8, -2, dtype=np.int32)
    pia, pja, pa = vp(), vp(), vp()
    try:
        call("HYPRE_MI_FSAIAdaptiveOp", int(bool(host)), n, bia, bja, ba, int(max_steps), int(max_step_size),
             float(kap_tolerance), int(table_slots), C.byref(pia), C.byref(pja), C.byref(pa), out)
    except HypreError as e:
        e.info = {k: int(v) for k, v in zip(FSAI_INFO_NAMES, out)}
        raise
    info = {k: int(v) for k, v in zip(FSAI_INFO_NAMES, out)}
    return _csr_from_caller(n, pia, pja, pa) + ((n, n),), info


def one_point_interp_op(A, S, cf, host=False):
    """One-point interpolation (HYPRE_MI_OnePointInterpOp) of a scipy CSR operator A with the pattern of the scipy CSR
    strength graph S and the marker cf (+1 C, -1 F, -3 special F), by the device routine or -- host=True -- the host
    routine.  Returns P as (ia int64, ja int32, a f64, shape)."""
    n = A.shape[0]
    aia = np.ascontiguousarray(A.indptr, dtype=np.int64)
    aja = np.ascontiguousarray(A.indices, dtype=np.int32)
    aa = np.ascontiguousarray(A.data, dtype=np.float64)
    sia = np.ascontiguousarray(S.indptr, dtype=np.int64)
    sja = np.ascontiguousarray(S.indices, dtype=np.int32)
    m = np.ascontiguousarray(cf, dtype=np.int32)
    nc = c_int()
    pia, pja, pa = vp(), vp(), vp()
    call("HYPRE_MI_OnePointInterpOp", int(bool(host)), n, aia, aja, aa, sia, sja, m, C.byref(nc), C.byref(pia),
         C.byref(pja), C.byref(pa))
    return _csr_from_caller(n, pia, pja, pa) + ((n, nc.value),)


def same_function_filter_op(A, dof, host=False):
    """The same-function operator (HYPRE_MI_SameFunctionFilterOp) of a square scipy CSR operator A: row i keeps the
    entries a_ij with dof[j] == dof[i] and its diagonal, by the device kernel or -- host=True -- the host routine.
    Returns (ia int64, ja int32, a f64, shape)."""
    n = A.shape[0]
    aia = np.ascontiguousarray(A.indptr, dtype=np.int64)
    aja = np.ascontiguousarray(A.indices, dtype=np.int32)
    aa = np.ascontiguousarray(A.data, dtype=np.float64)
    d = np.ascontiguousarray(dof, dtype=np.int32)
    assert d.shape == (n,)
    pia, pja, pa = vp(), vp(), vp()
    call("HYPRE_MI_SameFunctionFilterOp", int(bool(host)), n, aia, aja, aa, d, C.byref(pia), C.byref(pja), C.byref(pa))
    return _csr_from_caller(n, pia, pja, pa) + ((n, n),)


VEC_MASS_DOT, VEC_MASS_AXPY, VEC_LIN_COMB, VEC_AXPY_DOT, VEC_SCALE_POST = range(5)


def vector_kernel_op(op, vecs, coef, w, scale=1.0, xd=None, init=False, f32=False):
    """One of the Krylov loops' vector kernels on IJVectors (HYPRE_MI_VectorKernelOp, test hook): returns the scalar
    results -- m inner products (VEC_MASS_DOT), one (VEC_AXPY_DOT), (posted doubles, flag word, sequence number) for
    VEC_SCALE_POST, None for the updates.  w (and nothing else) is changed in place on the device.
    f32: the kernel's instantiation on float basis vectors (HYPRE_MI_VectorKernelOpF32: vecs are converted to float
    inside the call; VEC_SCALE_POST rounds w to float values and, given xd, leaves the float basis slot, widened, there)."""
    m = len(coef) if op == VEC_SCALE_POST else len(vecs)
    arr = (vp * max(len(vecs), 1))(*[v.par for v in vecs])
    cf = None if coef is None else dbl(coef)
    out = np.zeros(m + 2)
    call("HYPRE_MI_VectorKernelOpF32" if f32 else "HYPRE_MI_VectorKernelOp", op, m, arr, cf, c_dbl(scale), w.par,
         xd.par if xd is not None else None, 1 if init else 0, out)
    if op == VEC_MASS_DOT:
        return out[:m].copy()
    if op == VEC_AXPY_DOT:
        return float(out[0])
    if op == VEC_SCALE_POST:
        return out[:m].copy(), int(out[m]), int(out[m + 1])
    return None


VEC_MGS_BLOCK = 5
MGS_NB = 8


def mgs_block_pass(prev, nxt, last, c, gram, w, f32=False):
    """One pass of the blocked modified Gram-Schmidt step (k::mgs_block_pass through the test hook): the vectors `prev`
    are subtracted from w with the coefficients the kernel derives from their raw inner products c (MGS_NB doubles)
    and raw Gram rows gram (MGS_NB x (MGS_NB + 1)); then the inner products of the new w with the vectors `nxt`, or,
    in the last pass (nxt empty), with `prev`, and its squared norm.  Returns (sums, h, norm copy): MGS_NB + 1 sums,
    MGS_NB coefficients, the squared norm where the last pass leaves it a second time.  w is changed on the device."""
    vecs = list(prev) + ([] if last else list(nxt))
    arr = (vp * max(len(vecs), 1))(*[v.par for v in vecs])
    cf = dbl(np.concatenate([np.asarray(c, dtype=np.float64).ravel(), np.asarray(gram, dtype=np.float64).ravel()]))
    assert len(cf) == MGS_NB * (MGS_NB + 2)
    out = np.zeros(2 * MGS_NB + 2)
    call("HYPRE_MI_VectorKernelOpF32" if f32 else "HYPRE_MI_VectorKernelOp", VEC_MGS_BLOCK, len(vecs), arr, cf,
         c_dbl(float(len(prev))), w.par, None, 1 if last else 0, out)
    return out[:MGS_NB + 1].copy(), out[MGS_NB + 1:2 * MGS_NB + 1].copy(), float(out[2 * MGS_NB + 1])
