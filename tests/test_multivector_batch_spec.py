"""CPU: the public surface of the multivector batch (no device): the exported and declared symbols, the width switch,
and which instantiation serves nvec components of a multivector (k::choose_stream_kernel / k::choose_gs_kernel with
SolveKernelDesc::nvec, through HYPRE_MI_SolveKernelChoiceMulti).  The expected names are written out."""
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("HYPRE_MI_SetMultivectorBatch", "HYPRE_MI_GetMultivectorBatch", "HYPRE_MI_ParCSRMatrixMatvecMulti",
           "HYPRE_MI_SolveKernelChoiceMulti", "HYPRE_MI_BoomerAMGRelaxLevelMulti", "HYPRE_MI_BoomerAMGRelaxPairLevelMulti")
FP64, FP32, DICT = (False, False), (True, False), (False, True)  # (fp32 array, dictionary) held


def _held(h):
    return dict(fp32=h[0], dictionary=h[1])


def _flags(held, block):
    """the template arguments after NV (and TAG) of a batched instantiation"""
    return {FP64: "false, %d" % block, DICT: "true, %d" % block, FP32: "false, %d, true" % block}[held]


def test_symbols_are_exported_and_declared(mi_lib):
    header = open(os.path.join(ROOT, "include", "HYPRE_mi_ext.h")).read()
    for name in SYMBOLS:
        assert hasattr(mi_lib.lib(), name), name
        assert re.search(r"HYPRE_Int\s+%s\s*\(" % name, header), name
    for name in ("set_multivector_batch", "multivector_batch", "parcsr_matvec_multi", "solve_kernel_choice_multi"):
        assert callable(getattr(mi_lib, name)), name
    for name in ("relax_level_multi", "relax_pair_level_multi"):
        assert callable(getattr(mi_lib.BoomerAMG, name)), name


def test_width_round_trip_and_refusals(mi_lib):
    before = mi_lib.multivector_batch()
    assert 1 <= before <= 4
    try:
        for width in (1, 2, 3, 4):
            mi_lib.set_multivector_batch(width)
            assert mi_lib.multivector_batch() == width
        for width in (0, 5, -1):
            rc = mi_lib.call("HYPRE_MI_SetMultivectorBatch", width, allow=(mi_lib.HYPRE_ERROR_ARG,))
            assert rc == mi_lib.HYPRE_ERROR_ARG, (width, rc)
            mi_lib.call("HYPRE_ClearAllErrors")
            assert mi_lib.multivector_batch() == 4  # a refused width changes nothing
    finally:
        mi_lib.set_multivector_batch(before)


def test_one_component_is_the_single_vector_choice(mi_lib):
    """x cache on / off; tile 2048 / 4096; fp64 / dictionary / fp32; level0 0 / 1; epilogues 0, 1, 3; Gauss-Seidel with
    tiles 0 / 1, chunk 8 and 4, short and long rows"""
    one, multi = mi_lib.solve_kernel_choice, mi_lib.solve_kernel_choice_multi
    flags = (False, True)
    count = 0
    for xcache, tile_entries, held in itertools.product(flags, (2048, 4096), (FP64, DICT, FP32)):
        kw = dict(xcache=xcache, tile_entries=tile_entries, **_held(held))
        for epilogue, level0 in itertools.product((0, 1, 3), flags):
            assert multi(1, 0, epilogue=epilogue, level0=level0, **kw) == (one(0, epilogue=epilogue, level0=level0, **kw), False)
            count += 1
        for chunk, tiles, (avg, p95) in itertools.product((8, 4), flags, ((5, 7), (40, 70), (200, 300))):
            gs = dict(chunk=chunk, tiles=tiles, nnz=avg, nrows=1, rowlen_p95=p95, **kw)
            assert multi(1, 1, **gs) == (one(1, **gs), False)
            count += 1
    assert count == 12 * (6 + 12)


@pytest.mark.parametrize("nvec", [2, 3, 4])
def test_batched_instantiations(mi_lib, nvec):
    one, multi = mi_lib.solve_kernel_choice, mi_lib.solve_kernel_choice_multi
    for tile_entries, held in itertools.product((2048, 4096), (FP64, DICT, FP32)):
        block = 512 if tile_entries == 4096 else 256
        kw = dict(tile_entries=tile_entries, **_held(held))
        # x-cache SpMV, epilogue 0: its own level-0 instantiation on the 2048-entry tiles, as the single-vector kernel
        assert multi(nvec, 0, xcache=True, **kw) == ("spmv_stream_xc_mv<%d, 0, %s>" % (nvec, _flags(held, block)), True)
        tag = 1 if block == 256 else 0
        assert multi(nvec, 0, xcache=True, level0=True, **kw) == \
            ("spmv_stream_xc_mv<%d, %d, %s>" % (nvec, tag, _flags(held, block)), True)
        # tile Gauss-Seidel
        gs = dict(xcache=True, tiles=True, nnz=40, nrows=1, rowlen_p95=40, **kw)
        assert multi(nvec, 1, **gs) == ("gs_tile_mv_k<%d, %s>" % (nvec, _flags(held, block)), True)
        # what has no batched form: the launcher runs the single-vector kernel once per component
        for level0 in (False, True):
            assert multi(nvec, 0, xcache=False, level0=level0, **kw) == (one(0, xcache=False, level0=level0, **kw), False)
            for epilogue in (1, 3):
                for xcache in (False, True):
                    e = dict(xcache=xcache, epilogue=epilogue, level0=level0, **kw)
                    assert multi(nvec, 0, **e) == (one(0, **e), False)
        for changed in (dict(xcache=False), dict(tiles=False), dict(chunk=4)):
            other = dict(gs)
            other.update(changed)
            name, batched = multi(nvec, 1, **other)
            assert (name, batched) == (one(1, **other), False)
            assert name.startswith(("gs_group_k", "gs_dense_k", "gs_hybrid_k")), name
        for avg, p95 in ((5, 7), (12, 16), (200, 300)):  # group, dense and (chunk 4) hybrid rows
            for chunk in (8, 4):
                c = dict(chunk=chunk, nnz=avg, nrows=1, rowlen_p95=p95, xcache=True, **kw)
                assert multi(nvec, 1, **c) == (one(1, **c), False)


def test_the_set_of_batched_instantiations(mi_lib):
    """3 widths x 3 value formats x (wide, level-0, plain) mat-vecs and x (wide, narrow) tile Gauss-Seidel kernels"""
    got = set()
    for nvec, xcache, tile_entries, held, level0, tiles, chunk in itertools.product(
            (2, 3, 4), (False, True), (2048, 4096), (FP64, DICT, FP32, (True, True)), (False, True), (False, True), (8, 4)):
        kw = dict(xcache=xcache, tile_entries=tile_entries, **_held(held))
        for family, extra in ((0, dict(level0=level0)), (1, dict(tiles=tiles, chunk=chunk, nnz=9, nrows=1, rowlen_p95=9))):
            name, batched = mi_lib.solve_kernel_choice_multi(nvec, family, **kw, **extra)
            assert batched == ("_mv" in name)
            if batched:
                got.add(name)
                assert re.match(r"(spmv_stream_xc_mv|gs_tile_mv_k)<%d, " % nvec, name), name
    assert len(got) == 3 * 3 * 3 + 3 * 3 * 2, sorted(got)


def test_bad_widths_are_refused(mi_lib):
    for nvec in (0, 5, -1):
        for family in (0, 1):
            with pytest.raises(mi_lib.HypreError, match="SolveKernelChoiceMulti"):
                mi_lib.solve_kernel_choice_multi(nvec, family, xcache=True, tiles=True)
            mi_lib.call("HYPRE_ClearAllErrors")
    for kw in (dict(family=2), dict(tile_entries=1024), dict(epilogue=2), dict(chunk=0), dict(nrows=0)):
        args = dict(nvec=2, family=0)
        args.update(kw)
        with pytest.raises(mi_lib.HypreError, match="SolveKernelChoiceMulti"):
            mi_lib.solve_kernel_choice_multi(**args)
        mi_lib.call("HYPRE_ClearAllErrors")
