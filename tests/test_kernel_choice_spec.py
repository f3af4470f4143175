"""CPU: which instantiation of the solve kernels runs for which operator (k::choose_stream_kernel, k::choose_gs_kernel,
through HYPRE_MI_SolveKernelChoice).  The expected names are written out; nothing here is derived from the library."""
import itertools

import pytest

FP64, FP32, DICT, BOTH = (False, False), (True, False), (False, True), (True, True)  # (fp32 array, dictionary) held

# x cache, per tile size and value arrays: mat-vec, mat-vec of the level-0 class, Jacobi
XC = {
    (2048, FP64): ("spmv_stream_xc<0, 0, false, 256>", "spmv_stream_xc<0, 1, false, 256>", "spmv_stream_xc<1, 0, false, 256>"),
    (2048, DICT): ("spmv_stream_xc<0, 0, true, 256>", "spmv_stream_xc<0, 1, true, 256>", "spmv_stream_xc<1, 0, true, 256>"),
    (2048, FP32): ("spmv_stream_xc<0, 0, false, 256, true>", "spmv_stream_xc<0, 1, false, 256, true>",
                   "spmv_stream_xc<1, 0, false, 256, true>"),
    (4096, FP64): ("spmv_stream_xc<0, 0, false, 512>", "spmv_stream_xc<0, 0, false, 512>", "spmv_stream_xc<1, 0, false, 512>"),
    (4096, DICT): ("spmv_stream_xc<0, 0, true, 512>", "spmv_stream_xc<0, 0, true, 512>", "spmv_stream_xc<1, 0, true, 512>"),
    (4096, FP32): ("spmv_stream_xc<0, 0, false, 512, true>", "spmv_stream_xc<0, 0, false, 512, true>",
                   "spmv_stream_xc<1, 0, false, 512, true>"),
}
# no x cache (either tile size; a dictionary is not looked at)
PLAIN = {
    FP64: ("spmv_stream<0, 0>", "spmv_stream<0, 1>", "spmv_stream<1, 0>"),
    DICT: ("spmv_stream<0, 0>", "spmv_stream<0, 1>", "spmv_stream<1, 0>"),
    FP32: ("spmv_stream<0, 0, float>", "spmv_stream<0, 1, float>", "spmv_stream<1, 0, float>"),
}
TILE = {
    (2048, FP64): "gs_tile_k<false, 256>", (2048, DICT): "gs_tile_k<true, 256>", (2048, FP32): "gs_tile_k<false, 256, true>",
    (4096, FP64): "gs_tile_k<false, 512>", (4096, DICT): "gs_tile_k<true, 512>", (4096, FP32): "gs_tile_k<false, 512, true>",
}
# chunk 8 without tiles: (nnz of the one row = the mean row length, 95th percentile) -> kernel; every threshold from both sides
CHUNK = [
    (8, 8, "gs_group_k<8, 1>"), (8, 9, "gs_group_k<8, 2>"), (1, 0, "gs_group_k<8, 1>"), (3, 500, "gs_group_k<8, 2>"),
    (9, 8, "gs_dense_k<16, 1>"), (9, 16, "gs_dense_k<16, 1>"), (16, 16, "gs_dense_k<16, 1>"), (9, 17, "gs_dense_k<16, 2>"),
    (16, 17, "gs_dense_k<16, 2>"), (16, 500, "gs_dense_k<16, 2>"),
    (17, 16, "gs_dense_k<32, 1>"), (17, 64, "gs_dense_k<32, 1>"), (32, 64, "gs_dense_k<32, 1>"), (17, 65, "gs_dense_k<32, 2>"),
    (32, 65, "gs_dense_k<32, 2>"), (32, 129, "gs_dense_k<32, 2>"),
    (33, 8, "gs_dense_k<64, 1>"), (33, 64, "gs_dense_k<64, 1>"), (33, 65, "gs_dense_k<64, 2>"), (33, 128, "gs_dense_k<64, 2>"),
    (33, 129, "gs_dense_k<64, 4>"), (5000, 128, "gs_dense_k<64, 2>"), (5000, 5000, "gs_dense_k<64, 4>"),
]
CHUNK_NAMES = {"gs_group_k<8, 1>", "gs_group_k<8, 2>", "gs_dense_k<16, 1>", "gs_dense_k<16, 2>", "gs_dense_k<32, 1>",
               "gs_dense_k<32, 2>", "gs_dense_k<64, 1>", "gs_dense_k<64, 2>", "gs_dense_k<64, 4>"}


def _float(name):
    return name[:-1] + ", float>"


def _held(h):
    return dict(fp32=h[0], dictionary=h[1])


@pytest.mark.parametrize("tile_entries", [2048, 4096])
@pytest.mark.parametrize("held", [FP64, FP32, DICT])
def test_spmv_and_jacobi(mi_lib, tile_entries, held):
    pick = mi_lib.solve_kernel_choice
    for xcache, want in ((True, XC[tile_entries, held]), (False, PLAIN[held])):
        kw = dict(xcache=xcache, tile_entries=tile_entries, **_held(held))
        assert pick(0, epilogue=0, **kw) == want[0]
        assert pick(0, epilogue=0, level0=True, **kw) == want[1]
        assert pick(0, epilogue=1, **kw) == want[2]
        assert pick(0, epilogue=1, level0=True, **kw) == want[2]  # TAG belongs to the mat-vec alone
        # what only the Gauss-Seidel family looks at changes nothing
        assert pick(0, epilogue=0, chunk=4, tiles=True, nnz=999, nrows=3, rowlen_p95=70, **kw) == want[0]


def test_tag_stays_0_on_wide_tiles(mi_lib):
    for held in (FP64, FP32, DICT):
        name = mi_lib.solve_kernel_choice(0, xcache=True, tile_entries=4096, epilogue=0, level0=True, **_held(held))
        assert name.startswith("spmv_stream_xc<0, 0, ") and "512" in name, name


def test_fp32_wins_over_the_dictionary(mi_lib):
    pick = mi_lib.solve_kernel_choice
    for tile_entries in (2048, 4096):
        for xcache in (True, False):
            for epilogue, level0 in ((0, False), (0, True), (1, False)):
                kw = dict(xcache=xcache, tile_entries=tile_entries, epilogue=epilogue, level0=level0)
                assert pick(0, **kw, **_held(BOTH)) == pick(0, **kw, **_held(FP32))
        kw = dict(xcache=True, tile_entries=tile_entries, tiles=True, nnz=7, nrows=1)
        assert pick(1, **kw, **_held(BOTH)) == TILE[tile_entries, FP32]
    assert pick(0, xcache=True, **_held(BOTH)) == "spmv_stream_xc<0, 0, false, 256, true>"
    assert pick(1, nnz=9, rowlen_p95=9, **_held(BOTH)) == "gs_dense_k<16, 1, float>"
    assert pick(1, chunk=4, **_held(BOTH)) == "gs_hybrid_k<float>"


@pytest.mark.parametrize("tile_entries", [2048, 4096])
@pytest.mark.parametrize("held", [FP64, FP32, DICT])
def test_tile_gauss_seidel(mi_lib, tile_entries, held):
    pick = mi_lib.solve_kernel_choice
    kw = dict(tile_entries=tile_entries, nnz=40, nrows=1, rowlen_p95=40, **_held(held))
    assert pick(1, xcache=True, tiles=True, **kw) == TILE[tile_entries, held]
    assert pick(1, xcache=True, tiles=True, epilogue=1, level0=True, **kw) == TILE[tile_entries, held]
    # chunk 8, usable tiles and the x cache must all hold
    chunk_name = _float("gs_dense_k<64, 1>") if held == FP32 else "gs_dense_k<64, 1>"
    assert pick(1, xcache=False, tiles=True, **kw) == chunk_name
    assert pick(1, xcache=True, tiles=False, **kw) == chunk_name
    assert pick(1, xcache=True, tiles=True, chunk=4, **kw) == ("gs_hybrid_k<float>" if held == FP32 else "gs_hybrid_k")


@pytest.mark.parametrize("avg,p95,want", CHUNK)
def test_chunk_gauss_seidel(mi_lib, avg, p95, want):
    pick = mi_lib.solve_kernel_choice
    for xcache, tile_entries in ((False, 2048), (True, 2048), (True, 4096)):
        kw = dict(xcache=xcache, tile_entries=tile_entries, nnz=avg, nrows=1, rowlen_p95=p95)
        assert pick(1, **kw) == want
        assert pick(1, dictionary=True, **kw) == want  # the chunk kernels have no dictionary form
        assert pick(1, fp32=True, **kw) == _float(want)
    # the mean is nnz / nrows in floating point, not an integer quotient
    assert pick(1, nnz=avg * 1000, nrows=1000, rowlen_p95=p95) == want
    if avg in (8, 16, 32):
        above = {8: "gs_dense_k<16", 16: "gs_dense_k<32", 32: "gs_dense_k<64"}[avg]
        assert pick(1, nnz=avg * 1000 + 1, nrows=1000, rowlen_p95=p95).startswith(above)


def test_other_chunk_sizes(mi_lib):
    pick = mi_lib.solve_kernel_choice
    for chunk in (1, 4, 7, 9, 16, 32):
        for avg, p95 in ((3, 3), (20, 70), (200, 300)):
            kw = dict(chunk=chunk, nnz=avg, nrows=1, rowlen_p95=p95, xcache=True, tiles=True)
            assert pick(1, **kw) == "gs_hybrid_k" and pick(1, dictionary=True, **kw) == "gs_hybrid_k"
            assert pick(1, fp32=True, **kw) == "gs_hybrid_k<float>"


def test_the_set_of_instantiations(mi_lib):
    """Over the whole input grid: exactly the names of the tables above, 15 + 6 + 6 + 18 + 2 of them."""
    pick = mi_lib.solve_kernel_choice
    want = set(itertools.chain(*XC.values(), *PLAIN.values(), TILE.values(), CHUNK_NAMES, map(_float, CHUNK_NAMES),
                               ("gs_hybrid_k", "gs_hybrid_k<float>")))
    assert len(want) == 15 + 6 + 6 + 18 + 2
    got = set()
    flags = (False, True)
    for xcache, tile_entries, held in itertools.product(flags, (2048, 4096), (FP64, FP32, DICT, BOTH)):
        kw = dict(xcache=xcache, tile_entries=tile_entries, **_held(held))
        for epilogue, level0 in itertools.product((0, 1), flags):
            got.add(pick(0, epilogue=epilogue, level0=level0, **kw))
        for chunk, tiles, avg, p95 in itertools.product((4, 8), flags, (1, 8, 9, 16, 17, 32, 33, 200),
                                                        (0, 8, 9, 16, 17, 64, 65, 128, 129, 1000)):
            got.add(pick(1, chunk=chunk, tiles=tiles, nnz=avg, nrows=1, rowlen_p95=p95, **kw))
    assert got == want, (sorted(got - want), sorted(want - got))


def test_bad_descriptors_are_refused(mi_lib):
    for kw in (dict(family=2), dict(tile_entries=1024), dict(epilogue=2), dict(chunk=0), dict(chunk=33), dict(nrows=0),
               dict(nnz=-1), dict(rowlen_p95=-1)):
        args = dict(family=0)
        args.update(kw)
        with pytest.raises(mi_lib.HypreError, match="SolveKernelChoice"):
            mi_lib.solve_kernel_choice(**args)
        mi_lib.call("HYPRE_ClearAllErrors")
