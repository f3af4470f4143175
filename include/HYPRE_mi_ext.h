/* HYPRE_mi_ext.h -- entry points that HYPRE does not have: rank/GPU binding over
 * RCCL, hierarchy inspection for the parity tests, HIP-event kernel timing for
 * bench.py's roofline figure, and the synthetic problem generator. */
#ifndef HYPRE_MI_EXT_HEADER
#define HYPRE_MI_EXT_HEADER
#include "HYPRE_parcsr_ls.h"
#include "HYPRE_IJ_mv.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- communicator (one rank per GPU).  Replaces the MPI_Comm that libHYPRE
 * takes from src/main.cpp:33-35 / src/HypreSystem.cpp:12-13. */
#define HYPRE_MI_UNIQUE_ID_BYTES 128
HYPRE_Int HYPRE_MI_CommGetUniqueId(void *id128);               /* rank 0, then broadcast by the launcher */
HYPRE_Int HYPRE_MI_CommInitRCCL(const void *id128, HYPRE_Int rank, HYPRE_Int size);
/* RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT (torchrun's env); the id travels over TCP */
HYPRE_Int HYPRE_MI_CommInitFromEnv(void);
/* host-staged transport supplied by the caller (tests: torch.distributed gloo) */
typedef void (*HYPRE_MI_AllreduceFn)(void *ctx, void *buf, size_t count, int dtype /*0 f64,1 i64,2 i32,3 u8*/,
                                     int op /*0 sum,1 min,2 max*/);
typedef void (*HYPRE_MI_AllgatherFn)(void *ctx, const void *send, void *recv, size_t bytes_per_rank);
typedef void (*HYPRE_MI_ExchangeFn)(void *ctx, int nsend, const int *send_peers, void *const *send_ptrs,
                                    const size_t *send_bytes, int nrecv, const int *recv_peers, void *const *recv_ptrs,
                                    const size_t *recv_bytes);
HYPRE_Int HYPRE_MI_CommInitCallbacks(void *ctx, HYPRE_MI_AllreduceFn ar, HYPRE_MI_AllgatherFn ag,
                                     HYPRE_MI_ExchangeFn ex, HYPRE_Int rank, HYPRE_Int size);
/* Neighbour exchange (the halo updates) by peer stores instead of ncclSend/ncclRecv groups, on top of the
 * communicator set up before (RCCL or callbacks; it keeps the reductions and gathers): every rank exports a mailbox
 * arena with hipIpcGetMemHandle, maps the others' (xGMI peer memory; the same device when ranks share a GPU), and one
 * kernel launch per exchange stores the packed halo into the receiver's slot, publishes a sequence number and takes
 * the incoming messages out of its own slots.  slot_bytes: mailbox slot per directed pair and parity (0 = env
 * MI_HYPRE_IPC_SLOT_BYTES or 4 MiB; larger messages travel in parts).  Collective.  Waits are bounded
 * (MI_HYPRE_IPC_TIMEOUT_MS, default 20 000): HYPRE_MI_CommCheck reports a message that never arrived. */
HYPRE_Int HYPRE_MI_CommEnablePeerStoreExchange(HYPRE_BigInt slot_bytes);
HYPRE_Int HYPRE_MI_CommCheck(void);
/* sum all-reduce of `count` doubles in DEVICE memory through the current transport (what an inner product of the
 * Krylov loops does; completed on return).  On the peer-store transport up to 8 doubles take one launch: every rank
 * stores its values into every peer's mailbox and adds the contributions in rank order (identical bits everywhere). */
HYPRE_Int HYPRE_MI_CommAllreduceDevice(HYPRE_Real *dev_buf, HYPRE_Int count);
/* one neighbour exchange of DEVICE buffers through the current transport, on the library stream, completed on return
 * (what a halo update does; for transport tests) */
HYPRE_Int HYPRE_MI_CommExchangeDevice(HYPRE_Int nsend, const HYPRE_Int *send_peers, void *const *send_ptrs,
                                      const size_t *send_bytes, HYPRE_Int nrecv, const HYPRE_Int *recv_peers,
                                      void *const *recv_ptrs, const size_t *recv_bytes);
HYPRE_Int HYPRE_MI_CommName(char *name, HYPRE_Int max_len);
/* one-rank exercise of the RCCL transport (dlopen, init, all-reduce, all-gather, send/recv) */
HYPRE_Int HYPRE_MI_CommSelfTestRCCL(void);
HYPRE_Int HYPRE_MI_CommFinalize(void);
HYPRE_Int HYPRE_MI_CommRank(HYPRE_Int *rank);
HYPRE_Int HYPRE_MI_CommSize(HYPRE_Int *size);
HYPRE_Int HYPRE_MI_CommBarrier(void);
/* blocking all-reduce of a HOST buffer (loaders: src/HypreSystem.cpp:1166-1167, :829) */
HYPRE_Int HYPRE_MI_CommAllreduce(void *buf, size_t count, int dtype, int op);

/* ---- host-only halves of Assemble / Setup (no device needed): the N>1 host logic
 * -- row partition, halo plan, rank-local coarsening, P-row exchange, Galerkin
 * product -- is exercised by world_size-2 gloo tests on CPU through these. */
HYPRE_Int HYPRE_MI_IJMatrixAssembleHostOnly(HYPRE_IJMatrix matrix);
HYPRE_Int HYPRE_MI_BoomerAMGSetupHostOnly(HYPRE_Solver solver, HYPRE_ParCSRMatrix A);
/* arrays may be NULL to query the counts; send_starts/recv_starts hold npeers+1 offsets */
HYPRE_Int HYPRE_MI_ParCSRGetHaloPlan(HYPRE_ParCSRMatrix A, HYPRE_Int *nsend_peers, HYPRE_Int *send_peers,
                                     HYPRE_Int *send_starts, HYPRE_Int *send_map, HYPRE_Int *nrecv_peers,
                                     HYPRE_Int *recv_peers, HYPRE_Int *recv_starts);

/* ---- an assembled matrix as the library holds it (tests of the IJ assembly).  which: 0 the host copy of the diag
 * block (local columns), 1 the host copy of the offd block (compressed columns; their global ids: GetColMapOffd, ncols
 * entries), 2 the diag block read back from the device solve format.  0 and 1 need no device.  Arrays may be NULL. */
HYPRE_Int HYPRE_MI_ParCSRGetCSRSize(HYPRE_ParCSRMatrix A, HYPRE_Int which, HYPRE_Int *nrows, HYPRE_Int *ncols,
                                    HYPRE_BigInt *nnz);
HYPRE_Int HYPRE_MI_ParCSRGetCSR(HYPRE_ParCSRMatrix A, HYPRE_Int which, HYPRE_BigInt *ia, HYPRE_Int *ja, HYPRE_Complex *a);
HYPRE_Int HYPRE_MI_ParCSRGetColMapOffd(HYPRE_ParCSRMatrix A, HYPRE_BigInt *col_map_offd);
/* the assembly stamp: unique per assembly and per closed update round of an IJ matrix (0 = never assembled); a
 * preconditioner set up on another stamp was built from other values */
HYPRE_Int HYPRE_MI_ParCSRGetAssemblyStamp(HYPRE_ParCSRMatrix A, unsigned long long *stamp);
/* how the device diag block streams its values: 0 plain fp64, 8 through a value dictionary (at most 256 distinct values) */
HYPRE_Int HYPRE_MI_ParCSRGetValueKind(HYPRE_ParCSRMatrix A, HYPRE_Int *kind);

/* ---- device / stream */
HYPRE_Int HYPRE_MI_GetStream(void **hip_stream);
HYPRE_Int HYPRE_MI_StreamSynchronize(void);
HYPRE_Int HYPRE_MI_SetGSChunk(HYPRE_Int rows_per_chunk);   /* hybrid-GS "thread" size, default 8 */
HYPRE_Int HYPRE_MI_GetGSChunk(HYPRE_Int *rows_per_chunk);
/* How the first relaxation sweep of a cycle's down leg (zero guess on every level) is run: 0 like any other
 * sweep, 1 without gathering the known zeros, 2 also on the level's zero-guess sub-operator, built by
 * BoomerAMGSetup: the rows' in-chunk entries plus the F rows' C columns -- everything else multiplies zeros; 3
 * (default, env MI_HYPRE_GS_ZERO_SKIP) the residual that follows also reuses the F pass's product with the C values
 * and reads the F rows without their C columns.  Same result up to summation order. */
HYPRE_Int HYPRE_MI_SetZeroGuessMode(HYPRE_Int mode);
/* C-row hand-over: in a Krylov loop that runs in BoomerAMG's level ordering on one rank, the C
 * pass that ends the cycle stores (A z)_i for the level-0 C rows whose only C column is their diagonal, and the
 * mat-vec w = A z that follows leaves out the tiles made of such rows alone.  0 off, 1 (default, env
 * MI_HYPRE_C_HANDOVER) when at least 10 % of level 0's tiles are handed over, 2 whenever one is.  Same result up to
 * summation order.  Counters "handover_matvecs" / "handover_tiles_skipped" (HYPRE_MI_GetCounter). */
HYPRE_Int HYPRE_MI_SetCRowHandover(HYPRE_Int mode);
/* census[0 .. 4] of a level after Setup: tiles of its operator, tiles the reduced mat-vec runs, handed-over tiles,
 * C rows with an off-diagonal C column, the row at which the last handed-over tile ends.  Only level 0 of a one-rank
 * hierarchy swept by the tile kernel has handed-over tiles. */
HYPRE_Int HYPRE_MI_BoomerAMGGetCRowHandoverCensus(HYPRE_Solver solver, HYPRE_Int level, HYPRE_BigInt *census);
/* test hook: one cycle from a zero guess with the hand-over as a Krylov loop asks for it, then the mat-vec: z = M^-1 f,
 * w = A z by the path the mode takes (raised != 0: on the tile list), w_full = A z by the full mat-vec; host arrays in
 * level 0's ordering */
HYPRE_Int HYPRE_MI_BoomerAMGCycleThenMatvec(HYPRE_Solver solver, const HYPRE_Real *f_host, HYPRE_Real *z_host,
                                            HYPRE_Real *w_host, HYPRE_Real *w_full_host, HYPRE_Int *raised);
/* test hook: fill every level's solution / scratch vectors with NaN (a zero-guess cycle that skips its zero-fills must
 * not read them) */
HYPRE_Int HYPRE_MI_BoomerAMGPoisonWorkVectors(HYPRE_Solver solver);
/* test hook: the tile schedule of an operator with the given row pointers (host, n + 1 entries), built by the device
 * routine of the setup (bisection per tile) and by the host routine (the plain greedy loop); *mismatch = 0 when the two
 * agree tile by tile and in the chunk-alignment flag, else 1 + the index of the first tile that differs; *ntiles = the
 * host's tile count.  row_cap: 256 (operators a Gauss-Seidel kernel sweeps) ... 1024 (SpMV only); tile_entries: 2048 / 4096 */
HYPRE_Int HYPRE_MI_TileScheduleCheck(HYPRE_Int n, const HYPRE_BigInt *row_ptr, HYPRE_Int row_cap, HYPRE_Int tile_entries,
                                     HYPRE_Int *ntiles, HYPRE_Int *mismatch);
/* test hook: exactly one of the Krylov loops' vector kernels on this rank's part of ParVectors (every component of a
 * multivector, no collective); device coefficients are uploaded into the scalar slots the solvers use, the call
 * synchronises and copies scalar results into out.  op 0 block inner products out[j] = <vecs[j], w> (m <= 120); 1 block
 * update w += sum_j (scale * coef[j]) vecs[j] (m <= 120); 2 linear combination w = (init != 0) or w += sum_j coef[j]
 * vecs[j] (m <= 250); 3 fused update and inner product w += (scale * coef[0]) vecs[0], out[0] = <xd, w> (xd NULL:
 * <w, w>), m = 1; 4 the scaling kernel that posts an Arnoldi step's Hessenberg column to the host: w *= 1 / sqrt(coef[0])
 * when coef[0] > 0, out[0 .. m) = the m posted doubles (coef as the slots held them), out[m] = the flag word after the
 * kernel, out[m + 1] = the sequence number it was given (m <= 255); 5 one pass of the blocked modified Gram-Schmidt
 * step over blocks of NB = 8 vectors: scale = m_prev, vecs = the m_prev vectors subtracted, then the m - m_prev
 * vectors measured (init != 0: the last pass, m = m_prev), coef = NB raw inner products, then NB raw Gram rows of
 * NB + 1 doubles; out[0 .. NB] = the pass's sums, out[NB + 1 .. 2 NB] = the coefficients, out[2 NB + 1] = the last pass's
 * second copy of the squared norm (m <= 2 NB).  The block kernels work in passes of 8 vectors. */
HYPRE_Int HYPRE_MI_VectorKernelOp(HYPRE_Int op, HYPRE_Int m, HYPRE_ParVector *vecs, const HYPRE_Real *coef,
                                  HYPRE_Real scale, HYPRE_ParVector w, HYPRE_ParVector xd, HYPRE_Int init,
                                  HYPRE_Real *out);
/* test hook: the same kernels instantiated on float basis vectors (HYPRE_MI_SetKrylovBasisStorage mode 1).  `vecs` are
 * converted to float storage (round to nearest even) inside the call; w, the coefficients and all results stay double.
 * Ops 0, 1, 2 and 5 as above.  Op 4 runs the rounding variant of the posting scaling: w = rd(w / sqrt(coef[0])) with
 * rd(v) = (double)(float)v, and the float basis slot the kernel also writes starts as xd's values converted and comes back
 * widened in xd (xd may be NULL); the posted doubles and the flag are as above.  Op 3 is refused. */
HYPRE_Int HYPRE_MI_VectorKernelOpF32(HYPRE_Int op, HYPRE_Int m, HYPRE_ParVector *vecs, const HYPRE_Real *coef,
                                     HYPRE_Real scale, HYPRE_ParVector w, HYPRE_ParVector xd, HYPRE_Int init,
                                     HYPRE_Real *out);
/* test hook: a seeded storm of device allocations / releases of every size through the library's allocator (arena, block
 * cache or plain, whatever MI_HYPRE_POOL says), every block pattern-filled and checked before its release */
HYPRE_Int HYPRE_MI_ArenaSelfTest(HYPRE_Int seed, HYPRE_Int rounds, HYPRE_BigInt max_block_bytes, HYPRE_BigInt *verified,
                                 HYPRE_BigInt *peak_bytes);
/* Value dictionary of operators with at most 256 distinct values (constant-coefficient stencils such as the
 * reference generator's 26 / -1, /root/reference/src/laplace_3d_weak_scaling.hpp:558,600): one byte per entry instead
 * of the 8-byte value in the matrix stream; same doubles, same results.  on = 0 keeps the plain stream -- what a
 * general (variable-coefficient) operator gets anyway; applies to hierarchies set up afterwards (env
 * MI_HYPRE_VALUE_DICT).  bench.py uses it to report the general-operator roofline beside the headline. */
HYPRE_Int HYPRE_MI_SetValueDictionary(HYPRE_Int on);
/* Multivectors (HYPRE_IJVectorSetNumComponents > 1): how many components share one pass over an
 * operator in the mat-vecs and BoomerAMG cycles of a solve on one rank.  1 (the default; environment MI_HYPRE_MV_BATCH):
 * component by component; 2, 3, 4: at most that many per pass, more components in groups, in order.  Any other width
 * is refused (HYPRE_ERROR_ARG).  The results are the same bits for every width.  Counters (HYPRE_MI_GetCounter):
 * "mv_batched_cycles" / "mv_batched_matvecs" passes that ran batched, "mv_fallback_cycles" multivector cycles that
 * looped over the components (width 1, more than one rank, a smoother outside the hybrid Gauss-Seidel family). */
HYPRE_Int HYPRE_MI_SetMultivectorBatch(HYPRE_Int width);
HYPRE_Int HYPRE_MI_GetMultivectorBatch(HYPRE_Int *width);
/* y_c = alpha A x_c + beta y_c for every component c of two multivectors with the same number of components (batched
 * as set above; HYPRE_ParCSRMatrixMatvec acts on the current component alone).  x and y must be different vectors */
HYPRE_Int HYPRE_MI_ParCSRMatrixMatvecMulti(HYPRE_Complex alpha, HYPRE_ParCSRMatrix A, HYPRE_ParVector x, HYPRE_Complex beta,
                                           HYPRE_ParVector y);
/* GMRES and COGMRES preconditioned by this library's BoomerAMG (one cycle, zero tolerance, the matrix of its Setup) keep
 * the preconditioned directions z_j = M^-1 p_j of the Arnoldi steps and update x += sum_j y_j z_j, where gmres.c applies
 * the preconditioner once more to sum_j y_j p_j: the cycle is a fixed linear map, so the two are the same update with
 * other rounding, and a solve of m iterations runs m cycles instead of m + 1 per restart cycle.  Cost: one more vector
 * per basis vector in use, allocated step by step; without room for one the solve goes on with the recomputed update.
 * on = 0 restores the recomputed update (env MI_HYPRE_GMRES_KEEP_DIRECTIONS=0); applies to solves started afterwards.
 * N > 1 ranks: set it alike on every rank (the ranks agree per solve on whether all of them can keep). */
HYPRE_Int HYPRE_MI_SetGmresKeepDirections(HYPRE_Int on);
/* How GMRES, COGMRES and FlexGMRES store their Krylov basis (compressed-basis GMRES).  0 (the
 * default; environment MI_HYPRE_BASIS_STORAGE): fp64.  1: the basis vectors are stored as float -- half the traffic of
 * the Gram-Schmidt passes and half the basis memory; every sum, the Hessenberg matrix, the preconditioner, the kept
 * directions and x stay fp64.  2: fp64 vectors that hold the float-rounded values: the same iteration count, residual
 * history, x and final residual as mode 1, bit for bit (its reference).  Modes 1 and 2 restart from b - A x.  One restart
 * cycle cannot gain more than about 7 digits under them: leave the setting off for tight tolerances asked of a single
 * cycle.  Any other mode is refused (HYPRE_ERROR_ARG) and the setting stays.  Process-wide, applies to solves started
 * afterwards; BiCGSTAB and PCG ignore it.  One rank: a solve on N > 1 ranks under mode 1 or 2 is refused.  Counters
 * (HYPRE_MI_GetCounter): "krylov_basis_fp32_vectors" (float basis vectors allocated), "krylov_basis_bytes" (bytes the
 * basis vectors of the last solve hold). */
HYPRE_Int HYPRE_MI_SetKrylovBasisStorage(HYPRE_Int mode);
HYPRE_Int HYPRE_MI_GetKrylovBasisStorage(HYPRE_Int *mode);
/* test hook: the allocation of the kept direction number `at` (from 0) and of every later one counts as failed in the
 * solves started afterwards; at < 0 = off */
HYPRE_Int HYPRE_MI_TestGmresDirectionAllocFailsAt(HYPRE_Int at);
/* Counters of the multi-rank choreography since the library was loaded: "matvec_overlapped" (SpMVs whose
 * neighbour exchange ran beside the diag-block product), "gs_overlapped" / "gs_in_order" (relaxation passes that
 * swept their halo-free rows while the halo travelled / that waited for it first); collectives of the solve phase
 * on N > 1 ranks: "allreduce" (one per inner product; modified Gram-Schmidt needs i + 1 of them at Arnoldi step i --
 * each coefficient depends on the previous update -- the block classical Gram-Schmidt of COGMRES 2 per step),
 * "halo_exchange" (neighbour send/recv groups), "allgather" (coarsest / redundant levels); the distributed setup:
 * "setup_distributed" (count), "setup_ext_rows_max" (largest per-rank extended sub-problem, rows),
 * "setup_global_rows_gathered" (rows gathered on every rank: the redundant tail only), "setup_device_levels" (levels
 * of the distributed setup whose per-rank pieces were built on the device).
 * IJ assembly: "ij_device_assemblies" (matrices whose batches all arrived in device memory and
 * were assembled there; MI_HYPRE_DEVICE_ASSEMBLY=0 turns the path off), "ij_entries_fetched_to_host" (entries of matrix
 * batches and vector indices copied device -> host: zero for a device assembly), "ij_host_mirror_bytes" (host mirrors
 * downloaded by device assemblies), "ij_device_sort_lds_capacity" (rows with more entries are sorted by the any-length
 * path), "ij_last_kernels_us" / "ij_last_mirror_us" / "ij_last_format_us" (phases of the last device assembly).
 * Krylov solvers: "precond_cycles" (BoomerAMG cycles run as a Krylov solver's preconditioner, one per component of a
 * multivector), "gmres_direction_vectors" (vectors allocated for the directions z_j of FlexGMRES and of
 * HYPRE_MI_SetGmresKeepDirections), "handover_matvecs" / "handover_tiles_skipped" (mat-vecs of a Krylov loop that ran
 * on level 0's tile list after a C-row hand-over, and the tiles they left out). */
HYPRE_Int HYPRE_MI_GetCounter(const char *name, long long *value);
/* One rank's block keeps 32-bit local row ids in the solve format; the entry offsets of its diagonal block are 64-bit
 * (the reference's 27-point operator at 512^3 -- 3.6e9 entries, /root/reference/src/laplace_3d_weak_scaling.hpp:558,600
 * -- assembles and solves on ONE rank, as with HYPRE's bigint / mixedint builds, /root/reference/src/HypreSystem.h:174-219).
 * HYPRE_IJMatrixAssemble refuses (HYPRE_ERROR_ARG + message, never a wrap-around) >= 2147483000 local rows, a halo
 * block or a single row with that many entries.  This applies the same check to a row-pointer array. */
HYPRE_Int HYPRE_MI_CheckBlockRowPointers(HYPRE_BigInt nrows, const HYPRE_BigInt *row_ptr);

/* ---- results the driver never asks HYPRE for */
HYPRE_Int HYPRE_MI_KrylovGetResidualHistory(HYPRE_Solver solver, HYPRE_Real *norms, HYPRE_Int max_n, HYPRE_Int *n);
HYPRE_Int HYPRE_MI_KrylovGetSolveSeconds(HYPRE_Solver solver, HYPRE_Real *seconds);

/* ---- the setup phase's device sparse kernels on caller (host) CSR arrays: op 0 C = A*B,
 * 1 C = A^T, 2 C = rows of A in perm order (perm[new] = old, NULL = identity) with columns mapped through
 * colpos (NULL = identity) and re-sorted.  Bit-identical to the host/oracle arithmetic.  A and B are checked as
 * the other ...Op hooks check theirs (row pointers from 0 that do not decrease, columns in range and strictly
 * ascending within a row; NULL values = zeros): anything else is HYPRE_ERROR_ARG.  Results are malloc'ed: release
 * with HYPRE_MI_Free. */
HYPRE_Int HYPRE_MI_CSRDeviceOp(HYPRE_Int op, HYPRE_Int a_nrows, HYPRE_Int a_ncols, const HYPRE_BigInt *a_ia,
                               const HYPRE_Int *a_ja, const HYPRE_Complex *a_a, HYPRE_Int b_nrows, HYPRE_Int b_ncols,
                               const HYPRE_BigInt *b_ia, const HYPRE_Int *b_ja, const HYPRE_Complex *b_a,
                               const HYPRE_Int *perm, const HYPRE_Int *colpos, HYPRE_Int *c_nrows, HYPRE_Int *c_ncols,
                               HYPRE_BigInt **c_ia, HYPRE_Int **c_ja, HYPRE_Complex **c_a);

/* ---- the setup-reuse kernels ("Setup reuse") on caller (host) CSR arrays with ascending columns.
 * op 0: c_a[stored entry (i, j) of C] = (P^T (A P))_ij, A = (a_*), P = (b_*), summed in the refresh's order contract;
 *       lanes = lanes per coarse row of the kernel (a power of two up to 64; 0 = the library's choice).
 * op 1: c_a[stored entry (r, c) of C] = A[rowmap[r], colmap[c]] (NULL maps: identity).
 * *bad_row = -1, or the first row of C whose pattern does not fit: the call then fails and c_a is untouched. */
HYPRE_Int HYPRE_MI_CSRReuseOp(HYPRE_Int op, HYPRE_Int a_nrows, HYPRE_Int a_ncols, const HYPRE_BigInt *a_ia, const HYPRE_Int *a_ja,
                              const HYPRE_Complex *a_a, HYPRE_Int b_nrows, HYPRE_Int b_ncols, const HYPRE_BigInt *b_ia,
                              const HYPRE_Int *b_ja, const HYPRE_Complex *b_a, const HYPRE_Int *rowmap, const HYPRE_Int *colmap,
                              HYPRE_Int lanes, HYPRE_Int c_nrows, HYPRE_Int c_ncols, const HYPRE_BigInt *c_ia,
                              const HYPRE_Int *c_ja, HYPRE_Complex *c_a, HYPRE_Int *bad_row);

/* ---- the device routine of the matrix-matrix extended interpolation (interp_type 16 extended / 17 extended+i; DESIGN.md
 * section 3) on caller (host) arrays: the n x n operator A as CSR with ascending columns, the pattern of the strength
 * graph S (rows ascending), the marker cf (+1 C, -1 F, -3 special F).  trunc_factor / pmax truncate as Setup does;
 * lanes = lanes per row of the left-operand kernel of type 17 (a power of two up to 64; 0 = the library's choice): the
 * result does not depend on it.  P (n x *p_ncols, columns = the C points in order) is malloc'ed: release with
 * HYPRE_MI_Free.  *bad_row = -1, or the first row whose denominator is zero while its numerator is not empty: the call
 * then fails with HYPRE_ERROR_ARG and P is not made. */
HYPRE_Int HYPRE_MI_MMInterpOp(HYPRE_Int type, HYPRE_Int n, const HYPRE_BigInt *a_ia, const HYPRE_Int *a_ja,
                              const HYPRE_Complex *a_a, const HYPRE_BigInt *s_ia, const HYPRE_Int *s_ja, const HYPRE_Int *cf,
                              HYPRE_Real trunc_factor, HYPRE_Int pmax, HYPRE_Int lanes, HYPRE_Int *p_ncols,
                              HYPRE_BigInt **p_ia, HYPRE_Int **p_ja, HYPRE_Complex **p_a, HYPRE_Int *bad_row);

/* ---- the approximate ideal restriction (HYPRE_BoomerAMGSetRestriction 1) on caller (host) arrays:
 * the n x n operator A as CSR with ascending columns and the final marker cf (+1 C, -1 F).  on_host = 0 runs the device
 * routine, 1 the host routine (which needs no device); both give the same bits.  R (*r_nrows x n, rows = the C points in
 * order, columns ascending) is malloc'ed: release with HYPRE_MI_Free.  info[0] = 0 built / 1 not built (a neighbourhood
 * above 64 entries: the device routine leaves such a level to the host routine; R stays NULL and the call succeeds) /
 * 2 a singular local system (the call fails with HYPRE_ERROR_ARG); info[1] = the largest neighbourhood, info[2] = the C
 * rows with an empty one, info[3] = the entries the filter dropped, info[4..6] = the rows the 16-, 32- and 64-lane
 * instantiation solved (device routine), info[7] = the first singular row or -1. */
HYPRE_Int HYPRE_MI_AIRRestrictionOp(HYPRE_Int on_host, HYPRE_Int n, const HYPRE_BigInt *a_ia, const HYPRE_Int *a_ja,
                                    const HYPRE_Complex *a_a, const HYPRE_Int *cf, HYPRE_Real strong_threshold_r,
                                    HYPRE_Real filter_threshold_r, HYPRE_Int *r_nrows, HYPRE_BigInt **r_ia, HYPRE_Int **r_ja,
                                    HYPRE_Complex **r_a, HYPRE_Int info[8]);
/* ---- FSAI with the adaptive pattern (fsai_algo_type 4 -- this library's number, not HYPRE's, whose adaptive types 1 and
 * 2 are host threading schemes and stay refused) on caller (host) arrays: the n x n block B as CSR
 * with ascending columns.  on_host = 0 runs the device routine, 1 the host routine (which needs no device); both give
 * the same bits.  table_slots = 0: the library's choice of a row's candidate table in LDS; a small power of two sends
 * the rows whose candidates do not fit through the table in global memory -- the result never depends on it.  G (n x n,
 * lower triangular, columns ascending) is malloc'ed: release with HYPRE_MI_Free.  info[0] = 0 built / 2 a row failed
 * (the call fails and names the row), info[1] = the largest row of G, info[2] = the largest candidate count met,
 * info[3] = the rows that took the global-memory table (device routine), info[4..6] = the rows stopped by the tolerance
 * / for want of candidates / by max_steps, info[7] = the first failing row or -1.  Refused: max_steps < 1,
 * max_step_size < 1, max_steps * max_step_size + 1 > 64, kap_tolerance negative or not finite. */
HYPRE_Int HYPRE_MI_FSAIAdaptiveOp(HYPRE_Int on_host, HYPRE_Int n, const HYPRE_BigInt *b_ia, const HYPRE_Int *b_ja,
                                  const HYPRE_Complex *b_a, HYPRE_Int max_steps, HYPRE_Int max_step_size,
                                  HYPRE_Real kap_tolerance, HYPRE_Int table_slots, HYPRE_BigInt **g_ia, HYPRE_Int **g_ja,
                                  HYPRE_Complex **g_a, HYPRE_Int info[8]);
/* the same eight numbers for the G of a HYPRE_FSAI solver that is set up (static pattern: entries 2 ... 6 are 0) */
HYPRE_Int HYPRE_MI_FSAIGetSetupInfo(HYPRE_Solver solver, HYPRE_Int out[8]);
/* ---- one-point interpolation (interp_type 100) on caller (host) arrays: A, the pattern of the
 * strength graph S and the marker cf (+1 C, -1 F, -3 special F); on_host as above.  P (n x *p_ncols) is malloc'ed. */
HYPRE_Int HYPRE_MI_OnePointInterpOp(HYPRE_Int on_host, HYPRE_Int n, const HYPRE_BigInt *a_ia, const HYPRE_Int *a_ja,
                                    const HYPRE_Complex *a_a, const HYPRE_BigInt *s_ia, const HYPRE_Int *s_ja,
                                    const HYPRE_Int *cf, HYPRE_Int *p_ncols, HYPRE_BigInt **p_ia, HYPRE_Int **p_ja,
                                    HYPRE_Complex **p_a);
/* ---- same-function operator of a system with several unknowns (HYPRE_BoomerAMGSetNumFunctions; DESIGN.md section 3,
 * "Systems of PDEs") on caller (host) arrays: row i of the n x n matrix A keeps the entries a_ij with dof[j] == dof[i]
 * and its diagonal, in stored order.  on_host = 0: the device kernel, 1: the host routine (no device needed).  The
 * result is malloc'ed (HYPRE_MI_Free). */
HYPRE_Int HYPRE_MI_SameFunctionFilterOp(HYPRE_Int on_host, HYPRE_Int n, const HYPRE_BigInt *a_ia, const HYPRE_Int *a_ja,
                                        const HYPRE_Complex *a_a, const HYPRE_Int *dof, HYPRE_BigInt **out_ia,
                                        HYPRE_Int **out_ja, HYPRE_Complex **out_a);
/* how R of `level` was made: out[0] = 0 the transpose of P / 1 approximate ideal restriction built by the device / 2 by
 * the host routine; out[1] = the largest neighbourhood, out[2] = the C rows with an empty one, out[3] = the entries the
 * filter dropped */
HYPRE_Int HYPRE_MI_BoomerAMGGetRestrictionInfo(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int out[4]);

/* ---- setup reuse: mode 0 (default) = every Setup builds from scratch; 1 = a Setup on a handle that holds a finished
 * hierarchy of the same matrix object and pattern, built by the same entry point with the same structural settings on
 * one rank, keeps the splittings, orderings, P, R and all patterns and recomputes the values.  A Setup that cannot
 * refresh rebuilds, and says so.  Any other mode is HYPRE_ERROR_ARG.
 * GetSetupKind: kind 0 never set up, 1 built from scratch, 2 refreshed; reason (kind 1): 0 reuse is off, 1 first Setup
 * of this handle or the previous one failed, 2 another matrix object or pattern, 3 a setting the structure depends on
 * changed, 4 a setting the refresh does not cover is on (non-Galerkin tolerances, value storage,
 * restriction 1, interp_type 100, num_functions > 1), 5 more than one rank,
 * 6 the other setup entry point built the hierarchy.  Counters: "amg_setups_full", "amg_setups_refreshed". */
HYPRE_Int HYPRE_MI_BoomerAMGSetSetupReuse(HYPRE_Solver solver, HYPRE_Int mode);
HYPRE_Int HYPRE_MI_BoomerAMGGetSetupKind(HYPRE_Solver solver, HYPRE_Int *kind, HYPRE_Int *reason);
/* the reason of a rebuild in words (a static string; the library's print and the driver's use the same) */
const char *HYPRE_MI_SetupReuseReasonText(HYPRE_Int reason);

/* ---- hierarchy inspection (parity tests; mirrors hypre_ParAMGDataAArray) */
HYPRE_Int HYPRE_MI_BoomerAMGGetNumLevels(HYPRE_Solver solver, HYPRE_Int *num_levels);
HYPRE_Int HYPRE_MI_BoomerAMGGetOperatorComplexity(HYPRE_Solver solver, HYPRE_Real *cx);
HYPRE_Int HYPRE_MI_BoomerAMGGetSetupSeconds(HYPRE_Solver solver, HYPRE_Real *seconds);
/* which: 0 A diag block, 1 A offd block, 2 P diag, 3 R diag, 4 P offd (halo columns), 5 R offd.
 * P (rows: this level, columns: next level) and R = P^T are rectangular ParCSR operators.
 * GetLevelCSRSize also takes which = 6: the level's zero-guess sub-operator (the entries of the diag block a
 * first sweep on a zero guess can meet with a non-zero; 0 x 0 when the level has none), and which = 7: the x cache
 * of the level's diag block (nrows = number of tiles, nnz = unique columns summed over the tiles); which = 8: the
 * operator of the residual after a zero-guess sweep (0 x 0 when the level has none); which = 9: the C rows of the diag
 * block (nrows = number of C points, nnz = their entries: what a C pass of the relaxation streams).
 * GetLevelCSR takes which = 0-5, and 6 and 8 (the sub-operators' arrays, fetched from the device). */
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelCSRSize(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int which, HYPRE_Int *nrows,
                                            HYPRE_Int *ncols, HYPRE_BigInt *nnz);
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelCSR(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int which, HYPRE_BigInt *ia,
                                        HYPRE_Int *ja, HYPRE_Complex *a);
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelCF(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int *cf);
/* the unknown (0 ... num_functions - 1) every row of `level` belongs to, in GetLevelCF's row numbering; fails on a
 * hierarchy built with num_functions 1, which keeps none */
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelDofFunc(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int *dof);
/* The colouring of `level` in a hierarchy set up with relax type 40, 41 or 42 (multicolour Gauss-Seidel, this library's
 * own numbers) in some slot: info = { colours, rounds of the colouring, (block, colour) row ranges in the C block, ranges
 * in the F block }; colour (may be NULL): the colour of every row, in GetLevelCSR's row numbering -- non-decreasing over
 * the C rows and over the F rows.  Fails on a level that was not coloured. */
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelColours(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int info[4], HYPRE_Int *colour);
/* What the smoothers of a level divide by, in GetLevelCSR's row numbering: the diagonal, the l1 norm of the hybrid
 * Gauss-Seidel chunks (C/F aware, replaced by |a_ii| where it is at most 4/3 of it) and the full l1 norm of the row;
 * both norms carry the sign of the diagonal.  Any array may be NULL. */
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelNorms(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Real *diag, HYPRE_Real *l1gs,
                                          HYPRE_Real *l1jac);
/* Value storage of the operators (A, P, R, the zero-guess sub-operators) of the AMG levels >= first_level; call before
 * Setup.  mode 0: fp64 (the default), 1: the values are stored and streamed as fp32 and widened to fp64 where a
 * product is formed, 2: fp64 storage holding the fp32-rounded values (the reference semantics of mode 1: every
 * solve-phase result of the two is the same bit for bit).  Vectors, sums, diagonals, l1 norms, the coarsest dense
 * inverse and the Krylov solver stay fp64; the hierarchy is mode 0's with each stored value v replaced by
 * (double)(float)v.  first_level >= 1: level 0 is the system the Krylov solver multiplies by.  An operator with a
 * finite non-zero value outside the range of normal floats keeps its fp64 values.  Any other mode, or first_level < 1,
 * is HYPRE_ERROR_ARG.  Defaults of a new solver: MI_HYPRE_VALUE_STORAGE (0), MI_HYPRE_VALUE_STORAGE_FIRST_LEVEL (1). */
HYPRE_Int HYPRE_MI_BoomerAMGSetValueStorage(HYPRE_Solver solver, HYPRE_Int mode, HYPRE_Int first_level);
/* What an operator holds after Setup.  which: as in GetLevelCSRSize, 0-5, 6 and 8.  kind: 0 fp64 as built, 1 fp32,
 * 2 fp64 holding fp32-rounded values (halo blocks of a narrowed operator are always of this kind), 8 value dictionary.
 * value_bytes: device bytes of the operator's value arrays, padding included (0 for a hierarchy that is not on the
 * device, where kind is what Setup decided for the operator).  Either output may be NULL. */
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelValueStorage(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int which, HYPRE_Int *kind,
                                                 HYPRE_BigInt *value_bytes);
/* aggressive level built with agg_interp_type 5 (one rank): the markers after the first coarsening (stage1: C1) and
 * after the second one and the marker correction (stage2: C2, special F points still -3), in GetLevelCSR's row
 * numbering.  Either array may be NULL.  The markers are kept only when SetKeepAggMarkers(solver, 1) was called before
 * Setup (two bytes per row of host memory; off by default).  An error on every other level. */
HYPRE_Int HYPRE_MI_BoomerAMGSetKeepAggMarkers(HYPRE_Solver solver, HYPRE_Int keep);
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelAggMarkers(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int *stage1, HYPRE_Int *stage2);
/* What the device interpolation kernel ran to build the level's P (one rank): rows are binned by a
 * bound T on their interpolatory set and every bin has its own instantiation.  out[0..5]: rows taken by the 16-entry
 * tables (T <= 16, C points and empty rows included), the 32-entry tables (T <= 32), the 32-entry tables tried for
 * 33 <= T <= 128 and kept, the same rows given up and rerun in 128-entry tables, the 512-entry tables (T <= 512), the
 * 1024-entry tables (T <= 1024); out[6]: the largest T of the level; out[7]: flags -- 1: a row had T > 1024 and the
 * level's P was handed to the host routine (out[0..5] are zero), 2: the kernel was not asked at all (level set up on
 * the host, another interpolation type, the coarsest level; everything else is zero). */
HYPRE_Int HYPRE_MI_BoomerAMGGetInterpCensus(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int out[8]);
/* the level's C-first ordering: perm[new local row] = old local row (level matrices, P, R and the
 * C/F marker are reported in the NEW ordering; level 0 is a renumbered copy of the caller's matrix) */
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelPerm(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int *perm);
/* Internal locality numbering of the input (one rank, large systems; MI_HYPRE_LOCALITY_ORDER = 0 off / 1 on, unset:
 * at least MI_HYPRE_LOCALITY_MIN_ROWS = 1e6 rows): the hierarchy is built on Q A Q^T where Q groups rows into
 * graph-compact clusters (graph Voronoi cells of ~512 rows, ranked in sweep order) so that tiles of consecutive rows gather few distinct
 * columns.  order[new] = caller's local row (identity and *applied = 0 when not in use); GetLevelPerm(0) already
 * includes it (level-0 row -> caller row). */
HYPRE_Int HYPRE_MI_BoomerAMGGetInputOrdering(HYPRE_Solver solver, HYPRE_Int *applied, HYPRE_Int *order);
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelColMap(HYPRE_Solver solver, HYPRE_Int level, HYPRE_BigInt *col_map_offd,
                                           HYPRE_BigInt *row_start);
/* sorted global column ids of an offd block (which: 1 A, 4 P, 5 R; length = that block's ncols) */
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelOffdColMap(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int which,
                                               HYPRE_BigInt *col_map_offd);
/* one relaxation call / one cycle on HOST arrays of the level's local length */
HYPRE_Int HYPRE_MI_BoomerAMGRelaxLevel(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int relax_type, HYPRE_Int points,
                                       const HYPRE_Real *f_host, HYPRE_Real *u_host);
/* a C/F pair of hybrid Gauss-Seidel passes on HOST arrays, as a cycle runs them (first +1: C then F, -1: F then C);
 * zero_guess != 0 takes u = 0 on entry (u_host is then output only) and sweeps as the first sweep of a down leg does */
HYPRE_Int HYPRE_MI_BoomerAMGRelaxPairLevel(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int relax_type, HYPRE_Int first,
                                           HYPRE_Int zero_guess, const HYPRE_Real *f_host, HYPRE_Real *u_host);
/* the two hooks above on nvec = 2, 3 or 4 vectors at once, as a batched cycle runs them: f_host and
 * u_host hold the components one after the other, each of the level's local length.  Relax types 3, 4, 6, 8, 13, 14; one
 * rank.  Every component comes back with the bits of the single-vector hook on it */
HYPRE_Int HYPRE_MI_BoomerAMGRelaxLevelMulti(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int relax_type, HYPRE_Int points,
                                            HYPRE_Int nvec, const HYPRE_Real *f_host, HYPRE_Real *u_host);
HYPRE_Int HYPRE_MI_BoomerAMGRelaxPairLevelMulti(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int relax_type, HYPRE_Int first,
                                                HYPRE_Int zero_guess, HYPRE_Int nvec, const HYPRE_Real *f_host,
                                                HYPRE_Real *u_host);
/* ---- cycle trace: TEST HOOKS (tests/test_gpu_cycle_steps.py).  No solve path calls them, and a
 * solver that was never traced launches, synchronises and allocates exactly what it did before they existed.
 *
 * TraceCycle runs ONE cycle(level, zero guess iff u0_host == NULL) of the hierarchy on HOST arrays of nvec times the
 * level's local length, in GetLevelCSR's numbering, and records what the cycle's vectors hold after each of its steps,
 * where the cycle runs them (the state a step depends on -- a composite right-hand side, a skipped zero-fill -- is the
 * cycle's own).  nvec 2, 3 or 4 runs it as a batched cycle does (components one after the other); collapse == 0 makes
 * the cycle descend through the level whose sub-cycle is otherwise applied as a tabulated map.  One rank only.
 * *nrecords = the records kept in the solver until the next TraceCycle; GetTraceRecord copies record i:
 *   info[0] level, info[1] visit (0, 1, ... per level within this cycle), info[2] step, info[3] flags, info[4] the
 *   number of values (nvec x that level's rows); values may be NULL to query info.
 * steps: 0 f on entry; 1 u on entry (non-zero guess only); 2 u after the down sweeps; 3 the residual f - A u; 4 (level
 *   l + 1's record) the correction after the sub-cycle(s); 5 u after the prolongation; 6 u after the up sweeps; 7 u of the
 *   coarsest level after its solve; 8 u of the collapsed level (the map applied); 9 u after one sweep of a leg
 *   (flags bits 8-9: 0 down / 1 up / 2 coarsest, bits 10 and up: the sweep's number, bit 6: the sweep took u as zero).
 * flags: 1 (step 3) the residual ran on the reduced operator with the F pass's product as a composite right-hand side;
 *   2 (step 0) the level's zero-fill was skipped; 4 / 8 (step 7) the dense solve / relaxation sweeps ran; 16 (steps 0, 8)
 *   the visit applied the collapsed map; 32 (step 0) the visit started from a zero guess. */
HYPRE_Int HYPRE_MI_BoomerAMGTraceCycle(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int nvec, HYPRE_Int collapse,
                                       const HYPRE_Real *f_host, const HYPRE_Real *u0_host, HYPRE_Int *nrecords);
HYPRE_Int HYPRE_MI_BoomerAMGGetTraceRecord(HYPRE_Solver solver, HYPRE_Int i, HYPRE_Int info[5], HYPRE_Real *values);
/* test hook: the state of a level the cycle's steps depend on.  out[0] = 1 when R's rows are stored in another order
 * and written through a row map, out[1] = t_from (the first F row whose product with the C values the F pass hands to
 * the residual), out[2] = 1 when the level has the reduced residual operator, out[3] = 1 when it has the zero-guess
 * sub-operator, out[4] = the number of C rows, out[5] = the level whose sub-cycle is collapsed (-1: none) */
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelCycleInfo(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int out[6]);
/* test hook: the tabulated map of the collapsed coarse tail.  *level = -1 and *n = 0 without one; else *n <= 1024 rows
 * and row j of Bt_host (n x n, row-major) is column j of the map f -> u.  Bt_host may be NULL to query the size */
HYPRE_Int HYPRE_MI_BoomerAMGGetCollapsedTail(HYPRE_Solver solver, HYPRE_Int *level, HYPRE_Int *n, HYPRE_Real *Bt_host);
/* which branch of the tile Gauss-Seidel kernel's in-chunk sweep the waves of one pass take, counted on the host from
 * the level's pattern (points 0: an all-point pass; +1 / -1: the C / F pass of a C-then-F pair; zero_guess: the first
 * sweep on a zero guess).  counts[5]: waves launched, waves without a selected row (no sweep), waves whose chunks
 * couple to nothing in-chunk but their diagonals (one update per row), zero-guess waves (short forward sweep), waves
 * on the general sweep.  *on_tiles = 0 (and all counts 0) when the pass does not run on the tile kernel. */
HYPRE_Int HYPRE_MI_BoomerAMGGetGSSweepPaths(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int points, HYPRE_Int zero_guess,
                                            HYPRE_Int *on_tiles, HYPRE_BigInt *counts);
/* FSAI smoother of a level (smooth_type 4, levels < smooth_num_levels): its G as CSR in GetLevelCSR's numbering (the
 * rows and columns of the level's diag block), and omega.  Size: 0 x 0 and nnz 0 when the level has none */
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelFSAISize(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int *nrows, HYPRE_BigInt *nnz);
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelFSAI(HYPRE_Solver solver, HYPRE_Int level, HYPRE_BigInt *ia, HYPRE_Int *ja,
                                         HYPRE_Complex *a, HYPRE_Real *omega);
/* how that G was built: the info[8] of HYPRE_MI_FSAIAdaptiveOp (static pattern: entries 2 ... 6 are 0) */
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelFSAIInfo(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int out[8]);
/* Chebyshev data of a level (relax type 16 in some slot at Setup): out[0 .. 5] = the estimated
 * smallest and largest eigenvalue of D^-1 A, the interval [lower, upper] the polynomial is built for, its centre theta
 * and half width delta.  An error when the level has none. */
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelCheby(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Real *out);
/* HYPRE_ILU with the iterative setup (types 1-4): sweeps run by the last Setup on this rank and
 * the last correction / residual norm (-1 when the option bits did not ask for it); the kept histories (option bit
 * 16; null arrays: the lengths only); the factors L (unit, strictly lower) and U as one CSR of the rank's diagonal
 * block (columns ascending) */
HYPRE_Int HYPRE_MI_ILUGetIterativeSetupInfo(HYPRE_Solver solver, HYPRE_Int *sweeps, HYPRE_Real *correction,
                                            HYPRE_Real *residual);
HYPRE_Int HYPRE_MI_ILUGetIterativeSetupHistory(HYPRE_Solver solver, HYPRE_Int *ncorr, HYPRE_Real *corr, HYPRE_Int *nres,
                                               HYPRE_Real *res);
HYPRE_Int HYPRE_MI_ILUGetFactorsSize(HYPRE_Solver solver, HYPRE_Int *nrows, HYPRE_BigInt *nnz);
HYPRE_Int HYPRE_MI_ILUGetFactors(HYPRE_Solver solver, HYPRE_BigInt *ia, HYPRE_Int *ja, HYPRE_Complex *a);
/* Multicolour ordering (HYPRE_ILUSetLocalReordering / HYPRE_BoomerAMGSetILULocalReordering value 2, this library's own
 * number): the block that is factorised is B = P D P^T, row q of B being the caller's local row
 * perm[q], rows sorted by (colour, local index).  With the ordering on, HYPRE_MI_ILUGetFactors returns the factors of
 * B, in B's numbering.  info[5]: the reordering in force (0 or 2), the number of colours, the colouring rounds, the
 * level sets of the lower and of the upper factor (0 when the setup built none).  perm, colour: n entries each, colour
 * by the caller's local row; either may be null, and neither is written when no ordering is in force. */
HYPRE_Int HYPRE_MI_ILUGetOrdering(HYPRE_Solver solver, HYPRE_Int info[5], HYPRE_Int *perm, HYPRE_Int *colour);
/* the same of the ILU smoother of a level (smooth_type 5), rows in GetLevelCSR's numbering; an error without one */
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelILUOrdering(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int info[5], HYPRE_Int *perm,
                                                HYPRE_Int *colour);
/* one complex-smoother step of a level on HOST arrays (the counterpart of RelaxLevel): u <- u + M (f - A u) with the
 * level's smoother M; zero_guess != 0 takes u = 0 on entry (the mat-vec is skipped, as on a cycle's down leg) */
HYPRE_Int HYPRE_MI_BoomerAMGSmoothLevel(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int zero_guess,
                                        const HYPRE_Real *f_host, HYPRE_Real *u_host);

/* ---- HIP-event timing of kernel classes on the library stream.
 * id: 0 level-0 SpMV of the Krylov loop, 1 level-0 relaxation, 2 dot, 3 axpy; per AMG level l < 16:
 * 4 + l residual SpMV of the cycle, 20 + l relaxation passes, 36 + l restriction, 52 + l prolongation */
HYPRE_Int HYPRE_MI_ProfileEnable(HYPRE_Int id, HYPRE_Int capacity);
HYPRE_Int HYPRE_MI_ProfileReset(void);
/* instantiation (template flags included, as rocprofv3's kernel statistics spell it) of the kernel last launched
 * under the class; empty when none was */
HYPRE_Int HYPRE_MI_ProfileKernelName(HYPRE_Int id, char *name, HYPRE_Int max_len);
HYPRE_Int HYPRE_MI_ProfileGet(HYPRE_Int id, long long *launches, double *total_ms, double *min_ms);
/* test hook, needs no device: the instantiation the library launches for an operator described by plain integers.
 * family 0: SpMV (epilogue 0; level0: under class 0) / masked Jacobi (epilogue 1) / the in-place colour pass of relax
 * types 40 - 42 (epilogue 3; 2, the Chebyshev step, has its own entry below); family 1: hybrid Gauss-Seidel with
 * `chunk` rows per chunk, where tiles != 0 says that the operator's tiles are whole 8-row chunks and the tile mode
 * (MI_HYPRE_GS_TILE) lets it use them.  xcache: the operator has the LDS x cache (mean row length >= 3); tile_entries
 * 2048 or 4096; has_fp32 / has_dictionary: the value arrays it holds (fp32 wins); nnz, nrows, rowlen_p95 (the entry
 * floor(0.95 (nrows - 1)) of the sorted row lengths): of its diagonal block */
HYPRE_Int HYPRE_MI_SolveKernelChoice(HYPRE_Int family, HYPRE_Int xcache, HYPRE_Int tile_entries, HYPRE_Int has_fp32,
                                     HYPRE_Int has_dictionary, HYPRE_Int epilogue, HYPRE_Int level0, HYPRE_Int chunk,
                                     HYPRE_Int tiles, HYPRE_BigInt nnz, HYPRE_Int nrows, HYPRE_Int rowlen_p95, char *name,
                                     HYPRE_Int max_len);
/* the same for a pass that serves nvec components of a multivector (1 ... 4): the batched instantiation and
 * *batched = 1 where the family has one (x-cache SpMV with epilogue 0, tile Gauss-Seidel), else the single-vector
 * instantiation, which the launcher then runs once per component, and *batched = 0.  nvec = 1 is SolveKernelChoice */
HYPRE_Int HYPRE_MI_SolveKernelChoiceMulti(HYPRE_Int nvec, HYPRE_Int family, HYPRE_Int xcache, HYPRE_Int tile_entries,
                                          HYPRE_Int has_fp32, HYPRE_Int has_dictionary, HYPRE_Int epilogue, HYPRE_Int level0,
                                          HYPRE_Int chunk, HYPRE_Int tiles, HYPRE_BigInt nnz, HYPRE_Int nrows,
                                          HYPRE_Int rowlen_p95, char *name, HYPRE_Int max_len, HYPRE_Int *batched);
/* the same for the Chebyshev step (relax type 16), the third epilogue of the SpMV family */
HYPRE_Int HYPRE_MI_ChebyKernelChoice(HYPRE_Int xcache, HYPRE_Int tile_entries, HYPRE_Int has_fp32, HYPRE_Int has_dictionary,
                                     char *name, HYPRE_Int max_len);

/* ---- synthetic problem: n^3-type Laplacian, true lexicographic global numbering
 * (7-point: diag 6 / off -1; 27-point: diag 26 / off -1 as
 * src/laplace_3d_weak_scaling.hpp:558,600; rhs = row sum, :321).  Fills COO
 * triples for global rows [ilower, iupper]; buffers come from malloc and are
 * released with HYPRE_MI_Free. */
HYPRE_Int HYPRE_MI_Laplace3D(HYPRE_Int nx, HYPRE_Int ny, HYPRE_Int nz, HYPRE_Int stencil, HYPRE_BigInt ilower,
                             HYPRE_BigInt iupper, HYPRE_BigInt *nnz, HYPRE_BigInt **rows, HYPRE_BigInt **cols,
                             HYPRE_Complex **vals, HYPRE_Complex **rhs);
void HYPRE_MI_Free(void *p);
/* the same arrays generated by a kernel into DEVICE memory (row offsets from a scan of the per-row counts); released
 * with HYPRE_MI_FreeDevice */
HYPRE_Int HYPRE_MI_Laplace3DDevice(HYPRE_Int nx, HYPRE_Int ny, HYPRE_Int nz, HYPRE_Int stencil, HYPRE_BigInt ilower,
                                   HYPRE_BigInt iupper, HYPRE_BigInt *nnz, HYPRE_BigInt **rows, HYPRE_BigInt **cols,
                                   HYPRE_Complex **vals, HYPRE_Complex **rhs);
void HYPRE_MI_FreeDevice(void *p);

#ifdef __cplusplus
}
#endif
#endif
