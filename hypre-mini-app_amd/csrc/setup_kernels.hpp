// Device kernels of the AMG setup phase (hypre_BoomerAMGSetup side of
// src/HypreSystem.cpp:692): sparse products of the Galerkin operator, transposes
// and the C-first renumbering.  Every kernel reproduces the host/oracle
// arithmetic bit for bit (same accumulation order, no fused multiply-add): this
// file is compiled with -ffp-contract=off.
#pragma once
#include "mi_internal.hpp"

namespace mi {
namespace sk {

// device CSR of the setup phase: 64-bit row pointers, columns ascending inside a row
struct DCsr {
  int nrows = 0, ncols = 0;
  int64_t nnz = 0;
  DVec<long long> ia;
  DVec<int> ja;
  DVec<double> a;
  void upload(const HostCSR &h, hipStream_t s);
  void download(HostCSR &h, hipStream_t s) const;
  void release() {
    ia.release();
    ja.release();
    a.release();
    nrows = ncols = 0;
    nnz = 0;
  }
};

// strength-of-connection graph of a single-rank operator (no halo block): row i keeps column j != i iff
// a_ij < theta * min_k a_ik (a_ii >= 0; mirrored for a_ii < 0); rows with |sum_j a_ij| > max_row_sum |a_ii|
// keep nothing.  S has no values (S.a stays empty).
void strength(const DCsr &A, double theta, double max_row_sum, DCsr &S, hipStream_t s);

// The same-function operator F(A) of a system with several unknowns (num_functions > 1; DESIGN.md section 3, "Systems
// of PDEs"): row i keeps the entries a_ij with dof[j] == dof[i] and its diagonal, in stored order -- bit for bit
// hs::filter_same_function.  A is square, dof has A.nrows entries (device).  A count pass, a scan and a fill pass, the
// lanes per row chosen by the mean row length like strength().
void same_function_filter(const DCsr &A, const int *dof, DCsr &F, hipStream_t s);
// out = v at the C points of cf (+1), in their order: the dof_func of the coarse level
void gather_at_c_points(const int *cf, const int *v, int n, DVec<int> &out, hipStream_t s);

// PMIS on the graph S: measure = |S^T row| + Park-Miller(seed) drawn in row order (hypre_Rand; element i is
// computed directly as seed * 16807^(i+1) mod 2^31-1).  cf: +1 C, -1 F, -3 F without strong connections.
void pmis(const DCsr &S, int seed, DVec<int> &cf, hipStream_t s);

// Interpolation (interp_type 6 extended+i or 0 classical modified) with truncation to pmax entries /
// trunc_factor, rows of A and S in ascending column order.  cf is updated like the host code does (-3 -> -1).
// Returns false -- and builds nothing -- when a row's interpolatory set may exceed the kernels' LDS capacity
// (the caller then runs the host routine for this level).  nc = number of C points.
// census (optional): which instantiation of the kernel took how many of the rows (C points and rows without an
// interpolatory set count with the smallest tables) -- numbers the routine has on the host anyway.
struct InterpCensus {
  int cap16 = 0, cap32 = 0;              // bound <= 16, <= 32
  int try32_kept = 0, try32_retried = 0; // bound 33 ... 128: finished in the 32-entry tables / rerun in the 128-entry ones
  int cap512 = 0, cap1024 = 0;           // bound 129 ... 512, 513 ... 1024
  int max_bound = 0;                     // the largest bound of the level
  bool fell_back = false;                // a row's bound exceeds 1024: nothing ran, the return value is false
};
bool interp(const DCsr &A, const DCsr &S, DVec<int> &cf, int interp_type, double trunc_factor, int pmax, DCsr &P,
            int &nc, hipStream_t s, InterpCensus *census = nullptr);

// Aggressive level (amg_setup.cpp coarsen_aggressive): cf holds the marker of the first coarsening on entry.  The
// second-generation graph on its C points (C point i depends on C point j != i iff j is in S_i or in S_k for some k in
// S_i; C numbering, ascending) is coarsened by PMIS with `seed` and the marker corrected: a C point the second
// coarsening rejected takes its second mark (-1 or -3).  Point for point the host's splitting.
void aggressive_second_stage(const DCsr &S, DVec<int> &cf, int seed, hipStream_t s);
// Two-stage extended interpolation (agg_interp_type 5): P = trunc(trunc12(E(A, S, m1)) *
// trunc12(C1 rows of E(A, S, m2))), the numerators by spgemm -- bit for bit hs::build_two_stage_ext.  m2 is updated
// like the host code does (-3 -> -1); nc = number of C points of m2.  Returns -1, or the first row whose denominator
// is zero while its numerator is not empty (P is then not built).
int two_stage_ext(const DCsr &A, const DCsr &S, const DVec<int> &m1, DVec<int> &m2, double p12_trunc_factor, int p12_max,
                  double trunc_factor, int pmax, DCsr &P, int &nc, hipStream_t s);

// Extended (interp_type 16) and extended+i (17) interpolation in matrix-matrix form: two operand
// builders, spgemm for the numerators, w = -n / d, truncation -- bit for bit hs::build_mm_interp; rows of any length.
// Type 16 is the stage operator E(A, S, cf) of the two-stage interpolation.  Type 17's left operand is built with
// `lanes` lanes per row (a power of two up to 64; 0 = by the mean row length): the result does not depend on it.
// cf is updated like the host code does (-3 -> -1); nc = number of C points.  Returns -1, or the first row whose
// denominator is zero while its numerator is not empty (cf then keeps its -3).
int mm_interp(const DCsr &A, const DCsr &S, DVec<int> &cf, int interp_type, double trunc_factor, int pmax, DCsr &P,
              int &nc, hipStream_t s, int lanes = 0);

// Distance-1 approximate ideal restriction (restriction 1; DESIGN.md section 3, "Approximate ideal restriction") of the
// square operator A with the final marker cf (+1 C, anything else F): row c(i) of R (|C| x n) holds (i, 1.0) and the
// solution y of A[N_i, N_i]^T y = -A[i, N_i]^T on the F-neighbourhood N_i (|a_ij| >= theta_r * max_{k != i} |a_ik|),
// less the entries the filter phi drops -- bit for bit hs::build_air_restriction.  A counting and a fill pass for the
// neighbourhoods, one small dense solve per row on 16 / 32 / 64 lanes by |N_i| (the elimination of fsai_local_solve),
// filter and compaction.  Returns 0; 1 when some |N_i| > 64 (R is not built: the caller runs the host routine; max_m
// is set); 2 when a local system is singular (bad_row = the first such row of A; R is not built).
struct AirInfo {
  int max_m = 0;                    // the largest |N_i|
  int zero_rows = 0;                // C rows with an empty N_i
  long long dropped = 0;            // entries the filter dropped
  int group_rows[3] = {0, 0, 0};    // rows solved by the 16-, 32- and 64-lane instantiation (the device routine only)
  int bad_row = -1;
};
int air_restriction(const DCsr &A, const int *cf, double theta_r, double phi, DCsr &R, AirInfo &info, hipStream_t s);
// One-point interpolation (interp_type 100): a C point i gets (c(i), 1.0), an F point the C point
// of its row of S with the largest |a_ij| (the lowest column on a tie), or an empty row -- one row per lane, rows of any
// length, bit for bit hs::build_one_point_interp.  cf is updated like the host code does (-3 -> -1); nc = number of C points.
void one_point_interp(const DCsr &A, const DCsr &S, DVec<int> &cf, DCsr &P, int &nc, hipStream_t s);

// C = A * B.  Rows of B must have ascending columns.  Entry (i, j) is the sum of
// a_ik * b_kj taken in the stored order of A's row i (first product assigned,
// the others added one by one) -- exactly host_spgemm (amg_setup.cpp) and the
// oracle's ocsr_matmul; output columns ascending.
void spgemm(const DCsr &A, const DCsr &B, DCsr &C, hipStream_t s);

// Non-Galerkin sparsification of a square operator (amg_setup.cpp sparsify_non_galerkin, the oracle's function of the
// same name): with m_i = max_{j != i} |a_ij|, off-diagonal entries with |a_ij| < tol * min(m_i, m_j) are dropped and
// added to the row's diagonal in stored order.  In place (A is replaced).
// N > 1 (a rank's rows in an extended column space, diagonal of row i in column i + row0): `maxima` holds m for EVERY
// column -- the own rows' from non_galerkin_row_maxima, the remote ones fetched from their owners by the caller.
void sparsify_non_galerkin(DCsr &A, double tol, hipStream_t s, int row0 = 0, const double *maxima = nullptr);
// m[row0 + i] = max_{j != row0 + i} |a_ij| for the rows of A
void non_galerkin_row_maxima(const DCsr &A, int row0, double *m, hipStream_t s);

// out[0..n] = exclusive scan of the counts in[0..n) with 64-bit sums (out[n] = the total); complete on return
void exclusive_scan_counts(const int *in, long long *out, long long n, hipStream_t s);

// T = A^T with ascending columns in every row (entries of one output row keep
// the order of A's rows)
void transpose(const DCsr &A, DCsr &T, hipStream_t s);

// B = rows of A taken in `perm` order (perm[new] = old; null = identity) with
// columns mapped through colpos (null = identity) and re-sorted ascending
void permute(const DCsr &A, const int *perm, const int *colpos, DCsr &B, hipStream_t s);

// B = the nout rows rows[0..nout) of A (any subset, any order) with columns mapped through colpos (null =
// identity) and re-sorted ascending -- this rank's slice of a global level in the replicated multi-rank setup
void extract_rows(const DCsr &A, const int *rows, int nout, const int *colpos, DCsr &B, hipStream_t s);

// Solve-phase format of a setup-phase matrix, built on the device: 32-bit row pointers, the row-block
// schedule and x cache of the SpMV (DevCSR::upload builds the same from host arrays).  src's column and
// value arrays are MOVED into dst; only the row pointers travel to the host (for the greedy block schedule).
void to_solve_format(DCsr &src, DevCSR &dst, hipStream_t s);
// its tile schedule alone (k::build_row_blocks on the device, one thread per super-block, k::tile_end_bisect): rb on the
// device, blocks on the host, aligned = all tiles start on a multiple of 8 rows and were cut at whole chunks
void tile_schedule_device(int n, const long long *ia, int row_cap, int tile_entries, DVec<int> &rb, std::vector<int> &blocks,
                          bool &aligned, hipStream_t s);
// the host buffer to_solve_format keeps between calls goes back to the system (end of a setup)
void release_host_scratch();
// launches an empty kernel of this translation unit: its device code is loaded now (HYPRE_Init) instead of at the first setup
void load_device_code(hipStream_t s);
// The part of a C-first ordered square block (C points = indices < nc) that a FIRST relaxation sweep on a
// zero guess can touch: every row keeps the entries inside its own chunk of `chunk` rows, F rows also their C
// columns (written by the C pass that precedes the F pass).  Everything else multiplies zeros.  Columns stay
// ascending; Z goes through to_solve_format like any operator.
// mode 1: the operator of the residual that follows that sweep -- F rows from the first chunk boundary >= nc on
// lose their C columns (the F pass hands over f - A_FC u_C for them), every other row stays whole.
void zero_guess_operator(const DevCSR &A, int nc, int chunk, DCsr &Z, hipStream_t s, int mode = 0);
// C-row hand-over: which tiles of a C-first ordered operator in the tile format (C points =
// indices < nc) the mat-vec that follows a level-0 C pass may leave out.  A C row is FLAGGED when it has an off-diagonal
// C column; a tile is HANDED OVER when all its rows are C rows (r1 <= nc) and none is flagged -- the C pass then holds
// (A z)_i of every row of it.  mv_tdesc: the descriptors of the other tiles, in their order.
struct HandoverCensus {
  int tiles = 0, listed = 0, handed = 0;  // tiles of the operator = listed + handed
  long long flagged_c_rows = 0;
  int w_upto = 0;  // end of the last handed-over tile: no row from here on is handed over
};
void handover_tiles(const DevCSR &A, int nc, DVec<int> &mv_tdesc, HandoverCensus &census, hipStream_t s);
// setup-phase copy (64-bit row pointers) of an operator that lives in the solve format (device-to-device)
void from_solve_format(const DevCSR &src, DCsr &dst, hipStream_t s);
// Rounds of the internal locality numbering (amg_setup.cpp locality_order: graph Voronoi cells) on the device:
// labels start as the seeds' ranks (seeds ascending), -2 for excluded rows, -1 elsewhere; in every round an
// unlabelled row takes the smallest label among its neighbours of the same segment (row >> segshift) labelled in the
// previous round.  Stops when a round
// changes nothing or after max_rounds; label_host gets the result (-1 = never reached).  Returns the rounds run.
int locality_labels(const DCsr &A, const int *seeds_host, int nseeds, const unsigned char *exclude_host, int segshift,
                    int max_rounds, std::vector<int> &label_host, hipStream_t s);
// The whole internal numbering on the device (one rank, no excluded rows): order[new] = old, exactly hs::locality_order's
// result.  false (nothing usable in `order`) when more than a handful of cells outgrow the in-LDS sort.
bool locality_order_device(const DCsr &A, int segshift, int cluster, int max_rounds, DVec<int> &order, int &nseeds,
                           int &rounds, hipStream_t s);
// out[i] = (signed char)in[i]
void ints_to_i8(const int *in, long long n, signed char *out, hipStream_t s);
// pos[order[q]] = q
void invert_permutation(const int *order, int n, int *pos, hipStream_t s);
// back to host arrays (lazy host copies for the inspection API)
void solve_format_to_host(const DevCSR &src, HostCSR &h, hipStream_t s);

// diagonal, l1 norm of the hybrid-GS chunks (option 4, C/F aware) and full l1 norm per row (level_norms in
// amg_setup.cpp) of a single-rank operator; cf may be null
// halo (optional, N > 1): the level's halo block with full-length row pointers and the C/F type of its columns --
// its entries follow the diag block's in every sum, like hs::level_norms
void level_norms(const DCsr &A, const int *cf, int chunk, double *diag, double *l1gs, double *l1jac, hipStream_t s,
                 const DCsr *halo = nullptr, const int *cf_ext = nullptr);

// ---- setup reuse ("Setup reuse"): new values on the stored patterns of a finished hierarchy
// a CSR somebody else owns: 64-bit row pointers, columns ascending in every row
struct CsrRef {
  int nrows, ncols;
  int64_t nnz;
  const long long *ia;
  const int *ja;
  const double *a;
};
CsrRef ref_of(const DCsr &A);
// spgemm and level_norms on such views (the solve format's own arrays; the DCsr forms call these)
void spgemm(const CsrRef &A, const CsrRef &B, DCsr &C, hipStream_t s);
void level_norms(const CsrRef &A, const int *cf, int chunk, double *diag, double *l1gs, double *l1jac, hipStream_t s,
                 const DCsr *halo, const int *cf_ext);
// Numeric-only Galerkin product: the stored entries (i, j) of C take sum_k r_ik T_kj, k ascending along R's row, with
// T = spgemm(A, P) -- the bits of host_spgemm(R, host_spgemm(A, P)).  Stored row r of R is row r_rowmap[r] of C (null:
// r).  Two stages: spgemm for T, then one owner lane per stored entry of C that finds its column in the rows T_k by
// binary search (`lanes` per row: 0 = by the mean row length; rows of any length).  Returns -1 and writes c_a, or the
// first row of C whose stored pattern is not the product's -- then c_a is untouched.  seconds (optional): the stages.
int galerkin_values(const CsrRef &A, const CsrRef &P, const CsrRef &R, const int *r_rowmap, const CsrRef &C, double *c_a,
                    int lanes, hipStream_t s, double *seconds = nullptr);
int galerkin_values(const DevCSR &A, const DevCSR &P, const DevCSR &R, DevCSR &C, hipStream_t s, double *seconds = nullptr);
// dst_a[entry (r, c) of dst] = src[rowmap[r], colmap[c]] by binary search in src's row (null maps: identity).  Returns
// -1, or the first row of dst with an entry src does not store -- found by a pass that only looks, so nothing is written
int value_lookup(const CsrRef &dst, double *dst_a, const int *rowmap, const int *colmap, const CsrRef &src, hipStream_t s);
int value_lookup(DevCSR &dst, const int *rowmap, const int *colmap, const DevCSR &src, hipStream_t s);
// level_norms of an operator in the solve format (one rank)
void level_norms(const DevCSR &A, const int *cf, int chunk, double *diag, double *l1gs, double *l1jac, hipStream_t s);

// ---- multicolour ordering of the ILU (local_reordering 2): the first-fit greedy colouring of the
// graph of D + D^T (diagonal excluded) taken in the order of the rows' hashed priorities, found by Jones-Plassmann
// rounds -- one launch and one small download (the rows still uncoloured) per round, no waiting inside a launch.
// colour: n entries on return; rounds: launches run.  Returns 0, or -1 when n rounds left rows uncoloured (which a
// correct run cannot do: the caller fails).
int ilu_multicolour(const DCsr &D, DVec<int> &colour, int &rounds, hipStream_t s);
// ---- multicolour Gauss-Seidel (relax types 40-42)
// the smallest row of the square block D that stores no diagonal entry (kind 0) or stores a_ii == 0 (kind 1); -1: none
long long mcgs_bad_diagonal(const DCsr &D, int &kind, hipStream_t s);
// The stable sort of the rows by (block, colour), block 0 = rows below nc, block 1 = the others: order[new] = row.  One
// flagged scan per colour (twice: counts, then places), so the order inside a (block, colour) range is ascending.
// range_start: the ranges' first rows and n at the end; range_colour: their colours; ranges_c: how many lie below nc.
void mcgs_order(const int *colour, int n, int nc, DVec<int> &order, std::vector<int> &range_start,
                std::vector<int> &range_colour, int &ncolours, int &ranges_c, hipStream_t s);
// out[perm[q]] = in[q]
void ilu_unpermute(const int *perm, const double *in, double *out, int n, hipStream_t s);

// ---- ILU(0) of a single-rank block (HYPRE_ILU type 0, fill 0), level-scheduled
// position of the diagonal entry of every row (-1: none)
void ilu_diag_positions(const DCsr &A, long long *dpos, hipStream_t s);
// Everything below needs a stored diagonal in every row (dpos[i] >= 0): the caller refuses a pattern without one.
// The smallest row whose pivot u_ii is exactly zero, or -1 (one small download)
long long ilu_zero_pivot(const DCsr &LU, const long long *dpos, hipStream_t s);
// in-place IKJ factorisation of the rows rows[0..nrows) -- one level set: every row they depend on is final
void ilu_factor_level(DCsr &LU, const long long *dpos, const int *rows, int nrows, hipStream_t s);
// forward / backward substitution for one level set: y[i] = b[i] - sum_{k<i} l_ik y_k ;
// x[i] = (y[i] - sum_{j>i} u_ij x_j) / u_ii
// perm (nullable, here and in ilu_lower_jacobi): the lower substitution reads b[perm[i]] for row i -- the gather of a
// right-hand side in the caller's numbering when LU holds the factors of the reordered block P D P^T
void ilu_lower_level(const DCsr &LU, const long long *dpos, const int *rows, int nrows, const int *perm, const double *b,
                     double *y, hipStream_t s);
void ilu_upper_level(const DCsr &LU, const long long *dpos, const int *rows, int nrows, const double *y, double *x,
                     hipStream_t s);
// Jacobi sweeps on the triangular factors (HYPRE's iterative triangular solve):
// out = b - L_strict in   /   out = D^-1 (b - U_strict in) ; in == nullptr: out = b resp. D^-1 b
void ilu_lower_jacobi(const DCsr &LU, const long long *dpos, const int *perm, const double *b, const double *in,
                      double *out, hipStream_t s);
void ilu_upper_jacobi(const DCsr &LU, const long long *dpos, const double *b, const double *in, double *out, hipStream_t s);

// ---- iterative ILU(0) setup (ilu.cpp; DESIGN.md section 3, "Iterative ILU(0) setup"): fixed-point sweeps on the
// pattern S of LU.  Every stored entry (i,j) owns a value slot; the split layout (types 2-4) puts the L entries in CSR
// order first and the U entries after them by (column, row), the in-place layout (type 1) is LU's own order.  The
// pairs ((i,k), (k,j)) in S of every entry, k < min(i,j) ascending, are found once; a sweep gathers over them:
//   s = a_ij; s -= l_ik * u_kj (ascending k); l_ij = s / u_jj (i > j) or u_ij = s (i <= j)
// Slot and pair indices are 32-bit (the caller refuses nnz > INT_MAX).
// stat[4] (device, unsigned 64-bit): [0] max|x_m - x_(m-1)|, [1] max|x_m|, [2] max|a - LU| on S (or max|a|, itilu_abs_max)
// -- bit patterns of non-negative doubles, atomic maxima (exact in any order) -- and [3] the smallest row whose pivot
// u_jj was zero (all ones: none).  The caller zeroes [0..2] and fills [3] with ones.
struct ItiluPlan {
  long long nnz = 0, npairs = 0;
  DVec<int> perm;        // slot -> position in LU (empty: the identity)
  DVec<double> a;        // a_ij by slot
  DVec<int> dslot;       // L entry: slot of u_jj; off-diagonal U entry: -1; diagonal of row i: -(i + 2)
  DVec<long long> ptr;   // pairs of slot t: [ptr[t], ptr[t + 1])
  DVec<int> pl, pu;      // slots of l_ik and u_kj
};
// builds the plan; returns -1, or the first row without a stored diagonal (then nothing is built)
int itilu_plan(const DCsr &LU, const long long *dpos, bool split, ItiluPlan &P, hipStream_t s);
// x_0: L = strictly lower part of A with column j divided by a_jj, U = upper part of A (zero a_jj -> stat[3])
void itilu_start(const ItiluPlan &P, double *x, unsigned long long *stat, hipStream_t s);
// synchronous sweep xn = F(xo); fused_norm: the same launch also reduces stat[0], stat[1]
void itilu_sweep(const ItiluPlan &P, const double *xo, double *xn, bool fused_norm, unsigned long long *stat,
                 hipStream_t s);
// stat[0], stat[1] of a synchronous sweep
void itilu_correction(const ItiluPlan &P, const double *xo, const double *xn, unsigned long long *stat, hipStream_t s);
// asynchronous sweep in place (relaxed agent-scope loads and stores); norm: stat[0], stat[1] against the value replaced
void itilu_async_sweep(const ItiluPlan &P, double *x, bool norm, unsigned long long *stat, hipStream_t s);
// stat[2] = max over S of |a_ij - (L U)_ij|
void itilu_residual(const ItiluPlan &P, const double *x, unsigned long long *stat, hipStream_t s);
// stat[0] = max |a_ij|
void itilu_abs_max(const ItiluPlan &P, unsigned long long *stat, hipStream_t s);
// LU.a[perm[t]] = x[t]
void itilu_scatter(const ItiluPlan &P, const double *x, DCsr &LU, hipStream_t s);

// ---- FSAI with a static pattern (fsai.cpp), on a rank's diagonal block B (columns ascending in every row)
// S = B's pattern, values 1.0: filter -- (i,i) (inserted when B does not store it) and every (i,j) with
// |b_ij| >= theta * max_{l != i} |b_il|; no filter -- every entry; lower -- only the entries j <= i
void fsai_select(const DCsr &B, double theta, bool filter, bool lower, DCsr &S, hipStream_t s);
// G on the pattern P (rows ascending, the diagonal last): g_i = y / sqrt(y_last) with B[P_i, P_i]^T y = e_last by
// Gaussian elimination with partial pivoting, one row per 16 / 32 / 64 lanes by |P_i|.  max_row = largest |P_i|.
// Returns 0; 1 when max_row > 64 (G is not built); 2 when a row fails (bad_row = the first, bad_kind 1 singular,
// 2 y_last <= 0)
int fsai_local_solve(const DCsr &B, const DCsr &P, DCsr &G, int &max_row, int &bad_row, int &bad_kind, hipStream_t s);
// v[i] = element gid0 + i of the global Park-Miller stream seeded with `seed` (the PMIS measures' stream) / (2^31 - 1)
void fsai_random_vector(int n, long long gid0, int seed, double *v, hipStream_t s);

// ---- FSAI with the adaptive pattern (fsai_algo_type 4; DESIGN.md section 3, "FSAI (adaptive pattern)"), on a rank's
// diagonal block B (columns ascending in every row): every row grows its pattern from the Kaporin gradient in up to
// max_steps steps of up to max_step_size columns (max_steps * max_step_size + 1 <= 64), one row per 16 / 32 / 64 lanes
// by that bound, without leaving the kernel -- bit for bit hs::build_fsai_adaptive.  The candidate table of a row has
// table_slots slots in LDS (a power of two; 0 or above fsai_adaptive_lds_slots: that many); the rows whose candidates
// do not fit are computed again by the same code with the table in global memory.  Rows are written padded to the bound
// and compacted, fsai_adaptive_batch_rows rows at a time.  Returns 0, or 2 when a row fails (info.bad_row = the first,
// info.bad_kind 1 singular, 2 y_last <= 0; G is not built).
struct FsaiAdaptiveInfo {
  int status = 0;                                                   // 0 built, 2 a row failed
  int max_row = 0, max_candidates = 0;                              // the largest row of G / candidate count at a step
  int overflow_rows = 0;                                            // rows that took the global-memory table (device only)
  int stop_tolerance = 0, stop_no_candidate = 0, stop_max_steps = 0;  // rows by the reason they stopped growing
  int bad_row = -1, bad_kind = 0;
};
int fsai_adaptive(const DCsr &B, int max_steps, int max_step_size, double kap_tolerance, int table_slots, DCsr &G,
                  FsaiAdaptiveInfo &info, hipStream_t s);
int fsai_adaptive_lds_slots(int bound);         // LDS table slots per row for a row bound (16 x the lane-group size)
long long fsai_adaptive_batch_rows(int bound);  // rows per batch: 256 MiB of padded rows (MI_HYPRE_FSAI_BATCH_ROWS overrides)

// ---- distributed setup on the device (amg_setup_dist.cpp: BoomerAMG::build_distributed_device)
// Column map between two extended index spaces [remote below | own range | remote above] (ascending global ids):
// column c of the source becomes below[c] (c < nb_old), own_tab[c - nb_old] or own_new0 + (c - nb_old) (own range,
// n_own columns), above[c - nb_old - n_own] (the rest); a missing table, keep_own == false or a negative table value
// drops the entry.  Tables are device arrays.
struct ExtColMap {
  int nb_old = 0, n_own = 0;
  bool keep_own = true;
  int own_new0 = 0;
  const int *own_tab = nullptr;
  const int *below = nullptr;
  const int *above = nullptr;
};
// B = rows rows[0..nout) of A (rows == null: row0, row0 + 1, ...) with the columns mapped (entries keep their stored
// order; sort = true re-sorts every row by the new column)
void select_rows(const DCsr &A, const int *rows, int row0, int nout, const ExtColMap &m, int new_ncols, bool sort,
                 DCsr &B, hipStream_t s);
// the same change of column space in place, for maps that drop nothing and keep the order (checked)
void remap_columns(DCsr &A, const ExtColMap &m, int new_ncols, hipStream_t s);
// C = the parts' rows one block after the other (same column space)
void vconcat(const DCsr *const *parts, int nparts, DCsr &C, hipStream_t s);
// C = [A | B]: row i = A's entries, then B's with columns shifted by A.ncols
void hstack(const DCsr &A, const DCsr &B, DCsr &C, hipStream_t s);
// PMIS on the rows [row0, row0 + n) of an extended strength graph S; cnt / measure / cf / tmp span S.ncols entries,
// the caller exchanges their remote parts between the steps (hs distributed PMIS, amg_setup_dist.cpp)
void pmis_dist_counts(const DCsr &S, int row0, int n, int *cnt, hipStream_t s);  // cnt[col] += 1 per strong entry
int pmis_dist_init(const DCsr &S, int row0, int n, long long gid0, int seed, const int *cnt, double *measure, int *cf,
                   int *counter, hipStream_t s);  // returns the undecided own rows
void pmis_dist_compare(const DCsr &S, int row0, int n, int ne, const int *cf, const double *measure, signed char *tmp,
                       hipStream_t s);  // tmp = 1 everywhere, then 0 for the losers of this round's comparisons
void pmis_dist_select(int row0, int n, int *cf, const signed char *tmp, hipStream_t s);
int pmis_dist_fpoints(const DCsr &S, int row0, int n, int *cf, int *counter, hipStream_t s);  // returns undecided
// dst[k] = src[idx[k] + shift] for elements of 1, 4 or 8 bytes; dst[idx[k] + shift] += v[k]; dst[idx[k] + shift] = 0 where v[k] == 0
void gather_elems(const void *src, const int *idx, int shift, int n, int elem_bytes, void *dst, hipStream_t s);
void scatter_add_int(int *dst, const int *idx, int shift, const int *v, int n, hipStream_t s);
void scatter_zero_flags(signed char *dst, const int *idx, int shift, const signed char *v, int n, hipStream_t s);
// rank[i] = number of C points before entry i of cf[0..n) (rank[n] = their count, returned)
long long count_c_points(const int *cf, int n, DVec<long long> &rank, hipStream_t s);
// cg[i] = first + rank[i] for C points, -1 otherwise
void fill_coarse_ids(const int *cf, const long long *rank, int n, long long first, long long *cg, hipStream_t s);
// C-first order of n rows: pos[i] = new position of row i (C points first, both groups in their old order), perm = its inverse
void cfirst_order(const int *cf, const long long *crank, int n, int nc, int *pos, int *perm, hipStream_t s);
// rows of P with at least one column outside [c0, c1), ascending, on the host
int rows_with_columns_outside(const DCsr &P, int c0, int c1, std::vector<int> &rows_host, hipStream_t s);
// used[c] = 1 for every column that occurs in A
void mark_used_columns(const DCsr &A, DVec<unsigned char> &used, hipStream_t s);
void add_to_ints(int *v, int n, int add, hipStream_t s);

}  // namespace sk
}  // namespace mi
