// Launchers of the hand-written gfx950 kernels (kernels.hip).  All launches are
// asynchronous on the given stream; pointers are device pointers.
#pragma once
#include "mi_internal.hpp"

namespace mi {
namespace k {

constexpr int SPMV_BLOCK = 256;   // threads per workgroup (4 wave64)
constexpr int SPMV_TILE = 2048;   // LDS-staged products per workgroup
// Operators with long rows (coarse Galerkin levels with 100-150 entries per row) get tiles of twice the entries,
// run by twice the threads (same work per thread, 32 / 40 KB of LDS = still 32 waves per CU): an 8-row chunk of such
// rows holds 800-1500 entries, so 2048-entry tiles close after one or two chunks, 2/3 full, and share few columns.
// 512^3: level 3 / 4 / 5 relaxation 1.35 / 0.47 / 0.126 -> 1.23 / 0.42 / 0.103 ms; a level with 77 entries per row
// LOSES 6 % (its 2048-entry tiles are 90 % full already), hence the threshold
constexpr int SPMV_BLOCK_WIDE = 512;
constexpr int SPMV_TILE_WIDE = 4096;
constexpr int RED_MAX_BLOCKS = 2048;
constexpr int MASS_NV = 8;        // vectors per pass of the block inner product / block update
// basis vectors per block of the blocked modified Gram-Schmidt of single-rank GMRES (mgs_block_pass); -DMI_MGS_NB=4 / 16
// build the other sizes that profiles/gmres_blocked_mgs.txt compares
#ifndef MI_MGS_NB
#define MI_MGS_NB MASS_NV
#endif
constexpr int MGS_NB = MI_MGS_NB;
constexpr int GS_BLOCK = 256;     // chunks (lanes) per workgroup
constexpr int GS_MAX_CHUNK = 32;

// kernel classes that can be timed with HIP events (profile.cpp)
// 0..3: the classes bench.py times; then per AMG level l < PROF_LEVELS: the residual SpMV of the cycle, the
// relaxation passes, restriction and prolongation (profiles/roofline_table.py)
constexpr int PROF_LEVELS = 16;
enum ProfId {
  PROF_NONE = -1,
  PROF_SPMV_L0 = 0,
  PROF_RELAX_L0 = 1,
  PROF_DOT = 2,
  PROF_AXPY = 3,
  PROF_LVL_RESID = 4,
  PROF_LVL_RELAX = PROF_LVL_RESID + PROF_LEVELS,
  PROF_LVL_RESTRICT = PROF_LVL_RELAX + PROF_LEVELS,
  PROF_LVL_PROLONG = PROF_LVL_RESTRICT + PROF_LEVELS,
  PROF_LVL_RELAX0 = PROF_LVL_PROLONG + PROF_LEVELS,  // first sweep on a zero guess (runs on the sub-operator)
  PROF_LVL_RELAX_MC = PROF_LVL_RELAX0 + PROF_LEVELS,  // colour passes of relax types 40 / 41 / 42 (one launch per range)
  PROF_COUNT = PROF_LVL_RELAX_MC + PROF_LEVELS
};
inline int prof_level(int base, int level) { return level < PROF_LEVELS ? base + level : PROF_NONE; }

// Row-block (tile) schedule of the SpMV / tile Gauss-Seidel kernels: <= row_cap rows and < tile_entries entries per
// tile, or exactly one longer row; greedy, whole 8-row chunks while they fit.  Round 4: tiles never cross a multiple of
// TILE_SUPER_ROWS rows, so the schedule of every such super-block is independent of the others -- the device builds it
// with one thread per super-block (sk::to_solve_format) instead of the host walking the row pointers of the whole
// operator (1 GB of them per operator at 512^3, copied over PCIe first); the price is one underfull tile per 8192 rows.
// tile_end(): one step of the schedule, shared by the host routine and the device kernel.
constexpr int TILE_SUPER_ROWS = 8192;
// (ia: anything indexable by a row that yields its first entry -- the row pointers themselves, or the device kernel's
// staged copy of a super-block's chunk boundaries)
template <class IA>
__host__ __device__ inline int tile_end(int r, int limit, const IA &ia, int row_cap, int block_rows, int tile_entries,
                                        bool &aligned) {
  const long long start = (long long)ia[r];
  int e = r;
  if ((r & 7) == 0 && row_cap <= block_rows) {  // whole chunks while they fit (SpMV-only operators: any row)
    while (e < limit && e - r < row_cap) {
      const int e2 = (e + 8 < limit) ? e + 8 : limit;
      if ((long long)ia[e2] - start > tile_entries - 1) break;
      e = e2;
    }
  }
  if (e == r) {  // not even one chunk fits (or an unaligned start after such a chunk): row granularity
    aligned = false;
    // keep one slot of slack for the aligned-pair start
    while (e < limit && e - r < row_cap && (long long)ia[e + 1] - start <= tile_entries - 1) e++;
    if (e == r) e = r + 1;  // a single row longer than the tile
  }
  return e;
}
// The same step by bisection (the device schedule, sk::to_solve_format): the entry counts ascend with the row, so "as many
// whole chunks / rows as fit" is the last candidate end whose count fits -- ~10 dependent reads per tile instead of one
// per chunk or per row (SpMV-only operators are scheduled row by row: 8192 dependent reads per super-block, 8 ms per
// launch at 512^3).  tests/test_gpu_kernels.py compares the two on random row lengths (HYPRE_MI_TileScheduleCheck).
template <class IA>
__host__ __device__ inline int tile_end_bisect(int r, int limit, const IA &ia, int row_cap, int block_rows, int tile_entries,
                                               bool &aligned) {
  const long long start = (long long)ia[r];
  const long long room = (long long)tile_entries - 1;
  int e = r;
  if ((r & 7) == 0 && row_cap <= block_rows) {
    // candidate ends e_m = min(r + 8 m, limit), m = 1 .. M (the iterations the loop above can make)
    const int by_cap = (row_cap + 7) / 8, by_rows = (limit - r + 7) / 8;
    const int M = by_cap < by_rows ? by_cap : by_rows;
    int lo = 0, hi = M;  // the answer m lies in [lo, hi]; m = 0: not even one chunk
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      const int em = (r + 8 * mid < limit) ? r + 8 * mid : limit;
      if ((long long)ia[em] - start <= room)
        lo = mid;
      else
        hi = mid - 1;
    }
    if (lo > 0) e = (r + 8 * lo < limit) ? r + 8 * lo : limit;
  }
  if (e == r) {
    aligned = false;
    const int top = ((long long)r + row_cap < (long long)limit) ? r + row_cap : limit;
    int lo = r, hi = top;  // the last e in [r, top] with ia[e] - start <= room (e = r always qualifies)
    while (lo < hi) {
      const int mid = (int)(((long long)lo + hi + 1) >> 1);
      if ((long long)ia[mid] - start <= room)
        lo = mid;
      else
        hi = mid - 1;
    }
    e = lo;
    if (e == r) e = r + 1;
  }
  return e;
}
std::vector<int> build_row_blocks(int nrows, const int64_t *ia, bool *chunk_aligned = nullptr,
                                  int row_cap = SPMV_BLOCK, int tile_entries = SPMV_TILE);
// tile size of an operator with nnz entries in nrows rows (MI_HYPRE_WIDE_TILE_MIN_ROWLEN, default 100 entries per row; 0 = never wide)
int choose_tile_entries(int64_t nnz, int nrows);
constexpr int SPMV_ONLY_ROW_CAP = 4 * SPMV_BLOCK;  // rows per tile of operators no Gauss-Seidel kernel sweeps
constexpr int XC_ID_MASK = 0xFFF;   // block-local column id inside an lcol entry (at most SPMV_TILE_WIDE = 4096 ids)
constexpr int XC_INCH = 0x8000;     // the column lies in the row's own 8-row chunk ...
constexpr int XC_OFF_SHIFT = 12;    // ... at this offset (3 bits)

// per-tile descriptors of the SpMV / tile-GS kernels (row range, entry range, column-list range: 8 ints per
// tile); call after rb, ia and (x cache) uptr are in place
// ia64: the operator's 64-bit row pointers (device; the descriptors carry full 64-bit tile bases)
void build_tile_desc(DevCSR &A, const long long *ia64, hipStream_t s);
// value dictionary of an operator with at most 256 distinct values (called by build_tile_desc)
void build_value_dictionary(DevCSR &A, hipStream_t s);
// MI_HYPRE_VALUE_DICT / HYPRE_MI_SetValueDictionary: applies to operators put into the solve format afterwards
bool value_dictionary_enabled();
void set_value_dictionary(bool on);
// ---- fp32 value storage (HYPRE_MI_BoomerAMGSetValueStorage; the rule is DESIGN.md section 3)
// whether the value may be stored as a float: zero, Inf and NaN pass (they convert exactly); a finite non-zero value
// needs FLT_MIN <= |v| <= FLT_MAX, so that (double)(float)v is neither a subnormal, zero nor infinity
__host__ __device__ inline bool fits_float(double v) {
  const double m = v < 0.0 ? -v : v;
  if (!(m <= 1.79769313486231570814527423731704357e+308)) return true;  // Inf, NaN
  return m == 0.0 || (m >= 1.17549435082228750796873653722224568e-38 && m <= 3.40282346638528859811704183484516925e+38);
}
// device arrays: whether all n values fit (synchronises s); a[k] = (double)(float)a[k]
bool values_fit_float(const double *a, long long n, hipStream_t s);
void round_values(double *a, long long n, hipStream_t s);
// an operator in the solve format whose values fit: mode 1 moves them into A.a32 (A.a is released), mode 2 rounds A.a
// in place; an operator with a value dictionary keeps it in either mode, with the table and A.a rounded.  Sets A.value_kind.
void narrow_values(DevCSR &A, int mode, hipStream_t s);
// the operator's values as doubles: A.a, or A.a32 widened into tmp (setup paths that read a placed operator again)
const double *fp64_values(const DevCSR &A, DVec<double> &tmp, hipStream_t s);
// device bytes of the operator's value arrays (values, dictionary indices and table), padding included
long long value_stream_bytes(const DevCSR &A);
// ---- which instantiation of the solve kernels runs: decided here and nowhere else.  Pure host code that reads no
// device memory (HYPRE_MI_SolveKernelChoice hands it plain integers; tests/test_kernel_choice_spec.py holds the table).
struct SolveKernelDesc {
  bool xcache = false;
  int tile_entries = SPMV_TILE;
  ValueFormat format = ValueFormat::FP64;
  int epi = 0;          // SpMV family: 0 mat-vec, 1 masked Jacobi, 2 Chebyshev step, 3 in-place colour pass
  bool level0 = false;  // SpMV family: launched under the profiler's level-0 class
  // hybrid Gauss-Seidel family
  int chunk = 8;
  bool tiles = false;  // the tiles are whole 8-row chunks (DevCSR::gs_tiles) and MI_HYPRE_GS_TILE lets the operator use them
  int64_t nnz = 0;
  int nrows = 0;
  int rowlen_p95 = 0;
  // components of a multivector the launch serves (spmv_multi / gs_hybrid_multi): 2 .. 4 select the batched
  // instantiation where the family has one
  int nvec = 1;
};
enum class KernelFamily { STREAM, STREAM_XC, GS_TILE, GS_GROUP, GS_DENSE, GS_HYBRID };
struct KernelChoice {
  const void *kernel;  // instantiations of one family share a signature (apart from the value pointer of the float ones)
  const char *name;    // the instantiation as rocprofv3's kernel statistics spell it
  KernelFamily family;
  int block;  // threads per workgroup
  int lpc;    // GS_GROUP / GS_DENSE: lanes per chunk
  // nvec > 1: whether `kernel` is the batched instantiation for nvec components (other signature: MvStrides /
  // GsMvStrides after the scalars); false: the single-vector kernel, which the launcher runs once per component
  bool batched = false;
};
KernelChoice choose_stream_kernel(const SolveKernelDesc &d);
KernelChoice choose_gs_kernel(const SolveKernelDesc &d);

// y = alpha*A*x + beta*b   (b may alias y)
// b_lo (optional): rows < b_split take their b entry from b_lo instead of b
void spmv(const DevCSR &A, const double *x, double alpha, double beta, const double *b, double *y, hipStream_t s,
          int prof = PROF_NONE, const double *b_lo = nullptr, int b_split = 0);
// ---- multivectors: the same operations on the nvec components of component-major vectors, each
// vector with its own stride between components (in doubles).  At most multivector_batch() (and never more than
// MV_MAX_BATCH) components share one pass over the operator, in order (5 = 4 + 1); where the chosen family has no batched
// instantiation, or the width is 1, the single-vector kernel runs once per component.  Either way every component
// gets the bits of the single-vector call on it.
constexpr int GS_NO_ZEROS = 0x7fffffff;  // gs_hybrid's zero_from: no column is known to hold zero
constexpr int MV_MAX_BATCH = 4;
constexpr int MV_BATCH_DEFAULT = 1;  // opt-in: see README (round notes) for why
int multivector_batch();             // MI_HYPRE_MV_BATCH / HYPRE_MI_SetMultivectorBatch: 1 .. MV_MAX_BATCH
void set_multivector_batch(int width);
// returns the number of passes when the batched kernels ran (a trailing single component counts as a pass), else 0
int spmv_multi(const DevCSR &A, int nvec, const double *x, long long x_stride, double alpha, double beta, const double *b,
               long long b_stride, double *y, long long y_stride, hipStream_t s, int prof = PROF_NONE,
               const double *b_lo = nullptr, long long b_lo_stride = 0, int b_split = 0);
struct GsMultiStrides {
  long long u_lo, u_hi, out, f, offc, tout;
};
int gs_hybrid_multi(const DevCSR &A, int nvec, const GsMultiStrides &st, const double *u_lo, const double *u_hi, int split,
                    double *out, const double *f, const double *offc, const double *d, const signed char *cf, int points,
                    int chunk, bool fwd, bool bwd, double w, int row_begin, int row_end, hipStream_t s,
                    int prof = PROF_NONE, int zero_from = GS_NO_ZEROS, double *tout = nullptr, int t_from = 0);
// y[rows[k]] += alpha * (B*xext)[k]
void spmv_offd_add(const DevOffd &B, const double *xext, double alpha, double *y, hipStream_t s);
// out[rows[k]] = (B*xext)[k]   (other entries of out untouched)
void spmv_offd_set(const DevOffd &B, const double *xext, double *out, hipStream_t s);

// masked Jacobi family: u_new = u_old + w*(f - offc - A*u_old)/d on selected rows, copy elsewhere
void jacobi(const DevCSR &A, const double *u_old, double *u_new, const double *f, const double *offc, const double *d,
            const signed char *cf, int points, double w, hipStream_t s, int prof = PROF_NONE);
// Chebyshev step (relax type 16) in the stream SpMV's epilogue, one pass over A:
//   dc_i = a*dc_i + b*((f_i - (A u_old)_i - offc_i) / diag_i)   (a == 0: step 0, dc is not read),   u_new_i = u_old_i + dc_i
// dc is updated in place (row i's finishing lane alone touches dc_i); u_new must not alias u_old
void cheby_step(const DevCSR &A, const double *u_old, double *u_new, double *dc, const double *f, const double *offc,
                const double *diag, double a, double b, hipStream_t s, int prof = PROF_NONE);
// One colour pass of the multicolour Gauss-Seidel (relax types 40-42), the Jacobi family's data
// path in place:   u_i += w*(f_i - offc_i - (A u)_i) / d_i   for the rows i of [row_begin, row_end), u read as it
// stands.  The caller guarantees that no row of the range stores a column of the range but its own (the rows have one
// colour of a colouring of D + D^T); only the tiles that intersect the range are launched, and the rows of a tile
// outside the range are left alone.
void inplace_pass(const DevCSR &A, double *u, const double *f, const double *offc, const double *d, double w,
                  int row_begin, int row_end, hipStream_t s, int prof = PROF_NONE);
// step 0 on a zero guess, no matrix pass: dc_i = b0*(f_i / diag_i), u_i = dc_i -- the bits cheby_step gives from u_old = 0
void cheby_first(const double *f, const double *diag, double b0, double *dc, double *u, int n, hipStream_t s);
// out = 1 / sqrt(x);  out = x .* y (out may alias either)
void inv_sqrt(const double *x, double *out, int n, hipStream_t s);
void vec_mul(const double *x, const double *y, double *out, int n, hipStream_t s);
// this rank's Gershgorin bound of D^-1 A: max_i sum_j |a_ij| / diag_i over the diag block A and the halo block B, and
// the number of rows whose diag_i is not positive (they take no part in the maximum); work: n doubles; synchronises s
void gershgorin(const DevCSR &A, const DevOffd &B, const double *diag, double *work, double *lambda_max,
                long long *bad_diagonals, hipStream_t s);
// hybrid Gauss-Seidel family: chunks of `chunk` consecutive rows are swept
// sequentially (forward and/or backward), chunks see each other's pre-sweep
// values.  Only the chunks that intersect [row_begin, row_end) are swept (a C or
// an F pass of a C-first ordered level).  Pre-sweep values are read from u_lo
// for rows < split and from u_hi for rows >= split (the second pass of a C/F
// pair reads the first pass's output without a copy); the swept chunks' rows are
// written to out.  zero_from: the caller guarantees that every pre-sweep value with index >= zero_from is
// zero (first sweep on a zero guess); kernels may then skip those gathers -- same result, less traffic.
// whether gs_hybrid sweeps A tile by tile (A.rb_host boundaries) rather than chunk by chunk: a caller that
// splits one pass into several launches must cut at the unit the kernel writes back
bool gs_uses_tiles(const DevCSR &A, int chunk);
// whether a sweep with zero_from == 0 leaves the pre-sweep vector unread (its zero-fill can then be skipped)
bool gs_ignores_zero_vector(const DevCSR &A, int chunk);
void gs_hybrid(const DevCSR &A, const double *u_lo, const double *u_hi, int split, double *out, const double *f,
               const double *offc, const double *d, const signed char *cf, int points, int chunk, bool fwd, bool bwd,
               double w, int row_begin, int row_end, hipStream_t s, int prof = PROF_NONE, int zero_from = GS_NO_ZEROS,
               double *tout = nullptr, int t_from = 0, double *wout = nullptr);
// tout (tile kernel only -- check gs_uses_tiles): every swept row i >= t_from also stores f[i] minus its
// out-of-chunk sum there
// wout (tile kernel only): every swept row of a wave whose chunks couple to nothing in-chunk but their own diagonals
// also stores its out-of-chunk sum plus a_ii times its new value there -- (A u)_i for a row whose out-of-chunk
// columns the pass does not update (C-row hand-over); other rows of wout are left alone
// y = A x on the tiles tdesc[0 .. nb) alone (descriptors copied from A.tdesc; x-cache tile format only): the rows of
// the other tiles are not written
void spmv_listed_tiles(const DevCSR &A, const int *tdesc, int nb, const double *x, double *y, hipStream_t s,
                       int prof = PROF_NONE);
// which branches of the tile kernel's sweep phase the waves of such a pass take, counted on the host (kernels.hip)
bool gs_tile_path_census(const DevCSR &A, int chunk, const int64_t *ia, const int *ja, const int *cf, int points,
                         int row_begin, int row_end, int zero_from, long long counts[5]);

// BLAS-1
void dot(const double *x, const double *y, int n, double *out_dev, hipStream_t s);  // local sum, no collective
// fused MGS step: y += scale*(*alpha_dev)*xa, then out_dev = <xd, y> (xd == nullptr: <y, y>), local sum
void axpy_dot(const double *alpha_dev, double scale, const double *xa, double *y, const double *xd, int n,
              double *out_dev, hipStream_t s);
// one pass of the blocked MGS step over w: h_out[j] = the MGS coefficients of the m_prev
// vectors `prev` by forward substitution from their raw inner products c_prev[j] = <prev_j, w> and raw Gram rows
// gram_prev (row j: MGS_NB + 1 doubles, <prev_k, w_j> for k < j, then ||w_j||^2, w_j = prev_j before its scaling);
// w -= sum_j h_j prev_j; then out_dev[0 .. MGS_NB] = <next_j, w> for j < m_next (raw c of the next block), or, in the
// last pass of a step, <prev_j, w> for j < m_prev and ||w||^2 at [MGS_NB] and at out_norm: the raw Gram row of w.
// Entries beyond the counts are 0.  One launch; local sums in a fixed order
void mgs_block_pass(const double *const *prev, int m_prev, const double *const *next, int m_next, bool last,
                    const double *c_prev, const double *gram_prev, double *h_out, double *w, int n, double *out_dev,
                    double *out_norm, hipStream_t s);
// Krylov basis storage mode 1: the same kernels instantiated on basis vectors stored as float --
// mgs_block_pass, mass_dot, mass_axpy and lin_comb below take `const float *const *` too.  w, the sums and every output
// stay double; elements map to lanes and sums run as in the double instantiation, so a float call gives the bits of the
// double call on the same (float-representable) values.
void mgs_block_pass(const float *const *prev, int m_prev, const float *const *next, int m_next, bool last,
                    const double *c_prev, const double *gram_prev, double *h_out, double *w, int n, double *out_dev,
                    double *out_norm, hipStream_t s);
void mass_dot(const float *const *vecs, int m, const double *w, int n, double *out_dev, hipStream_t s);
void mass_axpy(const float *const *vecs, int m, const double *coef_dev, double scale, double *w, int n, hipStream_t s);
void lin_comb(const float *const *vecs, const double *coef_host, int m, bool init, double *w, int n, hipStream_t s);
// block Gram-Schmidt (COGMRES): out_dev[j] = <vecs[j], w> for j < m (local sums), and w += scale * sum_j coef_dev[j] vecs[j]
void mass_dot(const double *const *vecs, int m, const double *w, int n, double *out_dev, hipStream_t s);
void mass_axpy(const double *const *vecs, int m, const double *coef_dev, double scale, double *w, int n, hipStream_t s);
// w = coef[0] vecs[0] (init) or w += coef[0] vecs[0]; then w += coef[j] vecs[j], j = 1 .. m-1 in this order (host
// coefficients); MASS_NV vectors per pass
void lin_comb(const double *const *vecs, const double *coef_host, int m, bool init, double *w, int n, hipStream_t s);
void axpy(double alpha, const double *x, double *y, int n, hipStream_t s);
void axpy_dev(const double *alpha_dev, double scale, const double *x, double *y, int n, hipStream_t s);
void scale(double alpha, double *x, int n, hipStream_t s);
// scale_inv_sqrt_dev + the `count` doubles at `slots` and then `seq` posted into host memory (see scale_post_k)
void scale_inv_sqrt_post(const double *sumsq_dev, double *x, int n, const double *slots, int count, double *host_out,
                         unsigned long long *host_flag, unsigned long long seq, hipStream_t s);
void scale_inv_sqrt_dev(const double *sumsq_dev, double *x, int n, hipStream_t s);
// the three scalings with the rounding of basis storage modes 1 and 2: x_i = rd(x_i * a), rd(v) = (double)(float)v (the
// product first, then the rounding); slot (mode 1; NULL in mode 2) also receives (float)(x_i * a).  Posting as above.
void scale_round(double alpha, double *x, float *slot, int n, hipStream_t s);
void scale_inv_sqrt_post_round(const double *sumsq_dev, double *x, float *slot, int n, const double *slots, int count,
                               double *host_out, unsigned long long *host_flag, unsigned long long seq, hipStream_t s);
void scale_inv_sqrt_dev_round(const double *sumsq_dev, double *x, float *slot, int n, hipStream_t s);
void load_device_code(hipStream_t s);
void fill(double *x, int n, double v, hipStream_t s);
void copy(const double *x, double *y, int n, hipStream_t s);
void gather(const double *x, const int *map, double *out, int n, hipStream_t s);
// out[i] = (map[i] < split ? lo : hi)[map[i]]
void gather2(const double *lo, const double *hi, int split, const int *map, double *out, int n, hipStream_t s);
// two-stage Gauss-Seidel pieces (relax types 11 / 12): z = r / d, u += z;  zout = (L zin) / d, u += sign * zout
void two_stage_first(const double *r, const double *d, double *z, double *u, int n, hipStream_t s);
void two_stage_lower(const DevCSR &A, const double *d, const double *zin, double sign, double *zout, double *u,
                     hipStream_t s);
// u = M f, M dense n x m row-major
void dense_matvec(const double *M, const double *f, double *u, int n, int m, hipStream_t s);
// u = sum_j f[j] * Mt[j][:], Mt n x n row-major (row j = column j of the map); fixed summation order
void dense_matvec_t(const double *Mt, const double *f, double *u, int n, hipStream_t s);

// ---- peer-store neighbour exchange (comm.cpp IpcExchangeComm): one launch moves every message of a halo update.
// A SEND copies local data into the mailbox slot the peer holds for this rank (an IPC-mapped pointer: stores over
// xGMI) and then publishes the message's sequence number in the peer's flag word; a RECV waits for its flag word,
// copies its own mailbox slot to the destination and acknowledges in the peer's ack word, which is what the
// sender's NEXT use of that slot waits for.  Every wait is bounded (spin_limit ticks of the 100 MHz wall clock):
// a peer that never arrives sets *error_flag instead of hanging the GPU.
struct IpcTransfer {
  int kind;                      // 0 send, 1 recv
  int nblocks;                   // workgroups that share the copy
  unsigned long long bytes;
  const void *src;               // send: local data; recv: my mailbox slot
  void *dst;                     // send: the peer's mailbox slot; recv: local destination
  unsigned long long *wait_word; // send: my ack word for this slot (peer wrote it); recv: my flag word
  unsigned long long wait_value; // proceed when *wait_word >= wait_value
  unsigned long long *post_word; // send: the peer's flag word; recv: the peer's ack word
  unsigned long long post_value;
  unsigned *ticket;              // per-transfer counter of finished workgroups (self-resetting)
};
constexpr int IPC_MAX_TRANSFERS = 32;
struct IpcBatch {
  IpcTransfer t[IPC_MAX_TRANSFERS];
  int n;
};
void ipc_exchange(const IpcBatch &b, unsigned long long spin_limit, int *error_flag, hipStream_t s);
// Peer-store all-reduce (sum) of up to IPC_AR_MAX doubles: every rank stores its values into every peer's mailbox
// (slot [parity][rank]) and publishes the reduction's number; then it waits for all peers' numbers and adds the
// size contributions IN RANK ORDER -- the same order on every rank, so all ranks get the same bits.  Two parities:
// nobody can start reduction k + 2 before every rank has finished reduction k (it needs their k + 1 values first).
constexpr int IPC_AR_MAX = 8;
struct IpcAllreduce {
  int rank, size, count;
  unsigned long long seq;            // number of this reduction (1, 2, ...)
  double *buf;                       // in: this rank's values; out: the sums
  double *my_slots;                  // my arena: [2][size][IPC_AR_MAX]
  unsigned long long *my_flags;      // my arena: [2][size]
  double *peer_slots[16];            // every rank's slots / flags as mapped here (self: my own)
  unsigned long long *peer_flags[16];
};
void ipc_allreduce(const IpcAllreduce &a, unsigned long long spin_limit, int *error_flag, hipStream_t s);
// buf[0..count) = NaN when the transport's error flag is up (reductions that travel on the wrapped communicator)
void ipc_poison(double *buf, int count, const int *error_flag, hipStream_t s);

// IJ helpers
void scatter_set(double *x, const int *idx, const double *vals, int n, hipStream_t s);
// column-by-column tabulation inside a captured graph (see tab_unit_k / tab_store_k)
void bytes_differ(const unsigned char *p, size_t n, unsigned char tag, unsigned long long *out3, hipStream_t s);
void fill_bytes(unsigned char *p, size_t n, unsigned char tag, hipStream_t s);
void tab_unit(double *e, const int *col, hipStream_t s);
void tab_store(double *Bt, const double *u, int n, int *col, hipStream_t s);
void scatter_add(double *x, const int *idx, const double *vals, int n, hipStream_t s);

}  // namespace k
}  // namespace mi
