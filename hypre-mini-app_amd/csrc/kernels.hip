// Hand-written HIP kernels for gfx950 (MI355X, wave64, 256 CUs in 8 XCDs).
//
// Everything on this path is HBM-bandwidth bound sparse/vector work (arithmetic
// intensity ~0.13 flop/B): no MFMA.  The rules that matter are coalesced 16-byte
// streaming loads of the matrix, LDS staging of the per-entry products so that
// short rows reduce without divergence, __shfl wave reductions, and a
// workgroup->row-range map that keeps each XCD's L2 on its own slice of x.
#include <algorithm>

#include "kernels.hpp"

#include <cstring>
#include <limits>
#include "profile.hpp"

namespace mi {
namespace k {

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8 share an
// L2).  Remap so that XCD g walks the contiguous row-block range
// [g*chunk, (g+1)*chunk): neighbouring rows (and the x planes they gather) stay
// in one L2.  Speed only -- any placement gives the same result.
// Streams that are read exactly once per kernel in whole cache lines per load instruction (matrix values
// and column ids of the row-block SpMV) use non-temporal loads so that they do not evict the gathered
// vector from L2.  (Not in the GS kernel: its per-row segments share lines between load instructions, and
// non-temporal lines are not kept in L1 -- measured 35 % slower.)
typedef double d2_t __attribute__((ext_vector_type(2)));
typedef float f2_t __attribute__((ext_vector_type(2)));
typedef int i2_t __attribute__((ext_vector_type(2)));
typedef unsigned short us2_t __attribute__((ext_vector_type(2)));
typedef unsigned char uc2_t __attribute__((ext_vector_type(2)));
template <class T>
__device__ __forceinline__ T nt_load(const T *p) {
  return __builtin_nontemporal_load(p);
}
// Two consecutive elements of a Krylov basis vector stored as T = double or float (basis storage mode 1, DESIGN.md
// section 3), as the doubles the arithmetic takes: one 16-byte or one 8-byte load per lane, the same elements on the same
// lane either way, and float -> double is exact -- a kernel instantiated on float gives the bits its double instantiation
// gives on the same values.  NT: non-temporal, where the fp64 kernel's load is.
template <class T>
struct BasisPair;
template <>
struct BasisPair<double> {
  typedef d2_t type;
};
template <>
struct BasisPair<float> {
  typedef f2_t type;
};
template <bool NT, class T>
__device__ __forceinline__ d2_t load_pair(const T *p) {
  typedef typename BasisPair<T>::type V;
  const V v = NT ? nt_load(reinterpret_cast<const V *>(p)) : *reinterpret_cast<const V *>(p);
  d2_t r;
  r.x = (double)v.x;
  r.y = (double)v.y;
  return r;
}

// The tile kernels (spmv_stream_xc, gs_tile_k) read their matrix stream (values or value indices, 16-bit column words)
// and their column lists exactly once, in whole lines per load instruction: non-temporal loads too, so that what stays
// in L2 is the gathered vector, which neighbouring tiles share.  A/B at 512^3 on one box (profiles/r03_ab_stream_nt.txt):
// stream alone -0.6 % per solve, with the lists -1 %, level-0 SpMV 2.77 -> 2.73 ms; same bits.  -DMI_STREAM_NT=0 /
// -DMI_LIST_NT=0 build the plain loads.  (Also tried, no effect either way: non-temporal loads of the per-row vectors
// f / d / b, non-temporal stores of the swept vector.)
#if !defined(MI_STREAM_NT) || MI_STREAM_NT
#define STREAM_LOAD(p) nt_load(p)
#else
#define STREAM_LOAD(p) (*(p))
#endif
#if !defined(MI_LIST_NT) || MI_LIST_NT
#define LIST_LOAD(p) nt_load(p)
#else
#define LIST_LOAD(p) (*(p))
#endif

// Timing ablations of the tile kernels (profiles/debug/ablate_table.py; results are WRONG with any bit set, never in a
// shipped build): -DMI_ABLATE=<bits>  1: every gather reads one of x's first 64 entries (the list is still loaded)
// 2: no column-list load  4: no matrix-stream loads  8: no LDS product phase / row sums (SpMV), no 8x8 sweep (GS)
#ifndef MI_ABLATE
#define MI_ABLATE 0
#endif

__device__ __forceinline__ int xcd_remap(int bid, int chunk) { return (bid & 7) * chunk + (bid >> 3); }

// ---------------------------------------------------------------------------
// LDS-staged row-block SpMV ("CSR-stream") with fused epilogues.
//   phase 1: the workgroup streams its contiguous slice of (col,val) with
//            16-byte/8-byte coalesced loads, gathers x, writes products to LDS
//   phase 2: G lanes per row (G = 1..64, uniform per workgroup) sum the row's
//            products out of LDS; G > 1 finishes with __shfl_down
// A block that holds exactly one row longer than the tile takes the
// whole-workgroup path instead.
// EPI 0: y = alpha*s + beta*b          (matvec / residual / restrict / prolong)
// EPI 1: masked Jacobi  y = x_i + w*(f - offc - s)/d on selected rows, else x_i
// EPI 2: Chebyshev step dc_i = ca*dc_i + cb*((f - s - offc)/d), y = x_i + dc_i  (relax type 16)
// EPI 3: in-place pass over the rows [row_begin, row_end) of one colour (relax types 40-42):
//        u_i += w*(f - offc - s)/d.  The vector is gathered and written through EpiArgs::u alone -- the kernels'
//        x and y, which promise not to alias, are not used -- and only the tiles from blk0 on are launched; a tile that
//        straddles an end of the range computes all its rows and writes those inside.  The rows of the range do not
//        couple (colouring of D + D^T), so no workgroup gathers an entry another one writes for a row it keeps.
// ---------------------------------------------------------------------------
struct EpiArgs {
  double alpha, beta;      // EPI 0
  const double *b;         // EPI 0: b ; EPI 1: f
  const double *offc;      // EPI 1 (nullable)
  const double *d;         // EPI 1
  const signed char *cf;   // EPI 1 (nullable)
  int points;              // EPI 1
  const int *rowmap;       // EPI 0 (nullable): stored row r is row rowmap[r] of y and b (DevCSR::rowmap)
  const double *b_lo;      // EPI 0 (nullable): rows < b_split take their b entry from here (a composite right-hand
  int b_split;             //   side: BoomerAMG's residual after a zero-guess sweep, f for the C rows, f - A_FC u_C after)
  double *dc;              // EPI 2: the Chebyshev direction vector, updated in place (b = f, offc, d as for EPI 1)
  double ca, cb;           // EPI 2: the step's coefficients (ca == 0: step 0, dc is not read)
  double *u;               // EPI 3: the vector, read and written in place (b = f, offc, d, alpha = w as for EPI 1)
  int row_begin, row_end;  // EPI 3: the rows that are written
  int blk0;                // EPI 3: the first tile of the launch
};
__device__ __forceinline__ double epi_b(const EpiArgs &e, int ro) { return ((e.b_lo && ro < e.b_split) ? e.b_lo : e.b)[ro]; }

template <int EPI>
__device__ __forceinline__ void epilogue(int r, double s, const double *__restrict__ x, double *__restrict__ y,
                                         const EpiArgs &e) {
  if (EPI == 3) {
    if (r < e.row_begin || r >= e.row_end) return;
    double res = e.b[r] - s;
    if (e.offc) res -= e.offc[r];
    e.u[r] = e.u[r] + e.alpha * res / e.d[r];
  } else if (EPI == 0) {
    // y is written once and next read by another kernel: keep it out of L2's way
    const int ro = e.rowmap ? e.rowmap[r] : r;
    __builtin_nontemporal_store((e.beta == 0.0) ? e.alpha * s : e.alpha * s + e.beta * epi_b(e, ro), y + ro);
  } else if (EPI == 2) {
    // the specification's order of operations, without contraction: the restatement in the tests rounds the same way
#pragma clang fp contract(off)
    const double xi = x[r];
    double res = e.b[r] - s;
    if (e.offc) res -= e.offc[r];
    double dn = e.cb * (res / e.d[r]);
    if (e.ca != 0.0) dn = e.ca * e.dc[r] + dn;  // only row r's finishing lane touches dc[r]
    e.dc[r] = dn;
    y[r] = xi + dn;
  } else {
    const double xi = x[r];
    double out = xi;
    const bool sel = (e.points == 0) || (e.cf == nullptr) || (e.cf[r] == e.points);
    const double d = e.d[r];
    if (sel && d != 0.0) {
      double res = e.b[r] - s;
      if (e.offc) res -= e.offc[r];
      out = xi + e.alpha * res / d;
    }
    y[r] = out;
  }
}

// TAG only names the instantiation: TAG 1 = the level-0 operator, so that the
// rocprofv3 kernel statistics carry a row for exactly the launches bench.py times
// VT: the type of the stored values (double, or float for an operator with fp32 value storage -- DevCSR::a32; the
// value is widened where the product is formed, everything after it is the same arithmetic)
template <int EPI, int TAG, class VT = double>
__global__ __launch_bounds__(SPMV_BLOCK) void spmv_stream(int nb, int xchunk, const int *__restrict__ rb,
                                                          const int *__restrict__ ia, const int *__restrict__ ja,
                                                          const VT *__restrict__ av, const double *__restrict__ x,
                                                          double *__restrict__ y, EpiArgs e) {
  __shared__ double prod[SPMV_TILE];
  int blk = xcd_remap(blockIdx.x, xchunk);
  if (blk >= nb) return;
  if (EPI == 3) blk += e.blk0;  // nb tiles from e.blk0 on
  // the gathered vector: x, or (EPI 3) the in-place vector, a pointer that carries no promise about aliasing
  const double *xg = (EPI == 3) ? e.u : x;
  const int tid = threadIdx.x;
  const int r0 = rb[blk], r1 = rb[blk + 1];
  const int base = ia[r0], end = ia[r1];
  if (end - base >= SPMV_TILE) {
    // one long row: every lane strides over it, two-level reduction
    double s = 0.0;
    for (int k = base + tid; k < end; k += SPMV_BLOCK) s += (double)av[k] * xg[ja[k]];
    s = wave_sum(s);
    if ((tid & 63) == 0) prod[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) epilogue<EPI>(r0, prod[0] + prod[1] + prod[2] + prod[3], x, y, e);
    return;
  }
  // phase 1: aligned pairs -> double2 / int2 loads (arrays carry 2 pad entries)
  const int base_al = base & ~1;
  const int cnt = end - base_al;  // <= SPMV_TILE
  for (int k = 2 * tid; k < cnt; k += 2 * SPMV_BLOCK) {
    typedef VT v2_t __attribute__((ext_vector_type(2)));
    const v2_t v = nt_load(reinterpret_cast<const v2_t *>(av + base_al + k));
    const i2_t c = nt_load(reinterpret_cast<const i2_t *>(ja + base_al + k));
    const bool ok0 = (base_al + k >= base);
    const bool ok1 = (base_al + k + 1 < end);
    const double x0 = ok0 ? xg[c.x] : 0.0;
    const double x1 = ok1 ? xg[c.y] : 0.0;
    prod[k] = (double)v.x * x0;
    if (k + 1 < SPMV_TILE) prod[k + 1] = (double)v.y * x1;
  }
  __syncthreads();
  // phase 2
  const int nr = r1 - r0;
  int G = 1;
  while (G < 64 && nr * G * 2 <= SPMV_BLOCK) G <<= 1;
  const int lane = tid & (G - 1);
  for (int rr = tid / G; rr < nr; rr += SPMV_BLOCK / G) {
    const int r = r0 + rr;
    const int s0 = ia[r] - base_al, s1 = ia[r + 1] - base_al;
    double s = 0.0;
    for (int k = s0 + lane; k < s1; k += G) s += prod[k];
    for (int off = G >> 1; off > 0; off >>= 1) s += __shfl_down(s, off, G);
    if (lane == 0) epilogue<EPI>(r, s, x, y, e);
  }
}

// Same kernel with an LDS x cache, for levels with long rows (coarse AMG levels).
// There the plain version spends ~45 % of its time on the x gathers: 64
// consecutive entries hit 30-60 different lines, neighbouring rows re-request
// the same lines a moment later, and with 32 waves per CU the 32 KB L1 cannot
// hold them, so every lane becomes an L2 transaction.  Here each workgroup first
// gathers the sorted unique columns of its row block ONCE into LDS (adjacent
// lanes -> ascending addresses, well coalesced) and the entries then carry
// 16-bit block-local ids (which also shrinks the index stream from 4 to 2 B).
//
// Load order: the waves of this kernel wait ~84 % of their cycles with ~7 tiles resident per CU, i.e. a tile
// lives ~12 us, most of it in dependent round trips.  Vector-memory results are counted in issue order, so
// waiting for a LATE-issued short load also waits for every stream load issued before it.  The tile's row
// range, entry range and column-list range therefore arrive in one 32-byte (scalar) descriptor load, the
// column list is requested FIRST (its gathers are the longest chain), then the matrix stream and the row
// pointers of the row sums; the x gathers start as soon as the column ids are back, while the stream is still
// in flight.  (Worth ~0.5 % of the 512^3 solve over the rb -> ia -> stream / uptr -> ucols -> x order: the
// kernel is not bound by this chain alone -- VALU, LDS and the L1 gather path are each 25-30 % busy.)
// VAL8: the operator has a value dictionary (DevCSR::vidx / vlut): the stream is one byte per value, looked up in
// a 2 KB LDS copy of the table
// VAL4: the operator stores fp32 values (DevCSR::a32, handed in through `av`): the stream is 4 bytes per value, loaded
// in pairs and widened to double where the product is formed; products, the product buffer and the row sums are the
// fp64 ones of the plain stream.  (A trailing parameter, so that the instantiations that existed before it keep the
// leading part of their names in the profiler's statistics.)
template <int EPI, int TAG, bool VAL8, int BLOCK, bool VAL4 = false>
__global__ __launch_bounds__(BLOCK) void spmv_stream_xc(int nb, int xchunk, const int *__restrict__ tdesc,
                                                             const int *__restrict__ ia, const int *__restrict__ ja,
                                                             const double *__restrict__ av,
                                                             const int *__restrict__ ucols,
                                                             const unsigned short *__restrict__ lcol,
                                                             const double *__restrict__ x, double *__restrict__ y,
                                                             EpiArgs e, const unsigned char *__restrict__ vidx,
                                                             const double *__restrict__ vlut) {
  static_assert(!(VAL8 && VAL4), "one value format per instantiation");
  constexpr int TILE = 8 * BLOCK;  // TILE / TILE_WIDE
  __shared__ double prod[TILE];
  __shared__ double slut[VAL8 ? 256 : 1];
  double *xs = prod;
  int blk = xcd_remap(blockIdx.x, xchunk);
  if (blk >= nb) return;
  if (EPI == 3) blk += e.blk0;  // nb tiles from e.blk0 on
  // the gathered vector: x, or (EPI 3) the in-place vector, a pointer that carries no promise about aliasing
  const double *xg = (EPI == 3) ? e.u : x;
  const int tid = threadIdx.x;
  if (MI_ABLATE & 128) {  // launch only
    if (tid == 0 && blk == nb + 1) y[0] = 0.0;
    return;
  }
  // (the table entry waits in a register until the LDS writes before the first barrier: stored here, the kernel began
  // with a load, a wait and a write before anything else was requested)
  double lutv = 0.0;
  if (VAL8 && tid < 256) lutv = vlut[tid];
  const int4 d0 = reinterpret_cast<const int4 *>(tdesc)[2 * blk];
  const int4 d1 = reinterpret_cast<const int4 *>(tdesc)[2 * blk + 1];
  const int r0 = d0.x, r1 = d0.y, len = d0.w, u0 = d1.x, nu = d1.y;
  if (MI_ABLATE & 64) {  // launch + descriptor
    if (tid == 0 && r0 + len + u0 + nu + d1.z == -12345) y[0] = lutv;
    return;
  }
  // the tile's entry range starts at a 64-bit offset (operators beyond 2^31 entries); everything below is tile-local
  const long long base64 = ((long long)d1.z << 32) | (long long)(unsigned)d0.z;
  if (len >= TILE) {
    double s = 0.0;
    if (VAL4) {
      const float *av4 = reinterpret_cast<const float *>(av);
      for (long long k = base64 + tid; k < base64 + len; k += BLOCK) s += (double)av4[k] * xg[ja[k]];
    } else {
      for (long long k = base64 + tid; k < base64 + len; k += BLOCK) s += av[k] * xg[ja[k]];
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) prod[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
      double tot = prod[0] + prod[1] + prod[2] + prod[3];
      for (int wv = 4; wv < BLOCK / 64; wv++) tot += prod[wv];
      epilogue<EPI>(r0, tot, x, y, e);
    }
    return;
  }
  constexpr int NU = TILE / BLOCK;
  int uc[NU];
#pragma unroll
  for (int q = 0; q < NU; q++) {
    const int k = tid + q * BLOCK;
    // (nothing that needs the loaded id inside the branch: written as a select, the compiler put the id's 64-bit
    // extension there and with it a wait after every load -- up to eight SERIAL round trips per tile; check the ISA
    // when this line changes: no s_waitcnt between the list loads)
    uc[q] = 0;
    if (!(MI_ABLATE & 2) && k < nu) uc[q] = LIST_LOAD(ucols + u0 + k);
  }
  const long long base_al64 = base64 & ~1LL;
  const int base = (int)(base64 - base_al64), base_al = 0;  // tile-local: the aligned start is 0, the first entry 0 or 1
  const int end = base + len;
  const int cnt = end;
  const unsigned ia_off = (unsigned)base_al64;  // low word: (unsigned)ia[row] - ia_off = the row's tile-local offset
  const float *av4 = reinterpret_cast<const float *>(av) + base_al64;  // VAL4: the same argument, 4-byte entries
  av += base_al64;
  lcol += base_al64;
  if (VAL8) vidx += base_al64;
  constexpr int NIT = TILE / (2 * BLOCK);
  d2_t vv[NIT];
  f2_t vf[NIT];  // VAL4: two values, as loaded (widened after the first barrier)
  unsigned cw[NIT];  // two 16-bit column words, as loaded
  unsigned vw[NIT];  // two value indices, as loaded, one register each (nothing is unpacked or packed inside the
                     // branches: that makes the compiler wait for each load where it stands)
#pragma unroll
  for (int it = 0; it < NIT; it++) {
    const int k = 2 * tid + it * 2 * BLOCK;
    cw[it] = 0;
    vw[it] = 0;
    if (MI_ABLATE & 4) vv[it] = d2_t{1.0, 1.0}, vf[it] = f2_t{1.0f, 1.0f};
    if (!(MI_ABLATE & 4) && k < cnt) {
      if (VAL8)
        vw[it] = STREAM_LOAD(reinterpret_cast<const unsigned short *>(vidx + base_al + k));
      else if (VAL4)
        vf[it] = STREAM_LOAD(reinterpret_cast<const f2_t *>(av4 + base_al + k));
      else
        vv[it] = STREAM_LOAD(reinterpret_cast<const d2_t *>(av + base_al + k));
      cw[it] = STREAM_LOAD(reinterpret_cast<const unsigned *>(lcol + base_al + k));
    }
  }
  // the gathers: ALL of them in flight before the first LDS write, and before the loads below that depend on each other.
  // (Written as `if (k < nu) xs[k] = x[uc[q]]`, every load sat in a branch of its own with its wait and its LDS write:
  // up to eight serial round trips per tile.  Lanes beyond the list read x[0] -- uc is 0 there -- one cached sector.)
  double xv[NU];
#pragma unroll
  for (int q = 0; q < NU; q++) xv[q] = xg[(MI_ABLATE & 1) ? min(uc[q], 63) : uc[q]];
  // the entry range of the first row a thread sums (operators that the tile Gauss-Seidel kernel also sweeps have
  // <= BLOCK rows per tile: one row per thread; SpMV-only operators with short rows -- P, R, the residual
  // sub-operator -- get up to 4 x BLOCK rows to fill their tiles)
  const int nr = r1 - r0;
  int G = 1;
  while (G < 64 && nr * G * 2 <= BLOCK) G <<= 1;
  const int lane = tid & (G - 1);
  const int rr = tid / G;
  int s0 = 0, s1 = 0;
  double bpre = 0.0;  // EPI 0 with beta != 0: the b entry of this thread's row, requested with the other loads
  int ro = r0 + rr;   // EPI 0: where this thread's row lands in y (operators stored in another row order)
  if (rr < nr) {
    if (!(MI_ABLATE & 16)) {
      s0 = (int)((unsigned)ia[r0 + rr] - ia_off);
      s1 = (int)((unsigned)ia[r0 + rr + 1] - ia_off);
    }
    if (EPI == 0 && e.rowmap && lane == 0) ro = e.rowmap[r0 + rr];
    if (EPI == 0 && e.beta != 0.0 && lane == 0) bpre = epi_b(e, ro);
  }
  if (VAL8 && tid < 256) slut[tid] = lutv;  // visible after the barrier below
#pragma unroll
  for (int q = 0; q < NU; q++) {
    const int k = tid + q * BLOCK;
    if (k < nu) xs[k] = xv[q];
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < NIT; it++) {
    const int k = 2 * tid + it * 2 * BLOCK;
    if (k < cnt) {
      const bool ok0 = (base_al + k >= base);
      const bool ok1 = (base_al + k + 1 < end);
      if (VAL8) {
        vv[it].x = slut[vw[it] & 0xffu];
        vv[it].y = slut[vw[it] >> 8];
      }
      if (VAL4) {
        vv[it].x = (double)vf[it].x;
        vv[it].y = (double)vf[it].y;
      }
      vv[it].x = ok0 ? vv[it].x * xs[cw[it] & XC_ID_MASK] : 0.0;
      vv[it].y = ok1 ? vv[it].y * xs[(cw[it] >> 16) & XC_ID_MASK] : 0.0;
    }
  }
  if (MI_ABLATE & 8) {
    double s = (double)(s1 - s0);
#pragma unroll
    for (int it = 0; it < NIT; it++) s += vv[it].x + vv[it].y;
    if (rr < nr && lane == 0 && (!(MI_ABLATE & 32) || s == -12345.0)) __builtin_nontemporal_store(e.alpha * s + e.beta * bpre, y + ro);
    return;
  }
  __syncthreads();  // every x-cache read is done: the array becomes the product buffer
#pragma unroll
  for (int it = 0; it < NIT; it++) {
    const int k = 2 * tid + it * 2 * BLOCK;
    if (k < cnt) {
      prod[k] = vv[it].x;
      prod[k + 1] = vv[it].y;
    }
  }
  __syncthreads();
  if (rr < nr) {
    double s = 0.0;
    for (int k = s0 + lane; k < s1; k += G) s += prod[k];
    for (int off = G >> 1; off > 0; off >>= 1) s += __shfl_down(s, off, G);
    if (lane == 0) {
      if (EPI == 0)
        __builtin_nontemporal_store((e.beta == 0.0) ? e.alpha * s : e.alpha * s + e.beta * bpre, y + ro);
      else
        epilogue<EPI>(r0 + rr, s, x, y, e);
    }
  }
  // tiles with more rows than threads (G == 1 there): the remaining rows, one lane each
  for (int r2 = tid + BLOCK; r2 < nr; r2 += BLOCK) {
    const int a0 = (int)((unsigned)ia[r0 + r2] - ia_off), a1 = (int)((unsigned)ia[r0 + r2 + 1] - ia_off);
    double s = 0.0;
    for (int k = a0; k < a1; k++) s += prod[k];
    epilogue<EPI>(r0 + r2, s, x, y, e);
  }
}

// ---------------------------------------------------------------------------
// spmv_stream_xc, epilogue 0, for the NV components of a multivector in one pass over the operator:
//   y_c = alpha A x_c + beta b_c,   c = 0 .. NV-1
// The part of spmv_stream_xc that does not depend on the vector -- descriptor, column list, column words, value
// stream, the rows' entry ranges and their place in y -- is requested once per tile and stays in registers (the values
// as doubles, whatever the storage format: the dictionary is looked up and the floats are widened once).  The part that
// does -- gather -> LDS x cache -> products -> product buffer -> row sums -> store -- runs once per component, with
// that kernel's operands in that kernel's order, so every component gets the bits the single-vector kernel gives it
// (tests/test_gpu_multivector_batch.py).  The gathers of component c + 1 are issued as soon as the x cache of
// component c stands, and land while its products and row sums are formed.
// Every vector carries its own component stride (MvStrides, in doubles): Krylov multivectors are component-major
// with the local row count as stride, level vectors with the level's.
// ---------------------------------------------------------------------------
struct MvStrides {
  long long x, y, b, b_lo;
};
template <int NV, int TAG, bool VAL8, int BLOCK, bool VAL4 = false>
__global__ __launch_bounds__(BLOCK) void spmv_stream_xc_mv(int nb, int xchunk, const int *__restrict__ tdesc,
                                                           const int *__restrict__ ia, const int *__restrict__ ja,
                                                           const double *__restrict__ av,
                                                           const int *__restrict__ ucols,
                                                           const unsigned short *__restrict__ lcol,
                                                           const double *__restrict__ x, double *__restrict__ y,
                                                           EpiArgs e, MvStrides st,
                                                           const unsigned char *__restrict__ vidx,
                                                           const double *__restrict__ vlut) {
  static_assert(!(VAL8 && VAL4), "one value format per instantiation");
  static_assert(NV >= 2 && NV <= 4, "2, 3 or 4 components per pass");
  constexpr int TILE = 8 * BLOCK;
  __shared__ double prod[TILE];
  __shared__ double slut[VAL8 ? 256 : 1];
  double *xs = prod;
  const int blk = xcd_remap(blockIdx.x, xchunk);
  if (blk >= nb) return;
  const int tid = threadIdx.x;
  double lutv = 0.0;
  if (VAL8 && tid < 256) lutv = vlut[tid];
  const int4 d0 = reinterpret_cast<const int4 *>(tdesc)[2 * blk];
  const int4 d1 = reinterpret_cast<const int4 *>(tdesc)[2 * blk + 1];
  const int r0 = d0.x, r1 = d0.y, len = d0.w, u0 = d1.x, nu = d1.y;
  const long long base64 = ((long long)d1.z << 32) | (long long)(unsigned)d0.z;
  if (len >= TILE) {
    // one row longer than the tile: one pass over it, one accumulator per component
    double s[NV];
#pragma unroll
    for (int c = 0; c < NV; c++) s[c] = 0.0;
    for (long long k = base64 + tid; k < base64 + len; k += BLOCK) {
      const double a = VAL4 ? (double)reinterpret_cast<const float *>(av)[k] : av[k];
      const int j = ja[k];
#pragma unroll
      for (int c = 0; c < NV; c++) s[c] += a * x[c * st.x + j];
    }
#pragma unroll
    for (int c = 0; c < NV; c++) {
      const double sc = wave_sum(s[c]);
      if ((tid & 63) == 0) prod[c * (BLOCK / 64) + (tid >> 6)] = sc;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int c = 0; c < NV; c++) {
        const double *pc = prod + c * (BLOCK / 64);
        double tot = pc[0] + pc[1] + pc[2] + pc[3];
        for (int wv = 4; wv < BLOCK / 64; wv++) tot += pc[wv];
        EpiArgs ec = e;
        ec.b = e.b + c * st.b;
        ec.b_lo = e.b_lo ? e.b_lo + c * st.b_lo : nullptr;
        epilogue<0>(r0, tot, x + c * st.x, y + c * st.y, ec);
      }
    }
    return;
  }
  constexpr int NU = TILE / BLOCK;
  int uc[NU];
#pragma unroll
  for (int q = 0; q < NU; q++) {
    const int k = tid + q * BLOCK;
    uc[q] = 0;  // (a select, see spmv_stream_xc)
    if (k < nu) uc[q] = LIST_LOAD(ucols + u0 + k);
  }
  const long long base_al64 = base64 & ~1LL;
  const int base = (int)(base64 - base_al64);  // tile-local: the aligned start is 0, the first entry 0 or 1
  const int end = base + len;
  const int cnt = end;
  const unsigned ia_off = (unsigned)base_al64;
  const float *av4 = reinterpret_cast<const float *>(av) + base_al64;
  av += base_al64;
  lcol += base_al64;
  if (VAL8) vidx += base_al64;
  constexpr int NIT = TILE / (2 * BLOCK);
  d2_t vv[NIT];      // the values: as loaded (fp64), or from the first barrier on (dictionary, fp32)
  f2_t vf[NIT];
  unsigned cw[NIT], vw[NIT];
#pragma unroll
  for (int it = 0; it < NIT; it++) {
    const int k = 2 * tid + it * 2 * BLOCK;
    cw[it] = 0;
    vw[it] = 0;
    vv[it] = d2_t{0.0, 0.0};
    if (k < cnt) {
      if (VAL8)
        vw[it] = STREAM_LOAD(reinterpret_cast<const unsigned short *>(vidx + k));
      else if (VAL4)
        vf[it] = STREAM_LOAD(reinterpret_cast<const f2_t *>(av4 + k));
      else
        vv[it] = STREAM_LOAD(reinterpret_cast<const d2_t *>(av + k));
      cw[it] = STREAM_LOAD(reinterpret_cast<const unsigned *>(lcol + k));
    }
  }
  double xv[NU];
#pragma unroll
  for (int q = 0; q < NU; q++) xv[q] = x[uc[q]];
  const int nr = r1 - r0;
  int G = 1;
  while (G < 64 && nr * G * 2 <= BLOCK) G <<= 1;
  const int lane = tid & (G - 1);
  const int rr = tid / G;
  int s0 = 0, s1 = 0;
  int ro = r0 + rr;
  if (rr < nr) {
    s0 = (int)((unsigned)ia[r0 + rr] - ia_off);
    s1 = (int)((unsigned)ia[r0 + rr + 1] - ia_off);
    if (e.rowmap && lane == 0) ro = e.rowmap[r0 + rr];
  }
  if (VAL8 && tid < 256) slut[tid] = lutv;  // visible after the first barrier
#pragma unroll 1
  for (int c = 0; c < NV; c++) {
    const double *bc = e.b + c * st.b;
    const double *bloc = e.b_lo ? e.b_lo + c * st.b_lo : nullptr;
    double *yc = y + c * st.y;
    double bpre = 0.0;
    if (rr < nr && e.beta != 0.0 && lane == 0) bpre = ((bloc && ro < e.b_split) ? bloc : bc)[ro];
#pragma unroll
    for (int q = 0; q < NU; q++) {
      const int k = tid + q * BLOCK;
      if (k < nu) xs[k] = xv[q];
    }
    __syncthreads();
    if (c + 1 < NV) {  // the next component's gathers, in flight through the rest of this one
      const double *xn = x + (c + 1) * st.x;
#pragma unroll
      for (int q = 0; q < NU; q++) xv[q] = xn[uc[q]];
    }
    if (c == 0 && (VAL8 || VAL4)) {
#pragma unroll
      for (int it = 0; it < NIT; it++) {
        if (VAL8) {
          vv[it].x = slut[vw[it] & 0xffu];
          vv[it].y = slut[vw[it] >> 8];
        } else {
          vv[it].x = (double)vf[it].x;
          vv[it].y = (double)vf[it].y;
        }
      }
    }
    d2_t pv[NIT];
#pragma unroll
    for (int it = 0; it < NIT; it++) {
      const int k = 2 * tid + it * 2 * BLOCK;
      pv[it] = d2_t{0.0, 0.0};
      if (k < cnt) {
        const bool ok0 = (k >= base);
        const bool ok1 = (k + 1 < end);
        pv[it].x = ok0 ? vv[it].x * xs[cw[it] & XC_ID_MASK] : 0.0;
        pv[it].y = ok1 ? vv[it].y * xs[(cw[it] >> 16) & XC_ID_MASK] : 0.0;
      }
    }
    __syncthreads();  // every x-cache read is done: the array becomes the product buffer
#pragma unroll
    for (int it = 0; it < NIT; it++) {
      const int k = 2 * tid + it * 2 * BLOCK;
      if (k < cnt) {
        prod[k] = pv[it].x;
        prod[k + 1] = pv[it].y;
      }
    }
    __syncthreads();
    if (rr < nr) {
      double s = 0.0;
      for (int k = s0 + lane; k < s1; k += G) s += prod[k];
      for (int off = G >> 1; off > 0; off >>= 1) s += __shfl_down(s, off, G);
      if (lane == 0)
        __builtin_nontemporal_store((e.beta == 0.0) ? e.alpha * s : e.alpha * s + e.beta * bpre, yc + ro);
    }
    if (nr > BLOCK) {  // tiles with more rows than threads (G == 1 there): the remaining rows, one lane each
      EpiArgs ec = e;
      ec.b = bc;
      ec.b_lo = bloc;
      for (int r2 = tid + BLOCK; r2 < nr; r2 += BLOCK) {
        const int a0 = (int)((unsigned)ia[r0 + r2] - ia_off), a1 = (int)((unsigned)ia[r0 + r2 + 1] - ia_off);
        double s = 0.0;
        for (int k = a0; k < a1; k++) s += prod[k];
        epilogue<0>(r0 + r2, s, x, yc, ec);
      }
    }
    if (c + 1 < NV) __syncthreads();  // the row sums are done: the array becomes the next component's x cache
  }
}

__global__ __launch_bounds__(256) void tile_desc_k(int nb, const int *__restrict__ rb, const long long *__restrict__ ia,
                                                   const int *__restrict__ uptr, int *__restrict__ desc) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nb) return;
  const int r0 = rb[b], r1 = rb[b + 1];
  int4 *d = reinterpret_cast<int4 *>(desc) + 2 * (size_t)b;
  const int u0 = uptr ? uptr[b] : 0, u1 = uptr ? uptr[b + 1] : 0;
  const long long base = ia[r0], len = ia[r1] - base;
  // a single row longer than any tile (>= 2^31 entries it cannot be: such rows do not exist) keeps its true length
  d[0] = make_int4(r0, r1, (int)(unsigned)(base & 0xffffffffLL), (int)(len > 0x7fffffffLL ? 0x7fffffffLL : len));
  d[1] = make_int4(u0, u1 - u0, (int)(base >> 32), 0);
}

// compressed-row off-diagonal block: one lane per stored row (halo rows are few
// and short); MODE 0: y[row] += alpha*s ; MODE 1: y[row] = s
template <int MODE>
__global__ __launch_bounds__(256) void spmv_offd_k(int nrc, const int *__restrict__ rows, const int *__restrict__ ia,
                                                   const int *__restrict__ ja, const double *__restrict__ av,
                                                   const double *__restrict__ xext, double alpha,
                                                   double *__restrict__ y) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nrc) return;
  double s = 0.0;
  for (int q = ia[k]; q < ia[k + 1]; q++) s += av[q] * xext[ja[q]];
  const int r = rows[k];
  if (MODE == 0)
    y[r] += alpha * s;
  else
    y[r] = s;
}

// ---------------------------------------------------------------------------
// Hybrid Gauss-Seidel: lane c owns the chunk of `chunk` consecutive rows
// [c*chunk, ...), sweeps it sequentially (forward and/or backward) with its own
// running values in LDS, and reads every other chunk's PRE-sweep value from
// u_old.  This is HYPRE's hybrid smoother with chunks in the role of its
// threads/ranks (par_relax.c) and is bitwise independent of
// scheduling because u_old is never written.
// ---------------------------------------------------------------------------
template <class VT>
__global__ __launch_bounds__(GS_BLOCK) void gs_hybrid_k(int n, int chunk0, int nchunks, int chunk, const int *__restrict__ ia,
                                                        const int *__restrict__ ja, const VT *__restrict__ av,
                                                        const signed char *__restrict__ cf, int points,
                                                        const double *__restrict__ dd, const double *__restrict__ f,
                                                        const double *__restrict__ offc,
                                                        const double *__restrict__ u_lo,
                                                        const double *__restrict__ u_hi, int split,
                                                        double *__restrict__ u_new, int fwd, int bwd, double w) {
#define UOLD(j) (((j) < split ? u_lo : u_hi)[(j)])
  extern __shared__ double ucur[];  // [chunk][GS_BLOCK]
  const int tid = threadIdx.x;
  const long long c = chunk0 + (long long)blockIdx.x * GS_BLOCK + tid;
  if (c >= nchunks) return;
  const int cs = (int)(c * chunk);
  const int len = min(chunk, n - cs);
  for (int t = 0; t < len; t++) ucur[t * GS_BLOCK + tid] = UOLD(cs + t);
  for (int dir = 0; dir < 2; dir++) {
    if (dir == 0 ? !fwd : !bwd) continue;
    for (int t = 0; t < len; t++) {
      const int tt = (dir == 0) ? t : len - 1 - t;
      const int i = cs + tt;
      if (points != 0 && cf != nullptr && cf[i] != points) continue;
      const double d = dd[i];
      if (d == 0.0) continue;
      double res = f[i];
      if (offc) res -= offc[i];
      const int k1 = ia[i + 1];
      for (int k = ia[i]; k < k1; k++) {
        const int j = ja[k];
        const unsigned o = (unsigned)(j - cs);
        const double v = (o < (unsigned)len) ? ucur[o * GS_BLOCK + tid] : UOLD(j);
        res -= (double)av[k] * v;
      }
      ucur[tt * GS_BLOCK + tid] += w * res / d;
    }
  }
  for (int t = 0; t < len; t++) u_new[cs + t] = ucur[t * GS_BLOCK + tid];
#undef UOLD
}

// ---------------------------------------------------------------------------
// Hybrid Gauss-Seidel, cooperative form (chunk == 8, mean row length <= 8).
// A group of LPC = 8 lanes owns one chunk of R = 8 consecutive rows; a wave
// holds 64/LPC chunks, so for the 7-point fine level the wave's 64 lanes read
// 64 consecutive rows' entries.
//   phase A  every row of the chunk is loaded up front: lane g takes entries
//            g, g+LPC, ... of each row (adjacent lanes -> adjacent addresses),
//            and gathers u_old for the columns outside the chunk.  Nothing in
//            this phase depends on the sweep, so all loads are in flight at once.
//   phase B  the 8 rows are swept in order (forward and/or backward).  The
//            chunk's running values live one per lane (lane g holds row g) and
//            are read with __shfl; the row's dot product is a __shfl_xor
//            butterfly over the group.
// u_old is never written, so the result does not depend on scheduling.
// ---------------------------------------------------------------------------
// 64-bit DPP move (two dword moves); CTRL is a DPP control word
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
// sum over an aligned group of LPC lanes, result in every lane of the group.
// quad_perm [1,0,3,2] = 0xB1, [2,3,0,1] = 0x4E, row_half_mirror = 0x141,
// row_mirror = 0x140: cross-lane moves in the VALU, no LDS crossbar; only the
// 32- and 64-lane steps go through ds_bpermute.
template <int LPC>
__device__ __forceinline__ double group_sum(double v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x141>(v);
  if (LPC >= 16) v += dpp_mov<0x140>(v);
  if (LPC >= 32) v += __shfl_xor(v, 16, 64);
  if (LPC >= 64) v += __shfl_xor(v, 32, 64);
  return v;
}

template <int LPC, int E, class VT = double>
__global__ __launch_bounds__(256) void gs_group_k(int n, int chunk0, int nchunks, const int *__restrict__ ia,
                                                  const int *__restrict__ ja, const VT *__restrict__ av,
                                                  const signed char *__restrict__ cf, int points,
                                                  const double *__restrict__ dd, const double *__restrict__ f,
                                                  const double *__restrict__ offc,
                                                  const double *__restrict__ u_lo,
                                                  const double *__restrict__ u_hi, int split,
                                                  double *__restrict__ u_new, int fwd, int bwd, double w,
                                                  int zero_from) {
#define UOLD(j) (((j) < split ? u_lo : u_hi)[(j)])
  constexpr int R = 8;
  constexpr int CPW = 64 / LPC;
  const int lane = threadIdx.x & 63;
  const int g = lane & (LPC - 1);
  const int gbase = lane & ~(LPC - 1);
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const long long c = chunk0 + wave * CPW + (lane / LPC);
  const bool live = c < nchunks;
  const int cs = live ? (int)(c * R) : 0;
  const int len = live ? min(R, n - cs) : 0;

  // owner lane g < len holds the state of row cs+g
  double myu = 0.0, myrhs = 0.0, myd = 0.0;
  bool mysel = false;
  int my_k0 = 0, my_k1 = 0;
  if (g < len) {
    const int i = cs + g;
    my_k0 = ia[i];
    const int a1 = ia[i + 1];
    const int mark = (points != 0 && cf != nullptr) ? (int)cf[i] : points;
    myu = (i >= zero_from) ? 0.0 : UOLD(i);
    myd = dd[i];
    myrhs = f[i];
    if (offc) myrhs -= offc[i];
    const bool rowsel = (mark == points);
    my_k1 = rowsel ? a1 : my_k0;  // unselected rows load nothing
    mysel = rowsel && myd != 0.0;
  }
  // one division per row, outside the sweep (the sweep's VALU work is what bounds this kernel)
  const double mywd = mysel ? w / myd : 0.0;
  // phase A: three waves of independent loads (row pointers + marker, entries,
  // gathers).  Per entry one double survives: a_ij*u_old[j] for a column outside
  // the chunk, a_ij itself for a column inside it; the in-chunk offset (or 15)
  // of the 8 rows is packed 4 bits each into one register per strip.
  int k0s[R], k1s[R];
  unsigned longmask = 0;
#pragma unroll
  for (int t = 0; t < R; t++) {
    k0s[t] = __shfl(my_k0, gbase + t, 64);
    k1s[t] = __shfl(my_k1, gbase + t, 64);
  }
  double wv[R][E];
  int cols[R][E];
#pragma unroll
  for (int t = 0; t < R; t++) {
    if (k1s[t] - k0s[t] > LPC * E) longmask |= 1u << t;
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int k = k0s[t] + g + e * LPC;
      const bool ok = k < k1s[t];
      wv[t][e] = ok ? (double)av[k] : 0.0;
      cols[t][e] = ok ? ja[k] : cs;
    }
  }
  unsigned code[E];
#pragma unroll
  for (int e = 0; e < E; e++) code[e] = 0;
#pragma unroll
  for (int t = 0; t < R; t++) {
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int j = cols[t][e];
      const unsigned oo = (unsigned)(j - cs);
      const bool inch = oo < (unsigned)len;
      // gather issued without waiting on the in-chunk test; columns >= zero_from hold zeros by contract
      const double x = (j >= zero_from) ? 0.0 : UOLD(j);
      code[e] |= (inch ? oo : 15u) << (4 * t);
      if (!inch) wv[t][e] *= x;
    }
  }
  // phase B
#pragma unroll
  for (int dir = 0; dir < 2; dir++) {
    if (dir == 0 ? !fwd : !bwd) continue;
#pragma unroll
    for (int tt = 0; tt < R; tt++) {
      const int t = (dir == 0) ? tt : R - 1 - tt;
      double part = 0.0;
#pragma unroll
      for (int e = 0; e < E; e++) {
        const unsigned o = (code[e] >> (4 * t)) & 15u;
        const double cur = __shfl(myu, gbase + (int)(o & 7u), 64);
        part += (o == 15u) ? wv[t][e] : wv[t][e] * cur;
      }
      if (longmask & (1u << t)) {  // entries beyond the preloaded strips (group-uniform branch)
        const int i = cs + t;
        const int k1 = ia[i + 1];
        for (int k = ia[i] + LPC * E + g; k - g < k1; k += LPC) {
          double v = 0.0, x = 0.0;
          int o = -1;
          if (k < k1) {
            v = (double)av[k];
            const int j = ja[k];
            const unsigned oo = (unsigned)(j - cs);
            if (oo < (unsigned)len)
              o = (int)oo;
            else if (j < zero_from)
              x = UOLD(j);
          }
          const double cur = __shfl(myu, gbase + (o < 0 ? 0 : o), 64);
          part += v * (o < 0 ? x : cur);
        }
      }
      const double sum = group_sum<LPC>(part);
      if (g == t && mysel) myu += (myrhs - sum) * mywd;
    }
  }
  if (g < len) u_new[cs + g] = myu;
#undef UOLD
}


// ---------------------------------------------------------------------------
// Hybrid Gauss-Seidel, dense-chunk formulation (the default for chunk = 8).
//
// gs_group_k above sweeps the 8 rows of a chunk with one cross-lane reduction and
// one division per row and direction; counters showed its VALU pipes saturated
// (955 VALU instructions per wave, 100 % busy) while HBM idled at ~2 TB/s.  Here
// everything that does not depend on the sweep order leaves the serial part:
//   * entries with a column outside the chunk multiply the snapshot of u: their
//     8 row sums are reduced ONCE over the group by a reduce-scatter butterfly
//     (8 -> 4 -> 2 -> 1 values per lane while the lane count halves) and serve the
//     forward and the backward sweep;
//   * entries inside the chunk (diagonal included) are scattered into a dense
//     8x8 block in LDS, one block per chunk; owner lane t then holds row t of the
//     block in registers;
//   * rows longer than the preloaded strips are finished in the same pre-sweep
//     phase (no slow path inside the sweep);
//   * the sweep itself is 8 fused multiply-adds per row on the owner lanes, one
//     multiplication by the precomputed w/d, and one broadcast of the new value.
// ---------------------------------------------------------------------------
// LDS accesses of one wave are processed in issue order; this only keeps the compiler from moving them
__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int CTRL>
__device__ __forceinline__ double dpp_xchg(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
// value of the partner lane for the exchange step with distance M inside an aligned group:
// M = 1, 2: xor; 4: mirror inside 8 lanes; 8: mirror inside 16 lanes (both pair the two halves); 16, 32: xor
template <int M>
__device__ __forceinline__ double partner(double v) {
  if (M == 1) return dpp_xchg<0xB1>(v);
  if (M == 2) return dpp_xchg<0x4E>(v);
  if (M == 4) return dpp_xchg<0x141>(v);
  if (M == 8) return dpp_xchg<0x140>(v);
  return __shfl_xor(v, M, 64);
}

// reduce-scatter step: NV values per lane -> NV/2; lanes whose bit M is clear keep the lower half of the rows
template <int M, int NV>
__device__ __forceinline__ void rs_step(double *p, int g) {
  const bool hi = (g & M) != 0;
#pragma unroll
  for (int q = 0; q < NV / 2; q++) {
    const double keep = hi ? p[NV / 2 + q] : p[q];
    const double send = hi ? p[q] : p[NV / 2 + q];
    p[q] = keep + partner<M>(send);
  }
}

template <int LPC, int E, class VT = double>
__global__ __launch_bounds__(256) void gs_dense_k(int n, int chunk0, int nchunks, const int *__restrict__ ia,
                                                  const int *__restrict__ ja, const VT *__restrict__ av,
                                                  const signed char *__restrict__ cf, int points,
                                                  const double *__restrict__ dd, const double *__restrict__ f,
                                                  const double *__restrict__ offc,
                                                  const double *__restrict__ u_lo,
                                                  const double *__restrict__ u_hi, int split,
                                                  double *__restrict__ u_new, int fwd, int bwd, double w,
                                                  int /*zero_from: not used, the vector holds real zeros*/) {
#define UOLD(j) (((j) < split ? u_lo : u_hi)[(j)])
  constexpr int R = 8;
  constexpr int CPW = 64 / LPC;
  constexpr int GPB = 256 / LPC;
  __shared__ double Cs[GPB][R][R];
  const int lane = threadIdx.x & 63;
  const int g = lane & (LPC - 1);
  const int gbase = lane & ~(LPC - 1);
  const int grp = threadIdx.x / LPC;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const long long c = chunk0 + wave * CPW + (lane / LPC);
  const bool live = c < nchunks;
  const int cs = live ? (int)(c * R) : 0;
  const int len = live ? min(R, n - cs) : 0;

  // owner lane g < len holds the state of row cs+g
  double myu = 0.0, myrhs = 0.0, wd = 0.0;
  int my_k0 = 0, my_k1 = 0;
  if (g < len) {
    const int i = cs + g;
    my_k0 = ia[i];
    const int a1 = ia[i + 1];
    const int mark = (points != 0 && cf != nullptr) ? (int)cf[i] : points;
    myu = UOLD(i);
    const double myd = dd[i];
    myrhs = f[i];
    if (offc) myrhs -= offc[i];
    const bool rowsel = (mark == points);
    my_k1 = rowsel ? a1 : my_k0;  // unselected rows load nothing
    if (rowsel && myd != 0.0) wd = w / myd;
  }
  {
    double *blk = &Cs[grp][0][0];
#pragma unroll
    for (int q = g; q < R * R; q += LPC) blk[q] = 0.0;
  }
  int k0s[R], k1s[R];
#pragma unroll
  for (int t = 0; t < R; t++) {
    k0s[t] = __shfl(my_k0, gbase + t, 64);
    k1s[t] = __shfl(my_k1, gbase + t, 64);
  }
  double wv[R][E];
  int cols[R][E];
#pragma unroll
  for (int t = 0; t < R; t++) {
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int k = k0s[t] + g + e * LPC;
      const bool ok = k < k1s[t];
      wv[t][e] = ok ? (double)av[k] : 0.0;
      cols[t][e] = ok ? ja[k] : -1;
    }
  }
  wave_sync_lds();  // the block is zero before the scatter below (a chunk's block is private to its wave)
  double p[R];
#pragma unroll
  for (int t = 0; t < R; t++) {
    p[t] = 0.0;
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int j = cols[t][e];
      const unsigned oo = (unsigned)(j - cs);
      const bool inch = (j >= 0) && oo < (unsigned)len;
      const double x = UOLD(j < 0 ? cs : j);  // unconditional gather: no load waits on a branch
      if (inch)
        Cs[grp][t][oo] = wv[t][e];
      else
        p[t] += wv[t][e] * x;
    }
    if (k1s[t] - k0s[t] > LPC * E) {  // the rest of a long row (uniform inside the group)
      for (int k = k0s[t] + LPC * E + g; k < k1s[t]; k += LPC) {
        const double a = (double)av[k];
        const int j = ja[k];
        const unsigned oo = (unsigned)(j - cs);
        if (oo < (unsigned)len)
          Cs[grp][t][oo] = a;
        else
          p[t] += a * UOLD(j);
      }
    }
  }
  // row sums of the out-of-chunk part: reduce-scatter over the group, then the owners fetch theirs
  rs_step<LPC / 2, 8>(p, g);
  if (LPC >= 16) rs_step<(LPC >= 16 ? LPC / 4 : 1), 4>(p, g); else rs_step<2, 4>(p, g);
  if (LPC >= 32) rs_step<(LPC >= 32 ? LPC / 8 : 1), 2>(p, g); else if (LPC == 16) rs_step<2, 2>(p, g); else rs_step<1, 2>(p, g);
  double S = p[0];  // full sum of row g / (LPC / 8) once the low bits are folded in
  if (LPC >= 16) {
    S += partner<1>(S);
    if (LPC >= 32) S += partner<2>(S);
    if (LPC >= 64) S += partner<4>(S);
  }
  if (LPC > 8) S = __shfl(S, gbase + (g & 7) * (LPC / 8), 64);
  wave_sync_lds();  // the dense block is complete
  double crow[R], uc[R];
  {
    const int r = g & 7;
#pragma unroll
    for (int j = 0; j < R; j++) crow[j] = Cs[grp][r][j];
  }
#pragma unroll
  for (int j = 0; j < R; j++) uc[j] = __shfl(myu, gbase + j, 64);
#pragma unroll
  for (int dir = 0; dir < 2; dir++) {
    if (dir == 0 ? !fwd : !bwd) continue;
#pragma unroll
    for (int tt = 0; tt < R; tt++) {
      const int t = (dir == 0) ? tt : R - 1 - tt;
      double s = S;
#pragma unroll
      for (int j = 0; j < R; j++) s += crow[j] * uc[j];
      const double nu = myu + (myrhs - s) * wd;  // unselected rows: wd == 0
      double b;
      if (LPC == 64) {
        const int lo = __builtin_amdgcn_readlane(__double2loint(nu), t);
        const int hi = __builtin_amdgcn_readlane(__double2hiint(nu), t);
        b = __hiloint2double(hi, lo);
      } else {
        b = __shfl(nu, gbase + t, 64);
      }
      uc[t] = b;
      if (g == t) myu = b;
    }
  }
  if (g < len) u_new[cs + g] = myu;
#undef UOLD
}


// ---------------------------------------------------------------------------
// The dense 8x8 in-chunk sweep of gs_tile_k: crow[] = the lane's row of the chunk's block, uc[] = the lane's copy of
// the chunk's eight values (filled here), myu = the row's value before / after.
// The phase is VALU throughput (profiles/r04_ablation_tile_kernels.txt: 16 steps x (8 double FMAs + update + cross-lane
// read) on every wave = a quarter of a pass).  Every lane forms ITS row's sum at every step although only row t's is
// used at step t; what can be shared without touching the order of the additions (S, then columns 0..7 ascending):
// * forward, rows above t already hold their new values when row t's turn comes, and they are the FIRST terms of its
//   sum: `acc` = S + the terms of the columns swept so far is carried along (one FMA per step), step t adds the 8 - t
//   remaining terms to a copy of it -- 44 instead of 64 FMAs.  (Backward the new values are the LAST terms; the prefix
//   over the old ones has a different length in every lane, and masking it costs what it saves: all 8 terms there.)
// * the row's own value at its step is uc[t] (the lane's copy of the chunk's values), so `myu` need not follow the
//   sweep: it is picked out of uc[] once at the end instead of a select per step.
// Same operations on the same operands for the row whose turn it is; the other lanes' results were never used.
// zero_tile (uniform in the workgroup): every value of the chunk is 0 before the sweep.  The values are then not
// fetched from the other lanes, and in the forward sweep the terms over the columns not yet swept (j >= t) are
// products with 0: step t needs the carried `acc` alone -- 8 instead of 44 FMAs.  A backward sweep that follows (or
// comes alone) is the general one.
// A step reads lane gbase + t * LPR (below 64).  The byte address for ds_bpermute_b32 is formed at the step, one add of
// a scalar to the lane's 4 * gbase: held in registers through both sweeps, the eight addresses cost 8 VGPRs that the
// kernel does not have, and the compiler would otherwise hold them (the empty asm keeps the add where it is used).
__device__ __forceinline__ double gs_lane_read(const double v, const int gbase4, int off4) {
  asm volatile("" : "+s"(off4));
  const int lo = __builtin_amdgcn_ds_bpermute(gbase4 + off4, __double2loint(v));
  const int hi = __builtin_amdgcn_ds_bpermute(gbase4 + off4, __double2hiint(v));
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ void gs_tile_sweep(const double (&crow)[8], double (&uc)[8], double &myu, const double S,
                                              const double myrhs, const double wd, const int g, const int gbase,
                                              const int LPR, const int fwd, const int bwd, const bool zero_tile) {
#if !defined(MI_GS_SHARED_PREFIX) || MI_GS_SHARED_PREFIX
  const int gbase4 = 4 * gbase;
  int LPR4 = 4 * LPR;  // one of four constants selected by the tile's row count: as a plain number, t * LPR4 is one scalar op
  asm volatile("" : "+s"(LPR4));
  if (zero_tile) {
#pragma unroll
    for (int j = 0; j < 8; j++) uc[j] = 0.0;
    if (fwd) {
      double acc = S;
#pragma unroll
      for (int t = 0; t < 8; t++) {
        const double nu2 = 0.0 + (myrhs - acc) * wd;  // unselected rows: wd == 0
        const double b = gs_lane_read(nu2, gbase4, t * LPR4);
        uc[t] = b;
        acc += crow[t] * b;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++) uc[j] = gs_lane_read(myu, gbase4, j * LPR4);
    if (fwd) {
      double acc = S;
#pragma unroll
      for (int t = 0; t < 8; t++) {
        double sacc = acc;
#pragma unroll
        for (int j = t; j < 8; j++) sacc += crow[j] * uc[j];
        const double nu2 = uc[t] + (myrhs - sacc) * wd;  // unselected rows: wd == 0
        const double b = gs_lane_read(nu2, gbase4, t * LPR4);
        uc[t] = b;
        acc += crow[t] * b;
      }
    }
  }
  if (bwd) {
#pragma unroll
    for (int tt = 0; tt < 8; tt++) {
      const int t = 7 - tt;
      double sacc = S;
#pragma unroll
      for (int j = 0; j < 8; j++) sacc += crow[j] * uc[j];
      const double nu2 = uc[t] + (myrhs - sacc) * wd;
      uc[t] = gs_lane_read(nu2, gbase4, t * LPR4);
    }
  }
  if (fwd || bwd) {
#pragma unroll
    for (int j = 0; j < 8; j++) myu = (g == j) ? uc[j] : myu;
  }
#else
  // the sweep before the shared prefix (A/B timing): every step forms the full sum; no zero-tile path
#pragma unroll
  for (int j = 0; j < 8; j++) uc[j] = __shfl(myu, gbase + j * LPR, 64);
#pragma unroll
  for (int dir = 0; dir < 2; dir++) {
    if (dir == 0 ? !fwd : !bwd) continue;
#pragma unroll
    for (int tt = 0; tt < 8; tt++) {
      const int t = (dir == 0) ? tt : 7 - tt;
      double sacc = S;
#pragma unroll
      for (int j = 0; j < 8; j++) sacc += crow[j] * uc[j];
      const double nu2 = myu + (myrhs - sacc) * wd;  // unselected rows: wd == 0
      const double b = __shfl(nu2, gbase + t * LPR, 64);
      uc[t] = b;
      if (g == t) myu = b;
    }
  }
#endif
}

// ---------------------------------------------------------------------------
// Hybrid Gauss-Seidel on the SpMV tiles (levels with an x cache).
//
// The chunk kernels above read the matrix row by row and gather u through L1;
// on the coarse levels they wait on memory most of the time (53 % L1 misses,
// 2 TB/s).  This kernel reads like spmv_stream_xc -- one workgroup per tile of
// <= 256 rows / < 2048 entries, matrix stream in aligned pairs, the tile's
// unique columns gathered once (coalesced) into LDS -- and then sweeps the
// tile's chunks: 8 lanes per chunk, lane g owns row g, sums its out-of-chunk
// products out of LDS, picks its in-chunk coefficients by the code bits of the
// 16-bit column entries, and runs the dense 8x8 sweep of gs_dense_k.
// ---------------------------------------------------------------------------
// VAL4: fp32 value storage, see spmv_stream_xc.
template <bool VAL8, int BLOCK, bool VAL4 = false>
__global__ __launch_bounds__(BLOCK, 2048 / BLOCK) void gs_tile_k(int blk0, int nblk, const int *__restrict__ tdesc,
                                                        const int *__restrict__ ia, const double *__restrict__ av,
                                                        const int *__restrict__ ucols,
                                                        const unsigned short *__restrict__ lcol,
                                                        const signed char *__restrict__ cf, int points,
                                                        const double *__restrict__ dd, const double *__restrict__ f,
                                                        const double *__restrict__ offc,
                                                        const double *__restrict__ u_lo,
                                                        const double *__restrict__ u_hi, int split,
                                                        double *__restrict__ u_new, int fwd, int bwd, double w,
                                                        int row_begin, int row_end, int zero_from,
                                                        double *__restrict__ tout, int t_from,
                                                        const unsigned char *__restrict__ vidx,
                                                        const double *__restrict__ vlut, double *__restrict__ wout) {
#define UOLD(j) (((j) < split ? u_lo : u_hi)[(j)])
  constexpr int TILE = 8 * BLOCK;        // TILE / TILE_WIDE
  __shared__ double buf[TILE];           // x cache, then products / in-chunk coefficients
  // the entries' lcol words.  The value dictionary (see spmv_stream_xc) lives in the first 2 KB of the same bytes,
  // which are only written as `code` after the last lookup (second barrier) -- no LDS beyond the 20 KB that allow
  // 8 workgroups per CU.  One 8-byte-aligned byte array with two typed views.
  __shared__ __attribute__((aligned(8))) unsigned char code_bytes[TILE * sizeof(unsigned short)];
  static_assert(TILE * sizeof(unsigned short) >= 256 * sizeof(double), "the value table must fit the code array");
  unsigned short *code = reinterpret_cast<unsigned short *>(code_bytes);
  double *slut = reinterpret_cast<double *>(code_bytes);
  if ((int)blockIdx.x >= nblk) return;
  const int blk = blk0 + blockIdx.x;
  const int tid = threadIdx.x;
  double lutv = 0.0;  // stored to LDS with the x cache (see spmv_stream_xc)
  if (VAL8 && tid < 256) lutv = vlut[tid];
  // one descriptor load, then the loads in the order of their dependent chains (see spmv_stream_xc): column
  // list, matrix stream, the gathers as soon as the column ids are back, then the per-row data (C/F mark -> row
  // selected? -> divisor, right-hand side, row pointers: loads that wait for each other)
  const int4 d0 = reinterpret_cast<const int4 *>(tdesc)[2 * blk];
  const int4 d1 = reinterpret_cast<const int4 *>(tdesc)[2 * blk + 1];
  const int r0 = d0.x, r1 = d0.y, len = d0.w, u0 = d1.x, nu = d1.y;
  const long long base64 = ((long long)d1.z << 32) | (long long)(unsigned)d0.z;  // see spmv_stream_xc
  // columns >= zero_from hold zeros by contract (first sweep on a zero guess): nothing to gather there --
  // the unique columns ascend, so for zero_from == 0 not even the ids are read
  const bool all_zero = zero_from <= 0;
  constexpr int NU = TILE / BLOCK;
  int ucid[NU];
  if (!all_zero) {
#pragma unroll
    for (int q = 0; q < NU; q++) {
      const int k = tid + q * BLOCK;
      ucid[q] = 0;
      if (!(MI_ABLATE & 2) && k < nu) ucid[q] = LIST_LOAD(ucols + u0 + k);
    }
  }
  const long long base_al64 = base64 & ~1LL;
  const int base = (int)(base64 - base_al64), base_al = 0;  // tile-local from here on
  const int end = base + len;
  const int cnt = end;
  const unsigned ia_off = (unsigned)base_al64;
  const float *av4 = reinterpret_cast<const float *>(av) + base_al64;  // VAL4: the same argument, 4-byte entries
  av += base_al64;
  lcol += base_al64;
  if (VAL8) vidx += base_al64;
  constexpr int NIT = TILE / (2 * BLOCK);
  d2_t vv[NIT];
  f2_t vf[NIT];  // VAL4: two values, as loaded (widened after the first barrier)
  unsigned cw[NIT], vw[NIT];  // two 16-bit column words / two value indices, as loaded (see spmv_stream_xc)
#pragma unroll
  for (int it = 0; it < NIT; it++) {
    const int k = 2 * tid + it * 2 * BLOCK;
    cw[it] = 0;
    vw[it] = 0;
    if (MI_ABLATE & 4) vv[it] = d2_t{1.0, 1.0}, vf[it] = f2_t{1.0f, 1.0f};
    if (!(MI_ABLATE & 4) && k < cnt) {
      if (VAL8)
        vw[it] = STREAM_LOAD(reinterpret_cast<const unsigned short *>(vidx + base_al + k));
      else if (VAL4)
        vf[it] = STREAM_LOAD(reinterpret_cast<const f2_t *>(av4 + base_al + k));
      else
        vv[it] = STREAM_LOAD(reinterpret_cast<const d2_t *>(av + base_al + k));
      cw[it] = STREAM_LOAD(reinterpret_cast<const unsigned *>(lcol + base_al + k));
    }
  }
  // the gathers in flight together, before the first LDS write and before the per-row chain (see spmv_stream_xc); lanes
  // beyond the list and columns from zero_from on read entry 0 and are overwritten / not stored.  With 8-byte values in
  // registers all NU at once would cost 74 VGPRs (6 instead of 8 waves per SIMD): that variant takes them in two
  // batches -- the first covers tiles of up to 4 * BLOCK unique columns, i.e. nearly all of them.  With 4-byte values
  // (VAL4) the stream holds half the registers and all NU gathers go out at once, as with the dictionary.
  constexpr int GB = (VAL8 || VAL4) ? NU : NU / 2;
  double xv[GB];
  if (!all_zero) {
#pragma unroll
    for (int q = 0; q < GB; q++) {
      const int j = (ucid[q] >= zero_from) ? 0 : ((MI_ABLATE & 1) ? min(ucid[q], 63) : ucid[q]);
      xv[q] = UOLD(j);
    }
  }
  // LPR lanes per row, as many as this tile's row count leaves room for (uniform in the workgroup);
  // 8 * LPR consecutive lanes = one chunk; all lanes of a row carry its state, the first one writes it back
  const int nr = r1 - r0;
  const int LPR = nr <= BLOCK / 8 ? 8 : nr <= BLOCK / 4 ? 4 : nr <= BLOCK / 2 ? 2 : 1;
  const int rl = tid / LPR, sub = tid % LPR;
  const int i = r0 + rl;
  double myu = 0.0, myrhs = 0.0, wd = 0.0;
  bool rowsel = false;
  int s0 = 0, s1 = 0;
  if (rl < nr) {
    const int mark = (points != 0 && cf != nullptr) ? (int)cf[i] : points;
    myu = (i >= zero_from) ? 0.0 : UOLD(i);
    rowsel = (mark == points) && i >= row_begin && i < row_end;
    if (rowsel) {
      const double myd = dd[i];
      myrhs = f[i];
      if (offc) myrhs -= offc[i];
      if (myd != 0.0) wd = w / myd;
      s0 = (int)((unsigned)ia[i] - ia_off);
      s1 = (int)((unsigned)ia[i + 1] - ia_off);
    }
  }
  if (VAL8 && tid < 256) slut[tid] = lutv;
  if (!all_zero) {
#pragma unroll
    for (int q = 0; q < GB; q++) {
      const int k = tid + q * BLOCK;
      if (k < nu) buf[k] = (ucid[q] >= zero_from) ? 0.0 : xv[q];
    }
    if (GB < NU && nu > GB * BLOCK) {  // (uniform) the rare tile with more unique columns than the first batch holds
#pragma unroll
      for (int q = GB; q < NU; q++) {
        const int j = (ucid[q] >= zero_from) ? 0 : ucid[q];
        xv[q - GB] = UOLD(j);
      }
#pragma unroll
      for (int q = GB; q < NU; q++) {
        const int k = tid + q * BLOCK;
        if (k < nu) buf[k] = (ucid[q] >= zero_from) ? 0.0 : xv[q - GB];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < NIT; it++) {
    const int k = 2 * tid + it * 2 * BLOCK;
    if (k < cnt) {
      const bool ok0 = (base_al + k >= base);
      const bool ok1 = (base_al + k + 1 < end);
      const unsigned c0 = cw[it] & 0xffffu, c1 = cw[it] >> 16;
      if (VAL8) {
        vv[it].x = slut[vw[it] & 0xffu];
        vv[it].y = slut[vw[it] >> 8];
      }
      if (VAL4) {
        vv[it].x = (double)vf[it].x;
        vv[it].y = (double)vf[it].y;
      }
      // out-of-chunk: product with the snapshot value; in-chunk: the coefficient itself
      const double x0 = all_zero ? 0.0 : buf[c0 & XC_ID_MASK], x1 = all_zero ? 0.0 : buf[c1 & XC_ID_MASK];
      vv[it].x = ok0 ? ((c0 & XC_INCH) ? vv[it].x : vv[it].x * x0) : 0.0;
      vv[it].y = ok1 ? ((c1 & XC_INCH) ? vv[it].y : vv[it].y * x1) : 0.0;
    }
  }
  __syncthreads();  // every x-cache read is done
#pragma unroll
  for (int it = 0; it < NIT; it++) {
    const int k = 2 * tid + it * 2 * BLOCK;
    if (k < cnt) {
      buf[k] = vv[it].x;
      buf[k + 1] = vv[it].y;
      code[k] = (unsigned short)(cw[it] & 0xffffu);
      code[k + 1] = (unsigned short)(cw[it] >> 16);
    }
  }
  __syncthreads();
  // per row: out-of-chunk sum (the row's LPR lanes share the entries) and the row of the dense 8x8 chunk
  // block.  Columns ascend and a chunk is 8 consecutive ids, so the in-chunk entries of a row are ONE run
  // [kin, kin + popcount(mask)) of its entries, in ascending in-chunk offset: the loop only notes where the
  // run starts and which offsets occur; the coefficients are then read straight from the product buffer.
  double S = 0.0;
  unsigned inmask = 0;
  int kin = TILE;
  if (rowsel) {
    for (int k = s0 + sub; k < s1; k += LPR) {
      const unsigned c = code[k];
      const double v = buf[k];
      const bool in = (c & XC_INCH) != 0;
      S += in ? 0.0 : v;
      inmask |= in ? (1u << ((c >> XC_OFF_SHIFT) & 7)) : 0u;
      kin = in ? min(kin, k) : kin;
    }
  }
  for (int m = 1; m < LPR; m <<= 1) {
    S += __shfl_xor(S, m, 64);
    inmask |= (unsigned)__shfl_xor((int)inmask, m, 64);
    kin = min(kin, __shfl_xor(kin, m, 64));
  }
  // F pass on a zero guess: S is exactly the row's product with the C values -- f - S is what the residual that
  // follows needs from those columns (BoomerAMG::cycle)
  // (f is read again here rather than kept in two registers through the kernel: 66 -> 64 VGPRs = 8 waves per SIMD)
  if (tout && rowsel && sub == 0 && i >= t_from) tout[i] = f[i] - S;
  // the sweep: a chunk = 8 rows = 8 * LPR consecutive lanes (tiles start on a multiple of 8 rows)
  const int lane = tid & 63;
  const int g = (lane / LPR) & 7;
  const int gbase = lane & ~(8 * LPR - 1);
  // Three cases in which the 16-step sweep below would only multiply structural zeros are taken out of it, each by a
  // branch that is uniform in the wave (ballots) or in the tile (zero_tile), so no lane diverges inside a sweep.  None
  // changes the order or the operands of an addition that reaches a result: what is left out are terms c * 0 and
  // 0 * u (for finite data at most the sign of an exact zero can differ).  -DMI_GS_SWEEP_PATHS=<bits> selects them
  // (1: zero-guess tiles, 2: diagonal chunks, 4: idle waves; 0 = every wave runs the general sweep) for A/B timing.
#ifndef MI_GS_SWEEP_PATHS
#define MI_GS_SWEEP_PATHS 7
#endif
  // * no row of the wave is selected (LPR * nr <= 192, the last tile of a pass, a tile of the other colour's rows):
  //   every lane has wd == 0, the sweep would hand every row its old value back
  const bool wave_idle = (MI_GS_SWEEP_PATHS & 4) && __ballot(rowsel) == 0;
  // * no row of the wave has an in-chunk entry besides its diagonal (the C rows of a level on which all connections
  //   are strong: PMIS C points are an independent set): no row reads another row's new value, so every row's step is
  //   u += wd * (rhs - (S + a_ii u)) at once, the expression the sweep evaluates for row g at step g
  const bool wave_diag = (MI_GS_SWEEP_PATHS & 2) && __ballot((inmask & ~(1u << g)) != 0u) == 0;
  // * every row of the tile starts from 0 (first sweep on a zero guess: the whole C pass, the F pass but for the tile
  //   that straddles zero_from): the chunk's values need not be fetched, and the forward sum over the columns not yet
  //   swept is a sum of products with 0
  const bool zero_tile = (MI_GS_SWEEP_PATHS & 1) && r0 >= zero_from;
  if (wave_idle || (MI_ABLATE & 8)) {
    // nothing to sweep: myu is the row's value
  } else if (wave_diag) {
    const bool has = (inmask >> g) & 1u;
    const double cd = has ? buf[has ? kin : 0] : 0.0;
    if (fwd) myu = myu + (myrhs - (S + cd * myu)) * wd;  // unselected rows: wd == 0
    if (bwd) myu = myu + (myrhs - (S + cd * myu)) * wd;
    // C-row hand-over: a row whose out-of-chunk columns this pass leaves alone has its product with the new vector here
    if (wout && rowsel && sub == 0) wout[i] = S + cd * myu;
  } else {
    double crow[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const bool has = (inmask >> j) & 1u;
      const int pos = kin + __popc(inmask & ((1u << j) - 1u));
      crow[j] = has ? buf[has ? pos : 0] : 0.0;
    }
    double uc[8];
    gs_tile_sweep(crow, uc, myu, S, myrhs, wd, g, gbase, LPR, fwd, bwd, zero_tile);
  }
  if (rl < nr && sub == 0) u_new[i] = myu;
#undef UOLD
}

// ---------------------------------------------------------------------------
// gs_tile_k for the NV components of a multivector in one pass over the operator (no C-row hand-over: `wout` stays
// with the single-vector kernel).  As in spmv_stream_xc_mv, what does not depend on the vector is requested once per
// tile -- descriptor, column list, column words, values (held as doubles), the rows' marks, divisors and entry ranges,
// and the `code` words in LDS -- and the gather -> x cache -> products -> out-of-chunk sums -> 8x8 sweep -> store part
// of gs_tile_k runs once per component, on that kernel's operands in that kernel's order, through the same
// gs_tile_sweep and the same three uniform branches.  The value dictionary shares its LDS bytes with `code`, so it is
// looked up once, before the first component's code words are written.
// Holding the values through the component loop costs registers this kernel cannot have at gs_tile_k's 8 waves per
// SIMD; it is built without that bound (profiles/mv_batch_resources.txt has the figures: no scratch).
// ---------------------------------------------------------------------------
template <int NV, bool VAL8, int BLOCK, bool VAL4 = false>
__global__ __launch_bounds__(BLOCK) void gs_tile_mv_k(int blk0, int nblk, const int *__restrict__ tdesc,
                                                      const int *__restrict__ ia, const double *__restrict__ av,
                                                      const int *__restrict__ ucols,
                                                      const unsigned short *__restrict__ lcol,
                                                      const signed char *__restrict__ cf, int points,
                                                      const double *__restrict__ dd, const double *__restrict__ f_all,
                                                      const double *__restrict__ offc_all,
                                                      const double *__restrict__ u_lo_all,
                                                      const double *__restrict__ u_hi_all, int split,
                                                      double *__restrict__ u_new_all, int fwd, int bwd, double w,
                                                      int row_begin, int row_end, int zero_from,
                                                      double *__restrict__ tout_all, int t_from, GsMultiStrides st,
                                                      const unsigned char *__restrict__ vidx,
                                                      const double *__restrict__ vlut) {
#define UOLD(j) (((j) < split ? u_lo : u_hi)[(j)])
  static_assert(NV >= 2 && NV <= 4, "2, 3 or 4 components per pass");
  constexpr int TILE = 8 * BLOCK;
  __shared__ double buf[TILE];
  __shared__ __attribute__((aligned(8))) unsigned char code_bytes[TILE * sizeof(unsigned short)];
  static_assert(TILE * sizeof(unsigned short) >= 256 * sizeof(double), "the value table must fit the code array");
  unsigned short *code = reinterpret_cast<unsigned short *>(code_bytes);
  double *slut = reinterpret_cast<double *>(code_bytes);
  if ((int)blockIdx.x >= nblk) return;
  const int blk = blk0 + blockIdx.x;
  const int tid = threadIdx.x;
  double lutv = 0.0;
  if (VAL8 && tid < 256) lutv = vlut[tid];
  const int4 d0 = reinterpret_cast<const int4 *>(tdesc)[2 * blk];
  const int4 d1 = reinterpret_cast<const int4 *>(tdesc)[2 * blk + 1];
  const int r0 = d0.x, r1 = d0.y, len = d0.w, u0 = d1.x, nu = d1.y;
  const long long base64 = ((long long)d1.z << 32) | (long long)(unsigned)d0.z;
  const bool all_zero = zero_from <= 0;
  constexpr int NU = TILE / BLOCK;
  int ucid[NU];
#pragma unroll
  for (int q = 0; q < NU; q++) {
    const int k = tid + q * BLOCK;
    ucid[q] = 0;
    if (!all_zero && k < nu) ucid[q] = LIST_LOAD(ucols + u0 + k);
  }
  const long long base_al64 = base64 & ~1LL;
  const int base = (int)(base64 - base_al64);  // tile-local from here on
  const int end = base + len;
  const int cnt = end;
  const unsigned ia_off = (unsigned)base_al64;
  const float *av4 = reinterpret_cast<const float *>(av) + base_al64;
  av += base_al64;
  lcol += base_al64;
  if (VAL8) vidx += base_al64;
  constexpr int NIT = TILE / (2 * BLOCK);
  d2_t vv[NIT];  // the values: as loaded (fp64), or from the first barrier on (dictionary, fp32)
  f2_t vf[NIT];
  unsigned cw[NIT], vw[NIT];
#pragma unroll
  for (int it = 0; it < NIT; it++) {
    const int k = 2 * tid + it * 2 * BLOCK;
    cw[it] = 0;
    vw[it] = 0;
    vv[it] = d2_t{0.0, 0.0};
    if (k < cnt) {
      if (VAL8)
        vw[it] = STREAM_LOAD(reinterpret_cast<const unsigned short *>(vidx + k));
      else if (VAL4)
        vf[it] = STREAM_LOAD(reinterpret_cast<const f2_t *>(av4 + k));
      else
        vv[it] = STREAM_LOAD(reinterpret_cast<const d2_t *>(av + k));
      cw[it] = STREAM_LOAD(reinterpret_cast<const unsigned *>(lcol + k));
    }
  }
  // the two-batch gather of the fp64 form, as in gs_tile_k
  constexpr int GB = (VAL8 || VAL4) ? NU : NU / 2;
  // per row, once for all components: is it swept, its divisor and its entry range
  const int nr = r1 - r0;
  const int LPR = nr <= BLOCK / 8 ? 8 : nr <= BLOCK / 4 ? 4 : nr <= BLOCK / 2 ? 2 : 1;
  const int rl = tid / LPR, sub = tid % LPR;
  const int i = r0 + rl;
  double wd = 0.0;
  bool rowsel = false;
  int s0 = 0, s1 = 0;
  if (rl < nr) {
    const int mark = (points != 0 && cf != nullptr) ? (int)cf[i] : points;
    rowsel = (mark == points) && i >= row_begin && i < row_end;
    if (rowsel) {
      const double myd = dd[i];
      if (myd != 0.0) wd = w / myd;
      s0 = (int)((unsigned)ia[i] - ia_off);
      s1 = (int)((unsigned)ia[i + 1] - ia_off);
    }
  }
  const int lane = tid & 63;
  const int g = (lane / LPR) & 7;
  const int gbase = lane & ~(8 * LPR - 1);
  const bool zero_tile = (MI_GS_SWEEP_PATHS & 1) && r0 >= zero_from;
  if (VAL8 && tid < 256) slut[tid] = lutv;
#pragma unroll 1
  for (int c = 0; c < NV; c++) {
    const double *u_lo = u_lo_all + c * st.u_lo;
    const double *u_hi = u_hi_all + c * st.u_hi;
    const double *f = f_all + c * st.f;
    const double *offc = offc_all ? offc_all + c * st.offc : nullptr;
    double *u_new = u_new_all + c * st.out;
    double *tout = tout_all ? tout_all + c * st.tout : nullptr;
    double xv[GB];
    if (!all_zero) {
#pragma unroll
      for (int q = 0; q < GB; q++) {
        const int j = (ucid[q] >= zero_from) ? 0 : ucid[q];
        xv[q] = UOLD(j);
      }
    }
    double myu = 0.0, myrhs = 0.0;
    if (rl < nr) {
      myu = (i >= zero_from) ? 0.0 : UOLD(i);
      if (rowsel) {
        myrhs = f[i];
        if (offc) myrhs -= offc[i];
      }
    }
    if (!all_zero) {
#pragma unroll
      for (int q = 0; q < GB; q++) {
        const int k = tid + q * BLOCK;
        if (k < nu) buf[k] = (ucid[q] >= zero_from) ? 0.0 : xv[q];
      }
      if (GB < NU && nu > GB * BLOCK) {  // (uniform) more unique columns than the first batch holds
#pragma unroll
        for (int q = GB; q < NU; q++) {
          const int j = (ucid[q] >= zero_from) ? 0 : ucid[q];
          xv[q - GB] = UOLD(j);
        }
#pragma unroll
        for (int q = GB; q < NU; q++) {
          const int k = tid + q * BLOCK;
          if (k < nu) buf[k] = (ucid[q] >= zero_from) ? 0.0 : xv[q - GB];
        }
      }
    }
    __syncthreads();
    if (c == 0 && (VAL8 || VAL4)) {
#pragma unroll
      for (int it = 0; it < NIT; it++) {
        if (VAL8) {
          vv[it].x = slut[vw[it] & 0xffu];
          vv[it].y = slut[vw[it] >> 8];
        } else {
          vv[it].x = (double)vf[it].x;
          vv[it].y = (double)vf[it].y;
        }
      }
    }
    d2_t pv[NIT];
#pragma unroll
    for (int it = 0; it < NIT; it++) {
      const int k = 2 * tid + it * 2 * BLOCK;
      pv[it] = d2_t{0.0, 0.0};
      if (k < cnt) {
        const bool ok0 = (k >= base);
        const bool ok1 = (k + 1 < end);
        const unsigned c0 = cw[it] & 0xffffu, c1 = cw[it] >> 16;
        // out-of-chunk: product with the snapshot value; in-chunk: the coefficient itself
        const double x0 = all_zero ? 0.0 : buf[c0 & XC_ID_MASK], x1 = all_zero ? 0.0 : buf[c1 & XC_ID_MASK];
        pv[it].x = ok0 ? ((c0 & XC_INCH) ? vv[it].x : vv[it].x * x0) : 0.0;
        pv[it].y = ok1 ? ((c1 & XC_INCH) ? vv[it].y : vv[it].y * x1) : 0.0;
      }
    }
    __syncthreads();  // every x-cache read (and, c == 0, every dictionary lookup) is done
#pragma unroll
    for (int it = 0; it < NIT; it++) {
      const int k = 2 * tid + it * 2 * BLOCK;
      if (k < cnt) {
        buf[k] = pv[it].x;
        buf[k + 1] = pv[it].y;
        if (c == 0) {
          code[k] = (unsigned short)(cw[it] & 0xffffu);
          code[k + 1] = (unsigned short)(cw[it] >> 16);
        }
      }
    }
    __syncthreads();
    double S = 0.0;
    unsigned inmask = 0;
    int kin = TILE;
    if (rowsel) {
      for (int k = s0 + sub; k < s1; k += LPR) {
        const unsigned cc = code[k];
        const double v = buf[k];
        const bool in = (cc & XC_INCH) != 0;
        S += in ? 0.0 : v;
        inmask |= in ? (1u << ((cc >> XC_OFF_SHIFT) & 7)) : 0u;
        kin = in ? min(kin, k) : kin;
      }
    }
    for (int m = 1; m < LPR; m <<= 1) {
      S += __shfl_xor(S, m, 64);
      inmask |= (unsigned)__shfl_xor((int)inmask, m, 64);
      kin = min(kin, __shfl_xor(kin, m, 64));
    }
    if (tout && rowsel && sub == 0 && i >= t_from) tout[i] = f[i] - S;
    const bool wave_idle = (MI_GS_SWEEP_PATHS & 4) && __ballot(rowsel) == 0;
    const bool wave_diag = (MI_GS_SWEEP_PATHS & 2) && __ballot((inmask & ~(1u << g)) != 0u) == 0;
    if (wave_idle) {
      // nothing to sweep: myu is the row's value
    } else if (wave_diag) {
      const bool has = (inmask >> g) & 1u;
      const double cd = has ? buf[has ? kin : 0] : 0.0;
      if (fwd) myu = myu + (myrhs - (S + cd * myu)) * wd;  // unselected rows: wd == 0
      if (bwd) myu = myu + (myrhs - (S + cd * myu)) * wd;
    } else {
      double crow[8];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const bool has = (inmask >> j) & 1u;
        const int pos = kin + __popc(inmask & ((1u << j) - 1u));
        crow[j] = has ? buf[has ? pos : 0] : 0.0;
      }
      double uc[8];
      gs_tile_sweep(crow, uc, myu, S, myrhs, wd, g, gbase, LPR, fwd, bwd, zero_tile);
    }
    if (rl < nr && sub == 0) u_new[i] = myu;
    if (c + 1 < NV) __syncthreads();  // the sums and coefficients are read: the array becomes the next x cache
  }
#undef UOLD
}

// ---------------------------------------------------------------------------
// BLAS-1
// ---------------------------------------------------------------------------
// Second stage of the two-stage reductions inside the first-stage kernel: every block leaves its partial sum, takes a
// ticket, and the block that draws the last one adds the partials up -- in a fixed order
// (thread t takes partials t, t + 256, ...; wave shuffles; (w0 + w1) + (w2 + w3)), so the result does not depend on
// which block comes last and equals the two-launch form bit for bit.  One launch per inner product instead of two
// (a GMRES solve of m steps issues m(m+1)/2 + 2m + 3 of them).  The ticket counter is reset by the last block;
// reductions are serialised on the library stream, so one counter serves them all.
// Ordering without a release fence: an agent-scope release would write this XCD's L2 back for EVERY block (the
// vector the kernel has just stored included: measured +18 % on the fused Gram-Schmidt step).  Only the partial has
// to be visible before the ticket, and both are agent-scope atomics executed at the device's coherence point: the
// partial is stored by an exchange whose RETURN the lane waits for (s_waitcnt vmcnt(0): the operation has been
// performed) before it draws the ticket; the last block reads the partials with agent-scope atomic loads after its
// own ticket came back.
__device__ __forceinline__ void finish_reduction(double block_sum, double *__restrict__ partials,
                                                 unsigned *__restrict__ ticket, double *__restrict__ out, double *ws) {
  __shared__ unsigned s_last;
  const int tid = threadIdx.x;
  if (tid == 0) {
    unsigned long long *slot = reinterpret_cast<unsigned long long *>(partials + blockIdx.x);
    const unsigned long long old =
        __hip_atomic_exchange(slot, (unsigned long long)__double_as_longlong(block_sum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::"v"(old) : "memory");
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (t == gridDim.x - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  const int nb = (int)gridDim.x;
  double s = 0.0;
  for (int i = tid; i < nb; i += 256) s += __hip_atomic_load(partials + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  s = wave_sum(s);
  __syncthreads();  // ws is reused
  if ((tid & 63) == 0) ws[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    out[0] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(256) void dot_partial_k(const double *__restrict__ x, const double *__restrict__ y, int n,
                                                     double *__restrict__ partials, unsigned *__restrict__ ticket,
                                                     double *__restrict__ out) {
  __shared__ double ws[4];
  const int tid = threadIdx.x;
  double s = 0.0;
  const long long stride = (long long)gridDim.x * 512;
  long long i = ((long long)blockIdx.x * 256 + tid) * 2;
  for (; i + 1 < n; i += stride) {
    const d2_t a = nt_load(reinterpret_cast<const d2_t *>(x + i));
    const d2_t b = nt_load(reinterpret_cast<const d2_t *>(y + i));
    s += a.x * b.x + a.y * b.y;
  }
  if (i < n) s += x[i] * y[i];
  s = wave_sum(s);
  if ((tid & 63) == 0) ws[tid >> 6] = s;
  __syncthreads();
  finish_reduction((ws[0] + ws[1]) + (ws[2] + ws[3]), partials, ticket, out, ws);
}

// fused modified-Gram-Schmidt step: y += a*xa (a = scale * *alpha_dev), then the
// partial dot <xd, y_new> (xd == nullptr: <y_new, y_new>) in the same pass.
// Same per-thread accumulation pattern as dot_partial_k, so the result is
// bit-identical to axpy followed by dot.
__global__ __launch_bounds__(256) void axpy_dot_partial_k(const double *__restrict__ alpha_dev, double scale,
                                                          const double *__restrict__ xa, double *__restrict__ y,
                                                          const double *__restrict__ xd, int n,
                                                          double *__restrict__ partials, unsigned *__restrict__ ticket,
                                                          double *__restrict__ out) {
  __shared__ double ws[4];
  const int tid = threadIdx.x;
  const double a = scale * alpha_dev[0];
  double s = 0.0;
  const long long stride = (long long)gridDim.x * 512;
  long long i = ((long long)blockIdx.x * 256 + tid) * 2;
  for (; i + 1 < n; i += stride) {
    // every operand is streamed exactly once: non-temporal accesses keep them out of L2's way
    const d2_t xv = nt_load(reinterpret_cast<const d2_t *>(xa + i));
    d2_t yv = nt_load(reinterpret_cast<const d2_t *>(y + i));
    yv.x += a * xv.x;
    yv.y += a * xv.y;
    __builtin_nontemporal_store(yv, reinterpret_cast<d2_t *>(y + i));
    d2_t dv = yv;
    if (xd) dv = nt_load(reinterpret_cast<const d2_t *>(xd + i));
    s += dv.x * yv.x + dv.y * yv.y;
  }
  if (i < n) {
    const double yn = y[i] + a * xa[i];
    y[i] = yn;
    s += (xd ? xd[i] : yn) * yn;
  }
  s = wave_sum(s);
  if ((tid & 63) == 0) ws[tid >> 6] = s;
  __syncthreads();
  finish_reduction((ws[0] + ws[1]) + (ws[2] + ws[3]), partials, ticket, out, ws);
}



// ---- block Gram-Schmidt pieces of COGMRES: up to MASS_NV inner products off one vector in one pass, and the
// matching block update.  The per-thread accumulation pattern is dot_partial_k's, so every result equals the
// separate dot's bit for bit; the update adds the terms in ascending j like repeated axpys.
template <class T>
struct MassPtrs {
  const T *p[MASS_NV];
};

template <class T>
__global__ __launch_bounds__(256) void mass_dot_partial_k(MassPtrs<T> P, int m, const double *__restrict__ w, int n,
                                                          double *__restrict__ partials) {
  __shared__ double ws[MASS_NV][4];
  const int tid = threadIdx.x;
  double acc[MASS_NV];
#pragma unroll
  for (int j = 0; j < MASS_NV; j++) acc[j] = 0.0;
  const long long stride = (long long)gridDim.x * 512;
  long long i = ((long long)blockIdx.x * 256 + tid) * 2;
  for (; i + 1 < n; i += stride) {
    const double2 b = *reinterpret_cast<const double2 *>(w + i);
#pragma unroll
    for (int j = 0; j < MASS_NV; j++)
      if (j < m) {
        const d2_t a = load_pair<false>(P.p[j] + i);
        acc[j] += a.x * b.x + a.y * b.y;
      }
  }
  if (i < n) {
#pragma unroll
    for (int j = 0; j < MASS_NV; j++)
      if (j < m) acc[j] += (double)P.p[j][i] * w[i];
  }
#pragma unroll
  for (int j = 0; j < MASS_NV; j++) {
    const double v = wave_sum(acc[j]);
    if ((tid & 63) == 0) ws[j][tid >> 6] = v;
  }
  __syncthreads();
  if (tid < m) partials[(size_t)tid * RED_MAX_BLOCKS + blockIdx.x] = (ws[tid][0] + ws[tid][1]) + (ws[tid][2] + ws[tid][3]);
}

__global__ __launch_bounds__(256) void reduce_final_multi_k(const double *__restrict__ partials, int nb,
                                                            double *__restrict__ out) {
  __shared__ double ws[4];
  const int tid = threadIdx.x;
  const double *mine = partials + (size_t)blockIdx.x * RED_MAX_BLOCKS;
  double s = 0.0;
  for (int i = tid; i < nb; i += 256) s += mine[i];
  s = wave_sum(s);
  if ((tid & 63) == 0) ws[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) out[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// w += sum_j (scale * coef[j]) * p_j, terms added in ascending j
template <class T>
__global__ __launch_bounds__(256) void mass_axpy_k(MassPtrs<T> P, int m, const double *__restrict__ coef, double scale,
                                                   double *__restrict__ w, int n) {
  double c[MASS_NV];
#pragma unroll
  for (int j = 0; j < MASS_NV; j++) c[j] = (j < m) ? scale * coef[j] : 0.0;
  const long long stride = (long long)gridDim.x * 512;
  long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 2;
  for (; i + 1 < n; i += stride) {
    double2 wv = *reinterpret_cast<double2 *>(w + i);
#pragma unroll
    for (int j = 0; j < MASS_NV; j++)
      if (j < m) {
        const d2_t a = load_pair<false>(P.p[j] + i);
        wv.x += c[j] * a.x;
        wv.y += c[j] * a.y;
      }
    *reinterpret_cast<double2 *>(w + i) = wv;
  }
  if (i < n) {
    double v = w[i];
#pragma unroll
    for (int j = 0; j < MASS_NV; j++)
      if (j < m) v += c[j] * (double)P.p[j][i];
    w[i] = v;
  }
}

// ---- blocked modified Gram-Schmidt (single-rank GMRES): one pass of the scheme of DESIGN.md section 5.
// finish_reduction for NOUT sums per block: partial o of block b lies at partials[o * gridDim.x + b].  Lanes 0 .. NOUT-1
// (one wave) leave the block's partials by exchanges whose returns the wave waits for, then lane 0 draws the ticket;
// the last block adds every output up in finish_reduction's fixed order.  ws: NOUT x 4 wave sums on entry.
template <int NOUT>
__device__ __forceinline__ void finish_reduction_multi(double (*ws)[4], double *__restrict__ partials,
                                                       unsigned *__restrict__ ticket, double *__restrict__ out,
                                                       double *__restrict__ out_last) {
  static_assert(NOUT <= 64, "the partials are left by one wave");
  __shared__ unsigned s_last;
  const int tid = threadIdx.x;
  const int nb = (int)gridDim.x;
  if (tid < NOUT) {
    const double block_sum = (ws[tid][0] + ws[tid][1]) + (ws[tid][2] + ws[tid][3]);
    unsigned long long *slot = reinterpret_cast<unsigned long long *>(partials + (size_t)tid * nb + blockIdx.x);
    const unsigned long long old =
        __hip_atomic_exchange(slot, (unsigned long long)__double_as_longlong(block_sum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::"v"(old) : "memory");
  }
  if (tid == 0) {
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (t == gridDim.x - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
#pragma unroll
  for (int o = 0; o < NOUT; o++) {
    double s = 0.0;
    for (int i = tid; i < nb; i += 256)
      s += __hip_atomic_load(partials + (size_t)o * nb + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s = wave_sum(s);
    if ((tid & 63) == 0) ws[o][tid >> 6] = s;  // the block sums were read before the barrier above
  }
  __syncthreads();
  if (tid < NOUT) {
    const double v = (ws[tid][0] + ws[tid][1]) + (ws[tid][2] + ws[tid][3]);
    out[tid] = v;
    if (out_last && tid == NOUT - 1) out_last[0] = v;
  }
  if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int B, class T>
struct MgsPtrs {
  const T *prev[B];
  const T *next[B];
};

// Prologue (every thread, at most B(B-1)/2 FMAs): the MGS coefficients of the block `prev` from the raw inner products
// c_prev[j] = <prev_j, w> (all taken against the same w) and the block's raw Gram rows -- row j = B + 1 doubles,
// <prev_k, w_j> for k < j and, last, ||w_j||^2 of the vector w_j that became prev_j = w_j / ||w_j|| --
//   h_j = c_j - sum_{k < j} h_k g_jk,  g_jk = <prev_k, w_j> / sqrt(||w_j||^2)  (0 where the norm is not positive).
// Block 0 stores them at h_out.  Body: w -= sum_j h_j prev_j (ascending j), and off the new w
//   !LAST: out[j] = <next_j, w>, j < m_next (the raw c of the next block);
//   LAST:  out[j] = <prev_j, w>, j < m_prev, out[B] = ||w||^2 (also at out_norm): the raw Gram row of w.
// Streaming as axpy_dot_partial_k: every operand once, non-temporal.  Outputs beyond the counts are 0.
template <int B, bool LAST, class T>
__global__ __launch_bounds__(256) void mgs_block_pass_k(MgsPtrs<B, T> P, int m_prev, int m_next,
                                                        const double *__restrict__ c_prev,
                                                        const double *__restrict__ gram_prev, double *__restrict__ h_out,
                                                        double *__restrict__ w, int n, double *__restrict__ partials,
                                                        unsigned *__restrict__ ticket, double *__restrict__ out,
                                                        double *__restrict__ out_norm) {
  __shared__ double ws[B + 1][4];
  const int tid = threadIdx.x;
  double a[B];  // -h_j
#pragma unroll
  for (int j = 0; j < B; j++) {
    a[j] = 0.0;
    if (j < m_prev) {
      const double nrm = j > 0 ? gram_prev[j * (B + 1) + B] : 0.0;  // row 0 has no entries: never read
      const double inv = nrm > 0.0 ? 1.0 / sqrt(nrm) : 0.0;
      double h = c_prev[j];
#pragma unroll
      for (int k = 0; k < j; k++) h += a[k] * (gram_prev[j * (B + 1) + k] * inv);
      a[j] = -h;
      if (blockIdx.x == 0 && tid == 0) h_out[j] = h;
    }
  }
  double acc[B + 1];
#pragma unroll
  for (int j = 0; j <= B; j++) acc[j] = 0.0;
  const long long stride = (long long)gridDim.x * 512;
  long long i = ((long long)blockIdx.x * 256 + tid) * 2;
  for (; i + 1 < n; i += stride) {
    // all loads first, then the arithmetic: the branches on the (uniform) counts hold no wait between two loads
    d2_t wv = nt_load(reinterpret_cast<const d2_t *>(w + i));
    d2_t pv[B], qv[B];
#pragma unroll
    for (int j = 0; j < B; j++)
      if (j < m_prev) pv[j] = load_pair<true>(P.prev[j] + i);
    if (!LAST) {
#pragma unroll
      for (int j = 0; j < B; j++)
        if (j < m_next) qv[j] = load_pair<true>(P.next[j] + i);
    }
#pragma unroll
    for (int j = 0; j < B; j++)
      if (j < m_prev) {
        wv.x += a[j] * pv[j].x;
        wv.y += a[j] * pv[j].y;
      }
    if (m_prev > 0) __builtin_nontemporal_store(wv, reinterpret_cast<d2_t *>(w + i));
    if (LAST) {
#pragma unroll
      for (int j = 0; j < B; j++)
        if (j < m_prev) acc[j] += pv[j].x * wv.x + pv[j].y * wv.y;
      acc[B] += wv.x * wv.x + wv.y * wv.y;
    } else {
#pragma unroll
      for (int j = 0; j < B; j++)
        if (j < m_next) acc[j] += qv[j].x * wv.x + qv[j].y * wv.y;
    }
  }
  if (i < n) {
    double v = w[i];
#pragma unroll
    for (int j = 0; j < B; j++)
      if (j < m_prev) v += a[j] * (double)P.prev[j][i];
    if (m_prev > 0) w[i] = v;
    if (LAST) {
#pragma unroll
      for (int j = 0; j < B; j++)
        if (j < m_prev) acc[j] += (double)P.prev[j][i] * v;
      acc[B] += v * v;
    } else {
#pragma unroll
      for (int j = 0; j < B; j++)
        if (j < m_next) acc[j] += (double)P.next[j][i] * v;
    }
  }
#pragma unroll
  for (int j = 0; j <= B; j++) {
    const double v = wave_sum(acc[j]);
    if ((tid & 63) == 0) ws[j][tid >> 6] = v;
  }
  __syncthreads();
  finish_reduction_multi<B + 1>(ws, partials, ticket, out, LAST ? out_norm : nullptr);
}

// w = c_0 p_0 (INIT) or w += c_0 p_0, then += c_1 p_1, ... in this order: the chain copy / scale / axpy / axpy ... of the
// GMRES solution update in one pass over up to MASS_NV vectors (same operations per element in the same order)
struct MassCoef {
  double c[MASS_NV];
};
template <bool INIT, class T>
__global__ __launch_bounds__(256) void lin_comb_k(MassPtrs<T> P, int m, MassCoef C, double *__restrict__ w, int n) {
  const long long stride = (long long)gridDim.x * 512;
  long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 2;
  for (; i + 1 < n; i += stride) {
    double2 wv;
    if (INIT) {
      const d2_t a = load_pair<true>(P.p[0] + i);
      wv.x = C.c[0] * a.x;
      wv.y = C.c[0] * a.y;
    } else {
      wv = *reinterpret_cast<double2 *>(w + i);
    }
#pragma unroll
    for (int j = INIT ? 1 : 0; j < MASS_NV; j++)
      if (j < m) {
        const d2_t a = load_pair<true>(P.p[j] + i);
        wv.x += C.c[j] * a.x;
        wv.y += C.c[j] * a.y;
      }
    *reinterpret_cast<double2 *>(w + i) = wv;
  }
  if (i < n) {
    double v = INIT ? C.c[0] * (double)P.p[0][i] : w[i];
#pragma unroll
    for (int j = INIT ? 1 : 0; j < MASS_NV; j++)
      if (j < m) v += C.c[j] * (double)P.p[j][i];
    w[i] = v;
  }
}

// y += (scale * (alpha_dev ? *alpha_dev : 1)) * x
__global__ __launch_bounds__(256) void axpy_k(const double *__restrict__ alpha_dev, double scale,
                                              const double *__restrict__ x, double *__restrict__ y, int n) {
  const double a = scale * (alpha_dev ? alpha_dev[0] : 1.0);
  const long long stride = (long long)gridDim.x * 512;
  long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 2;
  for (; i + 1 < n; i += stride) {
    const double2 xv = *reinterpret_cast<const double2 *>(x + i);
    double2 yv = *reinterpret_cast<double2 *>(y + i);
    yv.x += a * xv.x;
    yv.y += a * xv.y;
    *reinterpret_cast<double2 *>(y + i) = yv;
  }
  if (i < n) y[i] += a * x[i];
}

// MODE 0: x *= scale ; MODE 1: x *= 1/sqrt(*sumsq_dev) when *sumsq_dev > 0
template <int MODE>
__global__ __launch_bounds__(256) void scale_k(const double *__restrict__ sumsq_dev, double scale,
                                               double *__restrict__ x, int n) {
  double a = scale;
  if (MODE == 1) {
    const double t = sumsq_dev[0];
    if (!(t > 0.0)) return;
    a = 1.0 / sqrt(t);
  }
  const long long stride = (long long)gridDim.x * 512;
  long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 2;
  for (; i + 1 < n; i += stride) {
    double2 v = *reinterpret_cast<double2 *>(x + i);
    v.x *= a;
    v.y *= a;
    *reinterpret_cast<double2 *>(x + i) = v;
  }
  if (i < n) x[i] *= a;
}

__global__ __launch_bounds__(256) void fill_k(double *__restrict__ x, int n, double v) {
  const long long stride = (long long)gridDim.x * 512;
  long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 2;
  for (; i + 1 < n; i += stride) *reinterpret_cast<double2 *>(x + i) = make_double2(v, v);
  if (i < n) x[i] = v;
}

__global__ __launch_bounds__(256) void gather_k(const double *__restrict__ x, const int *__restrict__ map,
                                                double *__restrict__ out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = x[map[i]];
}

__global__ __launch_bounds__(256) void gather2_k(const double *__restrict__ lo, const double *__restrict__ hi, int split,
                                                 const int *__restrict__ map, double *__restrict__ out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int j = map[i];
    out[i] = (j < split ? lo : hi)[j];
  }
}

template <int ADD>
__global__ __launch_bounds__(256) void scatter_k(double *__restrict__ x, const int *__restrict__ idx,
                                                 const double *__restrict__ vals, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    if (ADD)
      x[idx[i]] += vals[i];  // caller guarantees unique indices
    else
      x[idx[i]] = vals[i];
  }
}

// u = M f for the coarsest level (relax type 9: M = dense inverse, n small)
// two-stage Gauss-Seidel (relax types 11 / 12): z = r / d, u += z; then z_out = (L z_in) / d with L the strictly
// lower part of the block, u += sign * z_out.  One lane per row: these smoothers are not on the benchmark path.
__global__ __launch_bounds__(256) void two_stage_first_k(int n, const double *__restrict__ r, const double *__restrict__ d,
                                                         double *__restrict__ z, double *__restrict__ u) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double zi = (d[i] != 0.0) ? r[i] / d[i] : 0.0;
  z[i] = zi;
  u[i] += zi;
}
template <class VT>
__global__ __launch_bounds__(256) void two_stage_lower_k(int n, const int *__restrict__ ia, const int *__restrict__ ja,
                                                         const VT *__restrict__ a, const double *__restrict__ d,
                                                         const double *__restrict__ zin, double sign,
                                                         double *__restrict__ zout, double *__restrict__ u) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int k = ia[i]; k < ia[i + 1]; k++) {
    const int j = ja[k];
    if (j < i) s += (double)a[k] * zin[j];
  }
  const double zi = (d[i] != 0.0) ? s / d[i] : 0.0;
  zout[i] = zi;
  u[i] += sign * zi;
}

__global__ __launch_bounds__(256) void dense_matvec_k(const double *__restrict__ M, const double *__restrict__ f,
                                                      double *__restrict__ u, int n, int m) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int j = 0; j < m; j++) s += M[(size_t)i * m + j] * f[j];
  u[i] = s;
}

// u[i] = sum_j Mt[j*n + i] * f[j]: a workgroup of 1024 lanes owns 16 consecutive rows i (lane & 15) and splits the
// columns j over its 64 lane groups (128-byte reads of Mt's rows; ~n/64 loads per lane, all independent: the kernel
// is a latency chain, not a stream -- 47 workgroups and 12 loads per lane for the 753-row tail of the 512^3
// hierarchy); the 64 partial sums of a row are added in group order out of LDS -- a fixed order, the result does
// not depend on scheduling
__global__ __launch_bounds__(1024) void dense_matvec_t_k(const double *__restrict__ Mt, const double *__restrict__ f,
                                                         double *__restrict__ u, int n) {
  __shared__ double part[64][17];
  const int r = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + r;
  double s = 0.0;
  if (i < n)
    for (int j = g; j < n; j += 64) s += Mt[(size_t)j * (size_t)n + i] * f[j];
  part[g][r] = s;
  __syncthreads();
  if (g == 0 && i < n) {
    double t = part[0][r];
#pragma unroll 8
    for (int w = 1; w < 64; w++) t += part[w][r];
    u[i] = t;
  }
}

// peer-store neighbour exchange: see kernels.hpp.  blockIdx.x walks the transfers' workgroups in order.
__global__ __launch_bounds__(1024) void ipc_exchange_k(IpcBatch B, unsigned long long spin_limit, int *error_flag) {
  __shared__ int s_ok;
  int blk = (int)blockIdx.x, ti = 0;
  while (ti < B.n && blk >= B.t[ti].nblocks) blk -= B.t[ti++].nblocks;
  if (ti >= B.n) return;
  const IpcTransfer &T = B.t[ti];
  const int tid = threadIdx.x;
  if (tid == 0) {
    int ok = 1;
    const unsigned long long t0 = wall_clock64();
    // a rank whose flag is already up does not wait the full bound again (a dead transport would otherwise
    // cost bound x exchanges before the end-of-solve check sees it): 1 ms per wait from then on
    const unsigned long long limit = __hip_atomic_load(error_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? min(spin_limit, 100000ull) : spin_limit;
    while (__hip_atomic_load(T.wait_word, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < T.wait_value) {
      if (wall_clock64() - t0 > limit) {  // the peer never arrived: say so and fall through (no hang)
        ok = 0;
        atomicExch(error_flag, 1);
        break;
      }
      __builtin_amdgcn_s_sleep(8);
    }
    s_ok = ok;
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // what the peer stored before its flag is visible
  if (s_ok) {
    const unsigned long long n16 = T.bytes / 16;
    const bool al = ((((unsigned long long)T.src) | ((unsigned long long)T.dst)) & 15ull) == 0;
    const unsigned long long stride = (unsigned long long)T.nblocks * 1024ull;
    if (al) {
      const d2_t *sp = reinterpret_cast<const d2_t *>(T.src);
      d2_t *dp = reinterpret_cast<d2_t *>(T.dst);
      for (unsigned long long i = (unsigned long long)blk * 1024ull + tid; i < n16; i += stride) dp[i] = sp[i];
      const unsigned char *sb = reinterpret_cast<const unsigned char *>(T.src);
      unsigned char *db = reinterpret_cast<unsigned char *>(T.dst);
      for (unsigned long long i = n16 * 16 + (unsigned long long)blk * 1024ull + tid; i < T.bytes; i += stride) db[i] = sb[i];
    } else {
      const unsigned char *sb = reinterpret_cast<const unsigned char *>(T.src);
      unsigned char *db = reinterpret_cast<unsigned char *>(T.dst);
      for (unsigned long long i = (unsigned long long)blk * 1024ull + tid; i < T.bytes; i += stride) db[i] = sb[i];
    }
  }
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // this workgroup's stores are out
    const unsigned done = __hip_atomic_fetch_add(T.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (done == (unsigned)T.nblocks - 1) {
      __hip_atomic_store(T.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "");
      __hip_atomic_store(T.post_word, T.post_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// Workgroups of the streaming vector kernels.  Measured at 512^3 (134 M doubles per vector, profiles/
// r03_vector_grid_512.txt): the fused Gram-Schmidt step runs at 3.8 / 6.0 / 6.4 / 6.2 / 5.4 / 5.2 / 4.9 TB/s with
// 256 / 512 / 768 / 1024 / 2048 / 4096 / 16384 workgroups of 256 lanes -- three per CU stream best (fewer, longer
// streams keep DRAM pages open); more only adds concurrent streams.  MI_HYPRE_VEC_BLOCKS overrides.
// peer-store all-reduce: see kernels.hpp.  One workgroup of 64 lanes; lane r < size talks to rank r.
__global__ __launch_bounds__(64) void ipc_poison_k(double *buf, int count, const int *error_flag) {
  if ((int)threadIdx.x < count && __hip_atomic_load(error_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    buf[threadIdx.x] = __longlong_as_double(0x7ff8000000000000LL);
}
__global__ __launch_bounds__(64) void ipc_allreduce_k(IpcAllreduce A, unsigned long long spin_limit, int *error_flag) {
  __shared__ double mine[IPC_AR_MAX];
  const int r = threadIdx.x;
  const int par = (int)(A.seq & 1ull);
  // A rank whose error flag is up (one of its bounded waits expired: its data are no longer what the algorithm thinks)
  // contributes NaN: EVERY rank then sees NaN in the SAME reduction and the Krylov loops' NaN test (gmres.c's IEEE check,
  // krylov.cpp) takes all of them out of the loop at the same point -- the collectives that are not bounded (all-gathers
  // of the wrapped communicator) stay matched, and the end-of-solve gate (capi.cpp) reports the failure on every rank.
  const bool dead = __hip_atomic_load(error_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
  if (r < A.count) mine[r] = dead ? __longlong_as_double(0x7ff8000000000000LL) : A.buf[r];
  __syncthreads();
  if (r < A.size && r != A.rank) {
    double *dst = A.peer_slots[r] + ((size_t)par * A.size + A.rank) * IPC_AR_MAX;
    for (int q = 0; q < A.count; q++) __hip_atomic_store(dst + q, mine[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(A.peer_flags[r] + (size_t)par * A.size + A.rank, A.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (r < A.size && r != A.rank) {
    const unsigned long long *fl = A.my_flags + (size_t)par * A.size + r;
    const unsigned long long t0 = wall_clock64();
    const unsigned long long limit = __hip_atomic_load(error_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? min(spin_limit, 100000ull) : spin_limit;  // (see ipc_exchange_k)
    while (__hip_atomic_load(fl, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < A.seq) {
      if (wall_clock64() - t0 > limit) {
        atomicExch(error_flag, 1);
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  if (r < A.count) {
    double sum = 0.0;
    for (int q = 0; q < A.size; q++) {  // rank order: identical bits on every rank
      const double v = (q == A.rank) ? mine[r]
                                     : __hip_atomic_load(A.my_slots + ((size_t)par * A.size + q) * IPC_AR_MAX + r,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      sum = (q == 0) ? v : sum + v;
    }
    // a sum over slots that never arrived must not pass for a number: NaN ends the Krylov loop's tests on every rank that
    // timed out, and the end-of-solve check (capi.cpp transport_gate) reports it on all of them
    if (__hip_atomic_load(error_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) sum = __longlong_as_double(0x7ff8000000000000LL);
    A.buf[r] = sum;
  }
}

inline int vec_grid_cap() {
  static const int cap = getenv("MI_HYPRE_VEC_BLOCKS") ? std::max(1, std::min(RED_MAX_BLOCKS, atoi(getenv("MI_HYPRE_VEC_BLOCKS")))) : 768;
  return cap;
}
inline int vec_grid(int n) {
  long long want = ((long long)n + 511) / 512;
  if (want < 1) want = 1;
  if (want > vec_grid_cap()) want = vec_grid_cap();
  return (int)want;
}

}  // namespace

// ---------------------------------------------------------------- host side

// Tiles of the SpMV / tile Gauss-Seidel kernels: <= 256 rows and < SPMV_TILE entries.  Whenever no 8-row
// chunk exceeds a tile the blocks begin and end on multiples of 8 rows (the hybrid-GS chunks), which the
// tile Gauss-Seidel kernel needs; *chunk_aligned says whether that held for the whole matrix.
int choose_tile_entries(int64_t nnz, int nrows) {
  static const double wide_min = getenv("MI_HYPRE_WIDE_TILE_MIN_ROWLEN") ? atof(getenv("MI_HYPRE_WIDE_TILE_MIN_ROWLEN")) : 100.0;
  return (nrows > 0 && wide_min > 0.0 && (double)nnz / (double)nrows >= wide_min) ? SPMV_TILE_WIDE : SPMV_TILE;
}

std::vector<int> build_row_blocks(int nrows, const int64_t *ia, bool *chunk_aligned, int row_cap, int tile_entries) {
  // rows per tile: at most one per thread of the kernel that runs the tile (256, or 512 for the wide tiles) when a
  // Gauss-Seidel kernel sweeps the operator; SpMV-only operators pass a larger cap
  const int block_rows = tile_entries == SPMV_TILE_WIDE ? SPMV_BLOCK_WIDE : SPMV_BLOCK;
  if (row_cap < block_rows) row_cap = block_rows;
  std::vector<int> rb;
  rb.reserve((size_t)nrows / 200 + 2);
  rb.push_back(0);
  bool aligned = true;
  int r = 0;
  while (r < nrows) {
    const int limit = (int)std::min<long long>(nrows, ((long long)r / TILE_SUPER_ROWS + 1) * TILE_SUPER_ROWS);
    const int e = tile_end(r, limit, ia, row_cap, block_rows, tile_entries, aligned);
    rb.push_back(e);
    r = e;
  }
  if (chunk_aligned) *chunk_aligned = aligned;
  return rb;
}

// MI_HYPRE_GS_TILE: 0 never, 1 every level with tiles, unset: levels with mean row length > 5
// (MI_HYPRE_GS_TILE_AVG; 512^3 7-pt: the fine level gains 6 % over the shuffle kernel, its zero-guess
// sub-operator with 3.5 entries per row does not care)
static bool gs_tile_mode(const DevCSR &A) {
  static int v = -2;
  if (v == -2) {
    const char *e = getenv("MI_HYPRE_GS_TILE");
    v = e ? atoi(e) : -1;
  }
  if (v == 0) return false;
  if (v == 1 || A.prefer_gs_tiles) return true;
  static const double thr = getenv("MI_HYPRE_GS_TILE_AVG") ? atof(getenv("MI_HYPRE_GS_TILE_AVG")) : 5.0;
  return (double)A.nnz / (double)std::max(1, A.nrows) > thr;
}

// ---- the instantiations of the solve kernels, and which of them runs.  An entry's pointer and its name (as rocprofv3's
// kernel statistics spell it) come from the same template arguments.  A table's type is its family's signature, so an
// instantiation of another family does not compile INTO A TABLE; a KernelChoice carries the pointer untyped, and the
// launchers cast it back by its family tag -- that pairing is theirs to get right.
// The compiler emits the kernels in the order the tables name them.  The tables, and ValueFormat's values that index
// them, keep the order in which the kernels have always been emitted -- fp32, dictionary, fp64; wide tiles first; TAG 1
// first; float before double -- so that the code object is laid out as it was when the kernels were tuned.
template <class Fn>
struct KernelEntry {
  Fn kernel;
  const char *name;
};
#define MI_KERNEL(...) {&__VA_ARGS__, #__VA_ARGS__}
using XcKernel = decltype(&spmv_stream_xc<0, 0, false, SPMV_BLOCK>);
using GsTileKernel = decltype(&gs_tile_k<false, SPMV_BLOCK>);
using XcMvKernel = decltype(&spmv_stream_xc_mv<2, 0, false, SPMV_BLOCK>);  // NV = 2, 3, 4 share the signature
using GsTileMvKernel = decltype(&gs_tile_mv_k<2, false, SPMV_BLOCK>);
template <class VT>
using StreamKernel = decltype(&spmv_stream<0, 0, VT>);
template <class VT>
using GsChunkKernel = decltype(&gs_group_k<8, 1, VT>);  // gs_dense_k has the same signature
template <class VT>
using GsHybridKernel = decltype(&gs_hybrid_k<VT>);
static_assert(SPMV_BLOCK == 256 && SPMV_BLOCK_WIDE == 512, "the tables below spell the block sizes out");

static int tile_block(int tile_entries) { return tile_entries == SPMV_TILE_WIDE ? SPMV_BLOCK_WIDE : SPMV_BLOCK; }

template <class Fn>
static KernelChoice chosen(const KernelEntry<Fn> &e, KernelFamily family, int block, int lpc = 0, bool batched = false) {
  return KernelChoice{(const void *)e.kernel, e.name, family, block, lpc, batched};
}

// EPI: 0 mat-vec, 1 masked Jacobi, 2 Chebyshev step.  TAG 1 names the mat-vec of the level-0 class; the wide tiles have no such instantiation.
KernelChoice choose_stream_kernel(const SolveKernelDesc &d) {
  // [ValueFormat][EPI]
  static const KernelEntry<XcKernel> xc_wide[3][3] = {
      {MI_KERNEL(spmv_stream_xc<0, 0, false, 512, true>), MI_KERNEL(spmv_stream_xc<1, 0, false, 512, true>),
       MI_KERNEL(spmv_stream_xc<2, 0, false, 512, true>)},
      {MI_KERNEL(spmv_stream_xc<0, 0, true, 512>), MI_KERNEL(spmv_stream_xc<1, 0, true, 512>),
       MI_KERNEL(spmv_stream_xc<2, 0, true, 512>)},
      {MI_KERNEL(spmv_stream_xc<0, 0, false, 512>), MI_KERNEL(spmv_stream_xc<1, 0, false, 512>),
       MI_KERNEL(spmv_stream_xc<2, 0, false, 512>)}};
  // [ValueFormat][EPI, TAG = 0, 1 / 0, 0 / 1, 0 / 2, 0]
  static const KernelEntry<XcKernel> xc[3][4] = {
      {MI_KERNEL(spmv_stream_xc<0, 1, false, 256, true>), MI_KERNEL(spmv_stream_xc<0, 0, false, 256, true>),
       MI_KERNEL(spmv_stream_xc<1, 0, false, 256, true>), MI_KERNEL(spmv_stream_xc<2, 0, false, 256, true>)},
      {MI_KERNEL(spmv_stream_xc<0, 1, true, 256>), MI_KERNEL(spmv_stream_xc<0, 0, true, 256>),
       MI_KERNEL(spmv_stream_xc<1, 0, true, 256>), MI_KERNEL(spmv_stream_xc<2, 0, true, 256>)},
      {MI_KERNEL(spmv_stream_xc<0, 1, false, 256>), MI_KERNEL(spmv_stream_xc<0, 0, false, 256>),
       MI_KERNEL(spmv_stream_xc<1, 0, false, 256>), MI_KERNEL(spmv_stream_xc<2, 0, false, 256>)}};
  // the plain stream has no dictionary form: [EPI, TAG]
  static const KernelEntry<StreamKernel<float>> plain32[4] = {
      MI_KERNEL(spmv_stream<0, 1, float>), MI_KERNEL(spmv_stream<0, 0, float>), MI_KERNEL(spmv_stream<1, 0, float>),
      MI_KERNEL(spmv_stream<2, 0, float>)};
  static const KernelEntry<StreamKernel<double>> plain[4] = {MI_KERNEL(spmv_stream<0, 1>), MI_KERNEL(spmv_stream<0, 0>),
                                                             MI_KERNEL(spmv_stream<1, 0>), MI_KERNEL(spmv_stream<2, 0>)};
  // EPI 3, the in-place colour pass of relax types 40-42: tables of their own, named after the others, so that the
  // kernels above are emitted in the order they always were.  [ValueFormat]
  static const KernelEntry<XcKernel> xc_wide_inplace[3] = {MI_KERNEL(spmv_stream_xc<3, 0, false, 512, true>),
                                                           MI_KERNEL(spmv_stream_xc<3, 0, true, 512>),
                                                           MI_KERNEL(spmv_stream_xc<3, 0, false, 512>)};
  static const KernelEntry<XcKernel> xc_inplace[3] = {MI_KERNEL(spmv_stream_xc<3, 0, false, 256, true>),
                                                      MI_KERNEL(spmv_stream_xc<3, 0, true, 256>),
                                                      MI_KERNEL(spmv_stream_xc<3, 0, false, 256>)};
  static const KernelEntry<StreamKernel<float>> plain32_inplace = MI_KERNEL(spmv_stream<3, 0, float>);
  static const KernelEntry<StreamKernel<double>> plain_inplace = MI_KERNEL(spmv_stream<3, 0>);
  // the batched mat-vec of a multivector (x cache, EPI 0): [NV - 2][ValueFormat][wide / TAG 1 / TAG 0]; tables named
  // after the others, as above
#define MI_MV_XC(NV)                                                                                                   \
  {{MI_KERNEL(spmv_stream_xc_mv<NV, 0, false, 512, true>), MI_KERNEL(spmv_stream_xc_mv<NV, 1, false, 256, true>),     \
    MI_KERNEL(spmv_stream_xc_mv<NV, 0, false, 256, true>)},                                                            \
   {MI_KERNEL(spmv_stream_xc_mv<NV, 0, true, 512>), MI_KERNEL(spmv_stream_xc_mv<NV, 1, true, 256>),                   \
    MI_KERNEL(spmv_stream_xc_mv<NV, 0, true, 256>)},                                                                   \
   {MI_KERNEL(spmv_stream_xc_mv<NV, 0, false, 512>), MI_KERNEL(spmv_stream_xc_mv<NV, 1, false, 256>),                 \
    MI_KERNEL(spmv_stream_xc_mv<NV, 0, false, 256>)}}
  static const KernelEntry<XcMvKernel> xc_mv[MV_MAX_BATCH - 1][3][3] = {MI_MV_XC(2), MI_MV_XC(3), MI_MV_XC(4)};
#undef MI_MV_XC
  MI_REQUIRE(d.epi >= 0 && d.epi <= 3, "choose_stream_kernel: the epilogue is 0, 1, 2 or 3");
  MI_REQUIRE(d.nvec >= 1 && d.nvec <= MV_MAX_BATCH, "choose_stream_kernel: 1 to 4 components per pass");
  const int fmt = (int)d.format;
  if (d.nvec > 1 && d.xcache && d.epi == 0)
    return chosen(xc_mv[d.nvec - 2][fmt][d.tile_entries == SPMV_TILE_WIDE ? 0 : d.level0 ? 1 : 2], KernelFamily::STREAM_XC,
                  tile_block(d.tile_entries), 0, true);
  if (d.epi == 3) {
    if (d.xcache)
      return chosen(d.tile_entries == SPMV_TILE_WIDE ? xc_wide_inplace[fmt] : xc_inplace[fmt], KernelFamily::STREAM_XC,
                    tile_block(d.tile_entries));
    if (d.format == ValueFormat::FP32) return chosen(plain32_inplace, KernelFamily::STREAM, SPMV_BLOCK);
    return chosen(plain_inplace, KernelFamily::STREAM, SPMV_BLOCK);
  }
  const int epi_tag = d.epi == 2 ? 3 : d.epi == 1 ? 2 : d.level0 ? 0 : 1;
  if (d.xcache)
    return chosen(d.tile_entries == SPMV_TILE_WIDE ? xc_wide[fmt][d.epi] : xc[fmt][epi_tag], KernelFamily::STREAM_XC,
                  tile_block(d.tile_entries));
  if (d.format == ValueFormat::FP32) return chosen(plain32[epi_tag], KernelFamily::STREAM, SPMV_BLOCK);
  return chosen(plain[epi_tag], KernelFamily::STREAM, SPMV_BLOCK);
}

// the value stream as the tile kernels (spmv_stream_xc, gs_tile_k) take it: their VAL4 instantiations read the floats
// through the `av` of the other instantiations.  (vidx / vlut go to every instantiation; only the VAL8 ones look at them.)
static const double *tile_values(const DevCSR &A) {
  return A.value_format() == ValueFormat::FP32 ? reinterpret_cast<const double *>(A.a32.p) : A.a.p;
}
// launch(kernel, values) with the float or the double signature of a family whose kernels take the values as VT
template <template <class> class Fn, class Launch>
static void launch_on_values(const DevCSR &A, const KernelChoice &c, Launch launch) {
  if (A.value_format() == ValueFormat::FP32)
    launch((Fn<float>)c.kernel, A.a32.p);
  else
    launch((Fn<double>)c.kernel, A.a.p);
}

// returns the name of the instantiation it launched
static const char *launch_stream(int epi, const DevCSR &A, const double *x, double *y, const EpiArgs &e, hipStream_t s,
                                 bool level0 = false, int ntiles = 0, const int *tdesc = nullptr) {
  if (A.nrows == 0) return "";
  MI_REQUIRE(A.xcache || !A.big(), "an operator with 2^31 entries or more must be in the x-cache tile format");
  // (fp32 value storage, k::narrow_values: `a` is gone, the kernels stream a32)
  MI_REQUIRE(A.value_format() == ValueFormat::FP32 || A.a.p || A.nnz == 0, "SpMV: the operator holds no value array");
  const KernelChoice c = choose_stream_kernel({A.xcache, A.tile_entries, A.value_format(), epi, level0});
  // (EPI 3: the tiles [e.blk0, e.blk0 + ntiles); tdesc: the ntiles tiles of a descriptor list of the caller's)
  const int nb = (epi == 3 || tdesc) ? ntiles : A.nblocks;
  MI_REQUIRE(!tdesc || c.family == KernelFamily::STREAM_XC, "SpMV: a tile list needs the x-cache tile format");
  const int xchunk = (nb + 7) / 8;
  const dim3 grid(xchunk * 8), block(c.block);
  if (c.family == KernelFamily::STREAM_XC) {
    hipLaunchKernelGGL((XcKernel)c.kernel, grid, block, 0, s, nb, xchunk, tdesc ? tdesc : A.tdesc.p, A.ia.p, A.ja.p,
                       tile_values(A), A.ucols.p, A.lcol.p, x, y, e, A.vidx.p, A.vlut.p);
  } else {
    launch_on_values<StreamKernel>(A, c, [&](auto kernel, auto *values) {
      hipLaunchKernelGGL(kernel, grid, block, 0, s, nb, xchunk, A.rb.p, A.ia.p, A.ja.p, values, x, y, e);
    });
  }
  MI_HIP(hipGetLastError());
  return c.name;
}

namespace {
// vidx[k] = position of a[k] in the sorted table of bit patterns; *fail counts values that are not in it
__global__ __launch_bounds__(256) void value_index_k(long long n, const double *__restrict__ a,
                                                     const long long *__restrict__ table, int nt,
                                                     unsigned char *__restrict__ vidx, int *__restrict__ fail) {
  const long long stride = (long long)gridDim.x * 256;
  int bad = 0;
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n; k += stride) {
    const long long bits = __double_as_longlong(a[k]);
    int lo = 0, hi = nt;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (table[mid] < bits)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo < nt && table[lo] == bits)
      vidx[k] = (unsigned char)lo;
    else
      bad = 1;
  }
  if (bad) atomicAdd(fail, 1);
}
}  // namespace

namespace {
__global__ __launch_bounds__(256) void strided_sample_k(const double *__restrict__ a, size_t stride, int n, double *__restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < n) out[k] = a[(size_t)k * stride];
}
}  // namespace

static int g_value_dict = -1;
bool value_dictionary_enabled() {
  if (g_value_dict < 0) g_value_dict = (getenv("MI_HYPRE_VALUE_DICT") && atoi(getenv("MI_HYPRE_VALUE_DICT")) == 0) ? 0 : 1;
  return g_value_dict == 1;
}
void set_value_dictionary(bool on) { g_value_dict = on ? 1 : 0; }

// Value dictionary of an operator in the solve format: distinct values (bit patterns) of a sample, at most 256;
// one pass then encodes every entry or finds one that is not in the table (the operator keeps the plain stream).
// MI_HYPRE_VALUE_DICT=0 switches it off.
void build_value_dictionary(DevCSR &A, hipStream_t s) {
  A.vidx.release();
  A.vlut.release();
  if (!value_dictionary_enabled() || !A.xcache || A.nnz < (1 << 16) || !A.a.p) return;
  // a strided sample over the whole array (the leading rows alone are not representative: the C rows of a
  // zero-guess sub-operator hold nothing but their diagonal); enough to see > 256 distinct values at once
  const size_t sample = (size_t)std::min<int64_t>(A.nnz, 1 << 16);
  const size_t stride = (size_t)A.nnz / sample;
  std::vector<double> hs(sample);
  {
    // (a kernel, not hipMemcpy2DAsync: the strided source may span several physical chunks of the device arena, which
    // the 2-D copy refuses with "invalid argument")
    DVec<double> dsample(sample);
    hipLaunchKernelGGL(strided_sample_k, dim3((unsigned)((sample + 255) / 256)), dim3(256), 0, s, A.a.p, stride, (int)sample, dsample.p);
    MI_HIP(hipGetLastError());
    d2h(hs.data(), dsample.p, sample * sizeof(double), s);
    MI_HIP(hipStreamSynchronize(s));
  }
  std::vector<long long> bits(sample);
  std::memcpy(bits.data(), hs.data(), sample * sizeof(double));
  std::sort(bits.begin(), bits.end());
  bits.erase(std::unique(bits.begin(), bits.end()), bits.end());
  if (bits.size() > 256) return;
  const int nt = (int)bits.size();
  DVec<long long> dtab;
  dtab.upload(bits);
  DVec<int> fail(1);
  MI_HIP(hipMemsetAsync(fail.p, 0, sizeof(int), s));
  A.vidx.alloc((size_t)A.nnz);
  hipLaunchKernelGGL(value_index_k, dim3(4096), dim3(256), 0, s, (long long)A.nnz, A.a.p, dtab.p, nt, A.vidx.p, fail.p);
  int nfail = 0;
  d2h(&nfail, fail.p, sizeof(int), s);
  MI_HIP(hipStreamSynchronize(s));
  if (nfail) {  // a value beyond the sample's 256: plain stream
    A.vidx.release();
    return;
  }
  std::vector<double> lut(256, 0.0);
  std::memcpy(lut.data(), bits.data(), (size_t)nt * sizeof(double));
  A.vlut.upload(lut);  // (its presence is what makes the operator a dictionary one: DevCSR::value_format)
}

void build_tile_desc(DevCSR &A, const long long *ia64, hipStream_t s) {
  A.tdesc.release();
  if (A.nblocks <= 0 || !A.rb.p) return;
  A.tdesc.alloc((size_t)A.nblocks * 8);
  hipLaunchKernelGGL(tile_desc_k, dim3((unsigned)((A.nblocks + 255) / 256)), dim3(256), 0, s, A.nblocks, A.rb.p, ia64,
                     A.xcache ? A.uptr.p : nullptr, A.tdesc.p);
  MI_HIP(hipGetLastError());
  MI_HIP(hipStreamSynchronize(s));
  build_value_dictionary(A, s);
}

void spmv(const DevCSR &A, const double *x, double alpha, double beta, const double *b, double *y, hipStream_t s,
          int prof, const double *b_lo, int b_split) {
  EpiArgs e{};
  e.alpha = alpha;
  e.beta = beta;
  e.b = b;
  e.b_lo = b_lo;
  e.b_split = b_split;
  e.rowmap = A.rowmap.p;
  prof_begin(prof, s);
  prof_name(prof, launch_stream(0, A, x, y, e, s, prof == PROF_SPMV_L0));
  prof_end(prof, s);
}

static int g_mv_batch = 0;
int multivector_batch() {
  if (g_mv_batch == 0) {
    const int v = getenv("MI_HYPRE_MV_BATCH") ? atoi(getenv("MI_HYPRE_MV_BATCH")) : MV_BATCH_DEFAULT;
    g_mv_batch = (v >= 1 && v <= MV_MAX_BATCH) ? v : MV_BATCH_DEFAULT;
  }
  return g_mv_batch;
}
void set_multivector_batch(int width) {
  MI_REQUIRE(width >= 1 && width <= MV_MAX_BATCH, "multivector batch: the width is 1, 2, 3 or 4");
  g_mv_batch = width;
}

int spmv_multi(const DevCSR &A, int nvec, const double *x, long long x_stride, double alpha, double beta, const double *b,
               long long b_stride, double *y, long long y_stride, hipStream_t s, int prof, const double *b_lo,
               long long b_lo_stride, int b_split) {
  const int width = multivector_batch();
  // the batched form exists for the x-cache tile format alone (choose_stream_kernel); one component needs none
  const bool batch = nvec > 1 && width > 1 && A.nrows > 0 && A.xcache;
  int passes = 0;
  for (int c0 = 0; c0 < nvec;) {
    const int nv = batch ? std::min(width, nvec - c0) : 1;
    const double *xc = x + c0 * x_stride, *bc = b ? b + c0 * b_stride : nullptr;
    const double *bloc = b_lo ? b_lo + c0 * b_lo_stride : nullptr;
    double *yc = y + c0 * y_stride;
    if (nv == 1) {
      spmv(A, xc, alpha, beta, bc, yc, s, prof, bloc, b_split);
    } else {
      MI_REQUIRE(A.value_format() == ValueFormat::FP32 || A.a.p || A.nnz == 0, "SpMV: the operator holds no value array");
      SolveKernelDesc d{A.xcache, A.tile_entries, A.value_format(), 0, prof == PROF_SPMV_L0};
      d.nvec = nv;
      const KernelChoice c = choose_stream_kernel(d);
      MI_REQUIRE(c.batched, "SpMV: no batched instantiation for an operator in the x-cache tile format");
      EpiArgs e{};
      e.alpha = alpha;
      e.beta = beta;
      e.b = bc;
      e.b_lo = bloc;
      e.b_split = b_split;
      e.rowmap = A.rowmap.p;
      const MvStrides st{x_stride, y_stride, b_stride, b_lo_stride};
      const int nb = A.nblocks, xchunk = (nb + 7) / 8;
      prof_begin(prof, s);
      hipLaunchKernelGGL((XcMvKernel)c.kernel, dim3(xchunk * 8), dim3(c.block), 0, s, nb, xchunk, A.tdesc.p, A.ia.p, A.ja.p,
                         tile_values(A), A.ucols.p, A.lcol.p, xc, yc, e, st, A.vidx.p, A.vlut.p);
      MI_HIP(hipGetLastError());
      prof_name(prof, c.name);
      prof_end(prof, s);
    }
    if (batch) passes++;
    c0 += nv;
  }
  return passes;
}

void spmv_listed_tiles(const DevCSR &A, const int *tdesc, int nb, const double *x, double *y, hipStream_t s, int prof) {
  if (nb <= 0) return;
  MI_REQUIRE(tdesc && !A.rowmap.p, "SpMV on a tile list: no list, or an operator stored in another row order");
  EpiArgs e{};
  e.alpha = 1.0;
  prof_begin(prof, s);
  prof_name(prof, launch_stream(0, A, x, y, e, s, prof == PROF_SPMV_L0, nb, tdesc));
  prof_end(prof, s);
}

void jacobi(const DevCSR &A, const double *u_old, double *u_new, const double *f, const double *offc, const double *d,
            const signed char *cf, int points, double w, hipStream_t s, int prof) {
  EpiArgs e{};
  e.alpha = w;
  e.b = f;
  e.offc = offc;
  e.d = d;
  e.cf = cf;
  e.points = points;
  prof_begin(prof, s);
  prof_name(prof, launch_stream(1, A, u_old, u_new, e, s));
  prof_end(prof, s);
}

void cheby_step(const DevCSR &A, const double *u_old, double *u_new, double *dc, const double *f, const double *offc,
                const double *diag, double a, double b, hipStream_t s, int prof) {
  EpiArgs e{};
  e.b = f;
  e.offc = offc;
  e.d = diag;
  e.dc = dc;
  e.ca = a;
  e.cb = b;
  prof_begin(prof, s);
  prof_name(prof, launch_stream(2, A, u_old, u_new, e, s));
  prof_end(prof, s);
}

void inplace_pass(const DevCSR &A, double *u, const double *f, const double *offc, const double *d, double w,
                  int row_begin, int row_end, hipStream_t s, int prof) {
  row_begin = std::max(row_begin, 0);
  row_end = std::min(row_end, A.nrows);
  if (A.nrows == 0 || row_end <= row_begin) return;
  const std::vector<int> &rbh = A.rb_host;
  MI_REQUIRE((int)rbh.size() == A.nblocks + 1, "in-place pass: the operator has no host copy of its tile schedule");
  // the tiles that intersect the range: the last one that starts at or before row_begin ... the first that starts at or after row_end
  const int b0 = (int)(std::upper_bound(rbh.begin(), rbh.end(), row_begin) - rbh.begin()) - 1;
  const int b1 = (int)(std::lower_bound(rbh.begin(), rbh.end(), row_end) - rbh.begin());
  MI_REQUIRE(b0 >= 0 && b1 > b0 && b1 <= A.nblocks, "in-place pass: the row range lies outside the tile schedule");
  EpiArgs e{};
  e.alpha = w;
  e.b = f;
  e.offc = offc;
  e.d = d;
  e.u = u;
  e.row_begin = row_begin;
  e.row_end = row_end;
  e.blk0 = b0;
  prof_begin(prof, s);
  prof_name(prof, launch_stream(3, A, nullptr, nullptr, e, s, false, b1 - b0));
  prof_end(prof, s);
}

namespace {
// step 0 of a Chebyshev sweep on a zero guess: what the EPI 2 epilogue computes from a zero vector (row sum +0, no halo
// part), bit for bit
__global__ __launch_bounds__(256) void cheby_first_k(int n, const double *__restrict__ f, const double *__restrict__ diag,
                                                     double b0, double *__restrict__ dc, double *__restrict__ u) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double dn = b0 * ((f[i] - 0.0) / diag[i]);
  dc[i] = dn;
  u[i] = 0.0 + dn;
}
__global__ __launch_bounds__(256) void inv_sqrt_k(int n, const double *__restrict__ x, double *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = 1.0 / sqrt(x[i]);
}
__global__ __launch_bounds__(256) void vec_mul_k(int n, const double *__restrict__ x, const double *__restrict__ y,
                                                 double *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = x[i] * y[i];
}
// sum[i] = sum_j |a_ij| of the rows of a diag block (IA: the 32-bit row pointers, or the 64-bit ones of a big operator)
template <class IA, class VT>
__global__ __launch_bounds__(256) void row_abs_sum_k(int n, const IA *__restrict__ ia, const VT *__restrict__ a,
                                                     double *__restrict__ sum) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double t = 0.0;
  for (long long k = (long long)ia[i]; k < (long long)ia[i + 1]; k++) t += fabs((double)a[k]);
  sum[i] = t;
}
// ... plus the halo block's entries (compressed rows: each stored row belongs to one lane)
__global__ __launch_bounds__(256) void offd_abs_add_k(int nrows_c, const int *__restrict__ rows, const int *__restrict__ ia,
                                                      const double *__restrict__ a, double *__restrict__ sum) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nrows_c) return;
  double t = 0.0;
  for (int k = ia[q]; k < ia[q + 1]; k++) t += fabs(a[k]);
  sum[rows[q]] += t;
}
// out[0] = max_i sum[i] / diag[i] as the bit pattern of a non-negative double (patterns order like the values; a NaN
// sorts above every number and so survives), out[1] = number of rows whose diagonal is not positive.  out starts as 0, 0.
__global__ __launch_bounds__(256) void gershgorin_k(int n, const double *__restrict__ sum, const double *__restrict__ diag,
                                                    unsigned long long *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  unsigned long long bits = 0ULL, bad = 0ULL;
  if (i < n) {
    const double d = diag[i];
    if (d > 0.0)
      bits = (unsigned long long)__double_as_longlong(fabs(sum[i] / d));
    else
      bad = 1ULL;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(bits, off, 64);
    bits = o > bits ? o : bits;
    bad += __shfl_down(bad, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (bits) atomicMax(out, bits);
    if (bad) atomicAdd(out + 1, bad);
  }
}
}  // namespace

void cheby_first(const double *f, const double *diag, double b0, double *dc, double *u, int n, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(cheby_first_k, dim3((n + 255) / 256), dim3(256), 0, s, n, f, diag, b0, dc, u);
  MI_HIP(hipGetLastError());
}
void inv_sqrt(const double *x, double *out, int n, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(inv_sqrt_k, dim3((n + 255) / 256), dim3(256), 0, s, n, x, out);
  MI_HIP(hipGetLastError());
}
void vec_mul(const double *x, const double *y, double *out, int n, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(vec_mul_k, dim3((n + 255) / 256), dim3(256), 0, s, n, x, y, out);
  MI_HIP(hipGetLastError());
}
void gershgorin(const DevCSR &A, const DevOffd &B, const double *diag, double *work, double *lambda_max,
                long long *bad_diagonals, hipStream_t s) {
  const int n = A.nrows;
  *lambda_max = 0.0;
  *bad_diagonals = 0;
  if (n == 0) return;
  const dim3 grid((n + 255) / 256), block(256);
  MI_REQUIRE(A.a.p || A.a32.p || A.nnz == 0, "gershgorin: the operator holds no value array");
  if (A.big()) {
    MI_REQUIRE(A.ia64.p != nullptr, "gershgorin: a big operator without 64-bit row pointers");
    if (A.a.p)
      hipLaunchKernelGGL((row_abs_sum_k<long long, double>), grid, block, 0, s, n, A.ia64.p, A.a.p, work);
    else
      hipLaunchKernelGGL((row_abs_sum_k<long long, float>), grid, block, 0, s, n, A.ia64.p, A.a32.p, work);
  } else if (A.a.p) {
    hipLaunchKernelGGL((row_abs_sum_k<int, double>), grid, block, 0, s, n, A.ia.p, A.a.p, work);
  } else {
    hipLaunchKernelGGL((row_abs_sum_k<int, float>), grid, block, 0, s, n, A.ia.p, A.a32.p, work);
  }
  MI_HIP(hipGetLastError());
  if (B.nrows_c > 0) {
    hipLaunchKernelGGL(offd_abs_add_k, dim3((B.nrows_c + 255) / 256), block, 0, s, B.nrows_c, B.rows.p, B.ia.p, B.a.p, work);
    MI_HIP(hipGetLastError());
  }
  DVec<unsigned long long> out(2);
  MI_HIP(hipMemsetAsync(out.p, 0, 2 * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(gershgorin_k, grid, block, 0, s, n, work, diag, out.p);
  MI_HIP(hipGetLastError());
  unsigned long long h[2] = {0, 0};
  d2h(h, out.p, sizeof(h), s);
  MI_HIP(hipStreamSynchronize(s));
  std::memcpy(lambda_max, &h[0], sizeof(double));
  *bad_diagonals = (long long)h[1];
}

void spmv_offd_add(const DevOffd &B, const double *xext, double alpha, double *y, hipStream_t s) {
  if (B.nrows_c == 0) return;
  hipLaunchKernelGGL(spmv_offd_k<0>, dim3((B.nrows_c + 255) / 256), dim3(256), 0, s, B.nrows_c, B.rows.p, B.ia.p,
                     B.ja.p, B.a.p, xext, alpha, y);
  MI_HIP(hipGetLastError());
}
void spmv_offd_set(const DevOffd &B, const double *xext, double *out, hipStream_t s) {
  if (B.nrows_c == 0) return;
  hipLaunchKernelGGL(spmv_offd_k<1>, dim3((B.nrows_c + 255) / 256), dim3(256), 0, s, B.nrows_c, B.rows.p, B.ia.p,
                     B.ja.p, B.a.p, xext, 1.0, out);
  MI_HIP(hipGetLastError());
}

// Measured per level (256^3 / 512^3 Laplacian hierarchies, profiles/compare_gs.*):
//   mean row length <= 8 (the fine level): the shuffle kernel with 8 lanes per chunk is memory-bound
//   already (3.9 TB/s) and beats the dense-chunk kernel, whose barriers and LDS block it does not need;
//   longer rows: the dense-chunk kernel wins 10-18 %; for means up to 32 two chunks per wave (32 lanes
//   each, rows beyond 32 entries finished in the pre-sweep loop) beat one chunk per wave.
KernelChoice choose_gs_kernel(const SolveKernelDesc &d) {
  MI_REQUIRE(d.nvec >= 1 && d.nvec <= MV_MAX_BATCH, "choose_gs_kernel: 1 to 4 components per pass");
  if (d.nvec > 1 && d.chunk == 8 && d.tiles && d.xcache) {
    // the batched tile kernel of a multivector: [NV - 2][ValueFormat][2048-entry tiles]
#define MI_MV_GS(NV)                                                                            \
  {{MI_KERNEL(gs_tile_mv_k<NV, false, 512, true>), MI_KERNEL(gs_tile_mv_k<NV, false, 256, true>)}, \
   {MI_KERNEL(gs_tile_mv_k<NV, true, 512>), MI_KERNEL(gs_tile_mv_k<NV, true, 256>)},             \
   {MI_KERNEL(gs_tile_mv_k<NV, false, 512>), MI_KERNEL(gs_tile_mv_k<NV, false, 256>)}}
    static const KernelEntry<GsTileMvKernel> tile_mv[MV_MAX_BATCH - 1][3][2] = {MI_MV_GS(2), MI_MV_GS(3), MI_MV_GS(4)};
#undef MI_MV_GS
    return chosen(tile_mv[d.nvec - 2][(int)d.format][d.tile_entries != SPMV_TILE_WIDE], KernelFamily::GS_TILE,
                  tile_block(d.tile_entries), 0, true);
  }
  if (d.chunk == 8 && d.tiles && d.xcache) {
    // [ValueFormat][2048-entry tiles]
    static const KernelEntry<GsTileKernel> tile[3][2] = {
        {MI_KERNEL(gs_tile_k<false, 512, true>), MI_KERNEL(gs_tile_k<false, 256, true>)},
        {MI_KERNEL(gs_tile_k<true, 512>), MI_KERNEL(gs_tile_k<true, 256>)},
        {MI_KERNEL(gs_tile_k<false, 512>), MI_KERNEL(gs_tile_k<false, 256>)}};
    return chosen(tile[(int)d.format][d.tile_entries != SPMV_TILE_WIDE], KernelFamily::GS_TILE, tile_block(d.tile_entries));
  }
  const bool f32 = d.format == ValueFormat::FP32;
  if (d.chunk == 8) {
    // the first rule that holds: mean row length <= avg_max and 95th percentile of the row lengths <= p95_max
    struct Rule {
      double avg_max;
      int p95_max;
      KernelFamily family;
      int lpc;
      KernelEntry<GsChunkKernel<float>> fp32;
      KernelEntry<GsChunkKernel<double>> fp64;
    };
#define MI_CHUNK_KERNEL(KERNEL, FAMILY, LPC, E) \
  KernelFamily::FAMILY, LPC, MI_KERNEL(KERNEL<LPC, E, float>), MI_KERNEL(KERNEL<LPC, E>)
    constexpr int any = std::numeric_limits<int>::max();
    constexpr double longer = std::numeric_limits<double>::infinity();
    static const Rule rules[] = {{8.0, 8, MI_CHUNK_KERNEL(gs_group_k, GS_GROUP, 8, 1)},
                                 {8.0, any, MI_CHUNK_KERNEL(gs_group_k, GS_GROUP, 8, 2)},
                                 {16.0, 16, MI_CHUNK_KERNEL(gs_dense_k, GS_DENSE, 16, 1)},
                                 {16.0, any, MI_CHUNK_KERNEL(gs_dense_k, GS_DENSE, 16, 2)},
                                 {32.0, 64, MI_CHUNK_KERNEL(gs_dense_k, GS_DENSE, 32, 1)},
                                 {32.0, any, MI_CHUNK_KERNEL(gs_dense_k, GS_DENSE, 32, 2)},
                                 {longer, 64, MI_CHUNK_KERNEL(gs_dense_k, GS_DENSE, 64, 1)},
                                 {longer, 128, MI_CHUNK_KERNEL(gs_dense_k, GS_DENSE, 64, 2)},
                                 {longer, any, MI_CHUNK_KERNEL(gs_dense_k, GS_DENSE, 64, 4)}};
#undef MI_CHUNK_KERNEL
    const double avg = (double)d.nnz / (double)std::max(1, d.nrows);
    const Rule *r = rules;
    while (avg > r->avg_max || d.rowlen_p95 > r->p95_max) r++;  // (the last rule holds for every operator)
    return f32 ? chosen(r->fp32, r->family, 256, r->lpc) : chosen(r->fp64, r->family, 256, r->lpc);
  }
  static const KernelEntry<GsHybridKernel<float>> hybrid32 = MI_KERNEL(gs_hybrid_k<float>);
  // (the fp64 instantiation has gone by the template's bare name since before there was a float one)
  static const KernelEntry<GsHybridKernel<double>> hybrid = {&gs_hybrid_k<double>, "gs_hybrid_k"};
  return f32 ? chosen(hybrid32, KernelFamily::GS_HYBRID, GS_BLOCK) : chosen(hybrid, KernelFamily::GS_HYBRID, GS_BLOCK);
}
#undef MI_KERNEL

static KernelChoice gs_choice(const DevCSR &A, int chunk, int nvec = 1) {
  return choose_gs_kernel({A.xcache, A.tile_entries, A.value_format(), 0, false, chunk, A.gs_tiles && gs_tile_mode(A), A.nnz,
                           A.nrows, A.rowlen_p95, nvec});
}

bool gs_uses_tiles(const DevCSR &A, int chunk) { return gs_choice(A, chunk).family == KernelFamily::GS_TILE; }

// whether a sweep of A with zero_from == 0 never reads the pre-sweep vector (gs_tile_k and gs_group_k skip every
// gather and take 0 for the rows' own values; gs_dense_k and gs_hybrid_k, for chunk != 8, read real zeros)
bool gs_ignores_zero_vector(const DevCSR &A, int chunk) {
  if (A.nrows == 0) return false;
  const KernelFamily family = gs_choice(A, chunk).family;
  return family == KernelFamily::GS_TILE || family == KernelFamily::GS_GROUP;
}

// the tile kernel's launch for the rows [row_begin, row_end): the chunks [c0, c1) that intersect them are rows
// [first_row, last_row); they lie in the tiles [b0, b1) -- first tile with rb[b+1] > c0*8, last tile with rb[b] < c1*8
static void gs_tile_range(const DevCSR &A, int row_begin, int row_end, int &first_row, int &last_row, int &b0, int &b1) {
  const long long c0 = row_begin / 8;
  const long long c1 = ((long long)row_end + 7) / 8;
  const std::vector<int> &rbh = A.rb_host;
  first_row = (int)(c0 * 8);
  last_row = (int)std::min<long long>(c1 * 8, A.nrows);
  b0 = (int)(std::upper_bound(rbh.begin(), rbh.end(), first_row) - rbh.begin()) - 1;
  b1 = (int)(std::lower_bound(rbh.begin(), rbh.end(), last_row) - rbh.begin());
}

// Host-side census of the branches gs_tile_k's sweep phase takes in one pass (tests, and the per-level shares in
// DESIGN.md section 5): the same launch geometry and the same three predicates, evaluated on a host copy of the
// operator's pattern (ia / ja: any operator with A's in-chunk entries, e.g. the level operator for its zero-guess
// sub-operator; cf: +1 / -1 per row or null).  counts: waves launched, waves without a selected row, waves whose
// chunks couple to nothing in-chunk but their own diagonal, zero-guess waves on the short forward sweep, waves on the
// general sweep.  false: the pass does not run on the tile kernel.
bool gs_tile_path_census(const DevCSR &A, int chunk, const int64_t *ia, const int *ja, const int *cf, int points,
                         int row_begin, int row_end, int zero_from, long long counts[5]) {
  for (int q = 0; q < 5; q++) counts[q] = 0;
  const KernelChoice c = gs_choice(A, chunk);
  if (A.nrows == 0 || row_end <= row_begin || c.family != KernelFamily::GS_TILE) return false;
  int first_row, last_row, b0, b1;
  gs_tile_range(A, row_begin, row_end, first_row, last_row, b0, b1);
  const int block = c.block;
  for (int b = b0; b < b1; b++) {
    const int r0 = A.rb_host[(size_t)b], nr = A.rb_host[(size_t)b + 1] - r0;
    const int LPR = nr <= block / 8 ? 8 : nr <= block / 4 ? 4 : nr <= block / 2 ? 2 : 1;
    for (int wv = 0; wv < block / 64; wv++) {
      bool any = false, coupled = false;
      for (int rl = wv * 64 / LPR; rl < std::min((wv + 1) * 64 / LPR, nr); rl++) {
        const int i = r0 + rl;
        const int mark = (points != 0 && cf != nullptr) ? cf[i] : points;
        if (mark != points || i < first_row || i >= last_row) continue;
        any = true;
        for (int64_t q = ia[i]; q < ia[i + 1]; q++) coupled |= (ja[q] >> 3) == (i >> 3) && ja[q] != i;
      }
      counts[0]++;
      counts[!any ? 1 : !coupled ? 2 : r0 >= zero_from ? 3 : 4]++;
    }
  }
  return true;
}

void gs_hybrid(const DevCSR &A, const double *u_lo, const double *u_hi, int split, double *out, const double *f,
               const double *offc, const double *d, const signed char *cf, int points, int chunk, bool fwd, bool bwd,
               double w, int row_begin, int row_end, hipStream_t s, int prof, int zero_from, double *tout,
               int t_from, double *wout) {
  if (A.nrows == 0 || row_end <= row_begin) return;
  MI_REQUIRE(chunk >= 1 && chunk <= GS_MAX_CHUNK, "hybrid GS chunk out of range");
  // chunks that intersect [row_begin, row_end); pre-sweep values come from u_lo
  // (rows < split) / u_hi (rows >= split), the swept chunks' rows go to out
  const long long c0 = row_begin / chunk;
  const long long c1 = ((long long)row_end + chunk - 1) / chunk;
  const long long nch = c1 - c0;
  const KernelChoice c = gs_choice(A, chunk);
  const dim3 block(c.block);
  prof_begin(prof, s);
  if (c.family == KernelFamily::GS_TILE) {
    int first_row, last_row, b0, b1;
    gs_tile_range(A, row_begin, row_end, first_row, last_row, b0, b1);
    MI_REQUIRE(!wout || (MI_GS_SWEEP_PATHS & 2), "hybrid GS: the C-row hand-over needs the kernel's diagonal-chunk branch");
    if (b1 > b0) {
      prof_name(prof, c.name);
      hipLaunchKernelGGL((GsTileKernel)c.kernel, dim3((unsigned)(b1 - b0)), block, 0, s, b0, b1 - b0, A.tdesc.p, A.ia.p,
                         tile_values(A), A.ucols.p, A.lcol.p, cf, points, d, f, offc, u_lo, u_hi, split, out, fwd ? 1 : 0,
                         bwd ? 1 : 0, w, first_row, last_row, zero_from, tout, t_from, A.vidx.p, A.vlut.p, wout);
    }
  } else {
    MI_REQUIRE(!wout, "hybrid GS: only the tile kernel hands the C rows' products over");
    MI_REQUIRE(!A.big(), "an operator with 2^31 entries or more is swept by the tile Gauss-Seidel kernel only");
    prof_name(prof, c.name);
    if (c.family == KernelFamily::GS_HYBRID) {
      const size_t lds = (size_t)chunk * GS_BLOCK * sizeof(double);
      launch_on_values<GsHybridKernel>(A, c, [&](auto kernel, auto *values) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((nch + GS_BLOCK - 1) / GS_BLOCK)), block, lds, s, A.nrows, (int)c0,
                           (int)c1, chunk, A.ia.p, A.ja.p, values, cf, points, d, f, offc, u_lo, u_hi, split, out,
                           fwd ? 1 : 0, bwd ? 1 : 0, w);
      });
    } else {
      const long long waves = (nch + (64 / c.lpc) - 1) / (64 / c.lpc);
      launch_on_values<GsChunkKernel>(A, c, [&](auto kernel, auto *values) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((waves + 3) / 4)), block, 0, s, A.nrows, (int)c0, (int)c1, A.ia.p,
                           A.ja.p, values, cf, points, d, f, offc, u_lo, u_hi, split, out, fwd ? 1 : 0, bwd ? 1 : 0, w,
                           zero_from);
      });
    }
  }
  MI_HIP(hipGetLastError());
  prof_end(prof, s);
}

int gs_hybrid_multi(const DevCSR &A, int nvec, const GsMultiStrides &st, const double *u_lo, const double *u_hi, int split,
                    double *out, const double *f, const double *offc, const double *d, const signed char *cf, int points,
                    int chunk, bool fwd, bool bwd, double w, int row_begin, int row_end, hipStream_t s, int prof,
                    int zero_from, double *tout, int t_from) {
  if (A.nrows == 0 || row_end <= row_begin) return 0;
  const int width = multivector_batch();
  const bool batch = nvec > 1 && width > 1 && gs_uses_tiles(A, chunk);
  int passes = 0;
  for (int c0 = 0; c0 < nvec;) {
    const int nv = batch ? std::min(width, nvec - c0) : 1;
    const double *ulo = u_lo + c0 * st.u_lo, *uhi = u_hi + c0 * st.u_hi, *fc = f + c0 * st.f;
    const double *oc = offc ? offc + c0 * st.offc : nullptr;
    double *outc = out + c0 * st.out, *tc = tout ? tout + c0 * st.tout : nullptr;
    if (nv == 1) {
      gs_hybrid(A, ulo, uhi, split, outc, fc, oc, d, cf, points, chunk, fwd, bwd, w, row_begin, row_end, s, prof,
                zero_from, tc, t_from);
    } else {
      const KernelChoice c = gs_choice(A, chunk, nv);
      MI_REQUIRE(c.batched && c.family == KernelFamily::GS_TILE, "hybrid GS: no batched instantiation for a tile operator");
      int first_row, last_row, b0, b1;
      gs_tile_range(A, row_begin, row_end, first_row, last_row, b0, b1);
      prof_begin(prof, s);
      if (b1 > b0) {
        prof_name(prof, c.name);
        hipLaunchKernelGGL((GsTileMvKernel)c.kernel, dim3((unsigned)(b1 - b0)), dim3(c.block), 0, s, b0, b1 - b0, A.tdesc.p,
                           A.ia.p, tile_values(A), A.ucols.p, A.lcol.p, cf, points, d, fc, oc, ulo, uhi, split, outc,
                           fwd ? 1 : 0, bwd ? 1 : 0, w, first_row, last_row, zero_from, tc, t_from, st, A.vidx.p, A.vlut.p);
      }
      MI_HIP(hipGetLastError());
      prof_end(prof, s);
    }
    if (batch) passes++;
    c0 += nv;
  }
  return passes;
}

// workgroups of the inner-product kernels (MI_HYPRE_DOT_BLOCKS, at most RED_MAX_BLOCKS * MASS_NV partial slots)
static int dot_grid(int n) {
  static const int cap = getenv("MI_HYPRE_DOT_BLOCKS") ? std::max(1, std::min(RED_MAX_BLOCKS * MASS_NV, atoi(getenv("MI_HYPRE_DOT_BLOCKS")))) : vec_grid_cap();
  long long want = ((long long)n + 511) / 512;
  if (want < 1) want = 1;
  if (want > cap) want = cap;
  return (int)want;
}

void dot(const double *x, const double *y, int n, double *out_dev, hipStream_t s) {
  const int g = dot_grid(n);
  double *partials = ctx().red_partials.p;
  prof_begin(PROF_DOT, s);
  hipLaunchKernelGGL(dot_partial_k, dim3(g), dim3(256), 0, s, x, y, n, partials, ctx().red_ticket.p, out_dev);
  prof_end(PROF_DOT, s);
  MI_HIP(hipGetLastError());
}

void axpy_dot(const double *alpha_dev, double scale_, const double *xa, double *y, const double *xd, int n,
              double *out_dev, hipStream_t s) {
  const int g = dot_grid(n);
  double *partials = ctx().red_partials.p;
  prof_begin(PROF_DOT, s);
  hipLaunchKernelGGL(axpy_dot_partial_k, dim3(g), dim3(256), 0, s, alpha_dev, scale_, xa, y, xd, n, partials,
                     ctx().red_ticket.p, out_dev);
  prof_end(PROF_DOT, s);
  MI_HIP(hipGetLastError());
}

// The Gram-Schmidt and update launchers below exist for basis vectors stored as double and as float (Krylov basis
// storage mode 1): one body each, instantiated on the element type, the same grid and the same kernel body either way.
template <class T>
static void mgs_block_pass_t(const T *const *prev, int m_prev, const T *const *next, int m_next, bool last,
                             const double *c_prev, const double *gram_prev, double *h_out, double *w, int n, double *out_dev,
                             double *out_norm, hipStream_t s) {
  MI_REQUIRE(m_prev >= 0 && m_prev <= MGS_NB && m_next >= 0 && m_next <= MGS_NB, "mgs_block_pass: block too large");
  // MGS_NB + 1 partial sums per workgroup in the slots the reductions share
  const int g = std::min(dot_grid(n), RED_MAX_BLOCKS * MASS_NV / (MGS_NB + 1));
  MgsPtrs<MGS_NB, T> P;
  for (int j = 0; j < MGS_NB; j++) {
    P.prev[j] = j < m_prev ? prev[j] : nullptr;
    P.next[j] = (!last && j < m_next) ? next[j] : nullptr;
  }
  double *partials = ctx().red_partials.p;
  prof_begin(PROF_DOT, s);
  if (last)
    hipLaunchKernelGGL((mgs_block_pass_k<MGS_NB, true, T>), dim3(g), dim3(256), 0, s, P, m_prev, 0, c_prev, gram_prev, h_out,
                       w, n, partials, ctx().red_ticket.p, out_dev, out_norm);
  else
    hipLaunchKernelGGL((mgs_block_pass_k<MGS_NB, false, T>), dim3(g), dim3(256), 0, s, P, m_prev, m_next, c_prev, gram_prev,
                       h_out, w, n, partials, ctx().red_ticket.p, out_dev, out_norm);
  prof_end(PROF_DOT, s);
  MI_HIP(hipGetLastError());
}
void mgs_block_pass(const double *const *prev, int m_prev, const double *const *next, int m_next, bool last,
                    const double *c_prev, const double *gram_prev, double *h_out, double *w, int n, double *out_dev,
                    double *out_norm, hipStream_t s) {
  mgs_block_pass_t(prev, m_prev, next, m_next, last, c_prev, gram_prev, h_out, w, n, out_dev, out_norm, s);
}
void mgs_block_pass(const float *const *prev, int m_prev, const float *const *next, int m_next, bool last,
                    const double *c_prev, const double *gram_prev, double *h_out, double *w, int n, double *out_dev,
                    double *out_norm, hipStream_t s) {
  mgs_block_pass_t(prev, m_prev, next, m_next, last, c_prev, gram_prev, h_out, w, n, out_dev, out_norm, s);
}

template <class T>
static void mass_dot_t(const T *const *vecs, int m, const double *w, int n, double *out_dev, hipStream_t s) {
  const int g = vec_grid(n);
  double *partials = ctx().red_partials.p;
  prof_begin(PROF_DOT, s);
  for (int j0 = 0; j0 < m; j0 += MASS_NV) {
    const int mm = std::min(MASS_NV, m - j0);
    MassPtrs<T> P;
    for (int j = 0; j < MASS_NV; j++) P.p[j] = vecs[j0 + (j < mm ? j : 0)];
    hipLaunchKernelGGL(mass_dot_partial_k<T>, dim3(g), dim3(256), 0, s, P, mm, w, n, partials);
    hipLaunchKernelGGL(reduce_final_multi_k, dim3(mm), dim3(256), 0, s, partials, g, out_dev + j0);
  }
  prof_end(PROF_DOT, s);
  MI_HIP(hipGetLastError());
}

void mass_dot(const double *const *vecs, int m, const double *w, int n, double *out_dev, hipStream_t s) {
  mass_dot_t(vecs, m, w, n, out_dev, s);
}
void mass_dot(const float *const *vecs, int m, const double *w, int n, double *out_dev, hipStream_t s) {
  mass_dot_t(vecs, m, w, n, out_dev, s);
}

template <class T>
static void mass_axpy_t(const T *const *vecs, int m, const double *coef_dev, double scale_, double *w, int n,
                        hipStream_t s) {
  if (n == 0) return;
  prof_begin(PROF_AXPY, s);
  for (int j0 = 0; j0 < m; j0 += MASS_NV) {
    const int mm = std::min(MASS_NV, m - j0);
    MassPtrs<T> P;
    for (int j = 0; j < MASS_NV; j++) P.p[j] = vecs[j0 + (j < mm ? j : 0)];
    hipLaunchKernelGGL(mass_axpy_k<T>, dim3(vec_grid(n)), dim3(256), 0, s, P, mm, coef_dev + j0, scale_, w, n);
  }
  prof_end(PROF_AXPY, s);
  MI_HIP(hipGetLastError());
}

void mass_axpy(const double *const *vecs, int m, const double *coef_dev, double scale_, double *w, int n,
               hipStream_t s) {
  mass_axpy_t(vecs, m, coef_dev, scale_, w, n, s);
}
void mass_axpy(const float *const *vecs, int m, const double *coef_dev, double scale_, double *w, int n, hipStream_t s) {
  mass_axpy_t(vecs, m, coef_dev, scale_, w, n, s);
}

template <class T>
static void lin_comb_t(const T *const *vecs, const double *coef_host, int m, bool init, double *w, int n, hipStream_t s) {
  if (n == 0 || m == 0) return;
  prof_begin(PROF_AXPY, s);
  for (int j0 = 0; j0 < m; j0 += MASS_NV) {
    const int mm = std::min(MASS_NV, m - j0);
    MassPtrs<T> P;
    MassCoef C;
    for (int j = 0; j < MASS_NV; j++) {
      P.p[j] = vecs[j0 + (j < mm ? j : 0)];
      C.c[j] = j < mm ? coef_host[j0 + j] : 0.0;
    }
    if (init && j0 == 0)
      hipLaunchKernelGGL((lin_comb_k<true, T>), dim3(vec_grid(n)), dim3(256), 0, s, P, mm, C, w, n);
    else
      hipLaunchKernelGGL((lin_comb_k<false, T>), dim3(vec_grid(n)), dim3(256), 0, s, P, mm, C, w, n);
  }
  prof_end(PROF_AXPY, s);
  MI_HIP(hipGetLastError());
}

void lin_comb(const double *const *vecs, const double *coef_host, int m, bool init, double *w, int n, hipStream_t s) {
  lin_comb_t(vecs, coef_host, m, init, w, n, s);
}
void lin_comb(const float *const *vecs, const double *coef_host, int m, bool init, double *w, int n, hipStream_t s) {
  lin_comb_t(vecs, coef_host, m, init, w, n, s);
}

void axpy(double alpha, const double *x, double *y, int n, hipStream_t s) {
  if (n == 0) return;
  prof_begin(PROF_AXPY, s);
  hipLaunchKernelGGL(axpy_k, dim3(vec_grid(n)), dim3(256), 0, s, (const double *)nullptr, alpha, x, y, n);
  prof_end(PROF_AXPY, s);
  MI_HIP(hipGetLastError());
}
void axpy_dev(const double *alpha_dev, double scale_, const double *x, double *y, int n, hipStream_t s) {
  if (n == 0) return;
  prof_begin(PROF_AXPY, s);
  hipLaunchKernelGGL(axpy_k, dim3(vec_grid(n)), dim3(256), 0, s, alpha_dev, scale_, x, y, n);
  prof_end(PROF_AXPY, s);
  MI_HIP(hipGetLastError());
}
void scale(double alpha, double *x, int n, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(scale_k<0>, dim3(vec_grid(n)), dim3(256), 0, s, (const double *)nullptr, alpha, x, n);
  MI_HIP(hipGetLastError());
}
// x *= 1 / sqrt(*sumsq_dev) as scale_k<1>, and -- first wave of the first workgroup, before it touches x -- the `count`
// doubles at `slots` are stored into host memory the device can write (hipHostMalloc) followed by the number `seq` in a
// flag word, system-scope release: the host reads the Hessenberg column of an Arnoldi step by polling that word, while
// this kernel is still streaming the new basis vector, instead of a copy kernel and a stream synchronisation behind it
// (one idle queue of ~70 us per step, profiles/r03_gaps_512.txt).
__global__ __launch_bounds__(256) void scale_post_k(const double *__restrict__ sumsq_dev, double *__restrict__ x, int n,
                                                    const double *__restrict__ slots, int count,
                                                    double *__restrict__ host_out, unsigned long long *__restrict__ host_flag,
                                                    unsigned long long seq) {
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    for (int j = threadIdx.x; j < count; j += 64)
      __hip_atomic_store(host_out + j, slots[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // the wave's stores are out before the flag
    if (threadIdx.x == 0) __hip_atomic_store(host_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const double t = sumsq_dev[0];
  if (!(t > 0.0)) return;
  const double a = 1.0 / sqrt(t);
  const long long stride = (long long)gridDim.x * 512;
  long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 2;
  for (; i + 1 < n; i += stride) {
    double2 v = *reinterpret_cast<double2 *>(x + i);
    v.x *= a;
    v.y *= a;
    *reinterpret_cast<double2 *>(x + i) = v;
  }
  if (i < n) x[i] *= a;
}
void scale_inv_sqrt_post(const double *sumsq_dev, double *x, int n, const double *slots, int count, double *host_out,
                         unsigned long long *host_flag, unsigned long long seq, hipStream_t s) {
  // (n == 0: a rank without rows still posts)
  hipLaunchKernelGGL(scale_post_k, dim3(n ? vec_grid(n) : 1), dim3(256), 0, s, sumsq_dev, x, n, slots, count, host_out,
                     host_flag, seq);
  MI_HIP(hipGetLastError());
}
void scale_inv_sqrt_dev(const double *sumsq_dev, double *x, int n, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(scale_k<1>, dim3(vec_grid(n)), dim3(256), 0, s, sumsq_dev, 1.0, x, n);
  MI_HIP(hipGetLastError());
}
// ---- the rounding variants of the three scalings (Krylov basis storage modes 1 and 2): the
// product x_i * a of the plain kernel first, then its rounding to float; x_i = rd(x_i * a) = (double)(float)(x_i * a),
// and with SLOT the float itself goes into slot_i (mode 1's basis vector).  Same element-to-lane mapping as the plain
// kernels; the float pair of a lane is one 8-byte store.
template <bool SLOT>
__device__ __forceinline__ void scale_round_body(double a, double *__restrict__ x, float *__restrict__ slot, int n) {
  const long long stride = (long long)gridDim.x * 512;
  long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 2;
  for (; i + 1 < n; i += stride) {
    double2 v = *reinterpret_cast<double2 *>(x + i);
    f2_t f;
    f.x = (float)(v.x * a);
    f.y = (float)(v.y * a);
    v.x = (double)f.x;
    v.y = (double)f.y;
    *reinterpret_cast<double2 *>(x + i) = v;
    if (SLOT) *reinterpret_cast<f2_t *>(slot + i) = f;
  }
  if (i < n) {
    const float f = (float)(x[i] * a);
    x[i] = (double)f;
    if (SLOT) slot[i] = f;
  }
}
// MODE as scale_k
template <int MODE, bool SLOT>
__global__ __launch_bounds__(256) void scale_round_k(const double *__restrict__ sumsq_dev, double scale,
                                                     double *__restrict__ x, float *__restrict__ slot, int n) {
  double a = scale;
  if (MODE == 1) {
    const double t = sumsq_dev[0];
    if (!(t > 0.0)) return;
    a = 1.0 / sqrt(t);
  }
  scale_round_body<SLOT>(a, x, slot, n);
}
// scale_post_k with the rounding: the posting is that kernel's
template <bool SLOT>
__global__ __launch_bounds__(256) void scale_post_round_k(const double *__restrict__ sumsq_dev, double *__restrict__ x,
                                                          float *__restrict__ slot, int n, const double *__restrict__ slots,
                                                          int count, double *__restrict__ host_out,
                                                          unsigned long long *__restrict__ host_flag, unsigned long long seq) {
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    for (int j = threadIdx.x; j < count; j += 64)
      __hip_atomic_store(host_out + j, slots[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    if (threadIdx.x == 0) __hip_atomic_store(host_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const double t = sumsq_dev[0];
  if (!(t > 0.0)) return;
  scale_round_body<SLOT>(1.0 / sqrt(t), x, slot, n);
}
void scale_round(double alpha, double *x, float *slot, int n, hipStream_t s) {
  if (n == 0) return;
  if (slot)
    hipLaunchKernelGGL((scale_round_k<0, true>), dim3(vec_grid(n)), dim3(256), 0, s, (const double *)nullptr, alpha, x, slot, n);
  else
    hipLaunchKernelGGL((scale_round_k<0, false>), dim3(vec_grid(n)), dim3(256), 0, s, (const double *)nullptr, alpha, x, slot, n);
  MI_HIP(hipGetLastError());
}
void scale_inv_sqrt_dev_round(const double *sumsq_dev, double *x, float *slot, int n, hipStream_t s) {
  if (n == 0) return;
  if (slot)
    hipLaunchKernelGGL((scale_round_k<1, true>), dim3(vec_grid(n)), dim3(256), 0, s, sumsq_dev, 1.0, x, slot, n);
  else
    hipLaunchKernelGGL((scale_round_k<1, false>), dim3(vec_grid(n)), dim3(256), 0, s, sumsq_dev, 1.0, x, slot, n);
  MI_HIP(hipGetLastError());
}
void scale_inv_sqrt_post_round(const double *sumsq_dev, double *x, float *slot, int n, const double *slots, int count,
                               double *host_out, unsigned long long *host_flag, unsigned long long seq, hipStream_t s) {
  const dim3 g(n ? vec_grid(n) : 1);
  if (slot)
    hipLaunchKernelGGL(scale_post_round_k<true>, g, dim3(256), 0, s, sumsq_dev, x, slot, n, slots, count, host_out, host_flag, seq);
  else
    hipLaunchKernelGGL(scale_post_round_k<false>, g, dim3(256), 0, s, sumsq_dev, x, slot, n, slots, count, host_out, host_flag, seq);
  MI_HIP(hipGetLastError());
}
// Tabulation of a linear map column by column inside ONE captured graph (BoomerAMG::tabulate_cycle): the column number
// lives in device memory, so that every replay of the graph is the same sequence of launches.
//   tab_unit_k : e = unit vector number *col (the previous column's 1 is cleared)
//   tab_store_k: column *col of Bt = u, then ++*col (one workgroup: n is at most a few thousand)
__global__ __launch_bounds__(64) void tab_unit_k(double *__restrict__ e, const int *__restrict__ col) {
  if (threadIdx.x == 0) {
    const int j = *col;
    if (j > 0) e[j - 1] = 0.0;
    e[j] = 1.0;
  }
}
__global__ __launch_bounds__(256) void tab_store_k(double *__restrict__ Bt, const double *__restrict__ u, int n, int *__restrict__ col) {
  const int j = *col;
  for (int i = threadIdx.x; i < n; i += 256) Bt[(size_t)j * (size_t)n + i] = u[i];
  __syncthreads();
  if (threadIdx.x == 0) *col = j + 1;
}
// test support (HYPRE_MI_ArenaSelfTest): bytes of p[0..n) that differ from `tag`: their number and the first and last offset
__global__ __launch_bounds__(256) void bytes_differ_k(const unsigned char *__restrict__ p, size_t n, unsigned char tag,
                                                      unsigned long long *__restrict__ out) {
  size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
  unsigned long long cnt = 0, first = ~0ull, last = 0;
  for (; i < n; i += (size_t)gridDim.x * 256)
    if (p[i] != tag) {
      cnt++;
      if (i < first) first = i;
      if (i > last) last = i;
    }
  if (cnt) {
    atomicAdd(out, cnt);
    atomicMin(out + 1, first);
    atomicMax(out + 2, last);
  }
}
__global__ __launch_bounds__(256) void fill_bytes_k(unsigned char *__restrict__ p, size_t n, unsigned char tag) {
  size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * 256) p[i] = tag;
}
void fill_bytes(unsigned char *p, size_t n, unsigned char tag, hipStream_t s) {
  hipLaunchKernelGGL(fill_bytes_k, dim3(2048), dim3(256), 0, s, p, n, tag);
  MI_HIP(hipGetLastError());
}
void bytes_differ(const unsigned char *p, size_t n, unsigned char tag, unsigned long long *out3, hipStream_t s) {
  hipLaunchKernelGGL(bytes_differ_k, dim3(2048), dim3(256), 0, s, p, n, tag, out3);
  MI_HIP(hipGetLastError());
}
void tab_unit(double *e, const int *col, hipStream_t s) {
  hipLaunchKernelGGL(tab_unit_k, dim3(1), dim3(64), 0, s, e, col);
  MI_HIP(hipGetLastError());
}
void tab_store(double *Bt, const double *u, int n, int *col, hipStream_t s) {
  hipLaunchKernelGGL(tab_store_k, dim3(1), dim3(256), 0, s, Bt, u, n, col);
  MI_HIP(hipGetLastError());
}
namespace {
__global__ void load_module_k(int *p) {
  if (p) *p = 0;
}
}  // namespace
void load_device_code(hipStream_t s) {  // see sk::load_device_code
  load_module_k<<<1, 1, 0, s>>>(nullptr);
  MI_HIP(hipGetLastError());
}
void fill(double *x, int n, double v, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(fill_k, dim3(vec_grid(n)), dim3(256), 0, s, x, n, v);
  MI_HIP(hipGetLastError());
}
void copy(const double *x, double *y, int n, hipStream_t s) {
  if (n == 0 || x == y) return;
  MI_HIP(hipMemcpyAsync(y, x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
}
void gather2(const double *lo, const double *hi, int split, const int *map, double *out, int n, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(gather2_k, dim3((n + 255) / 256), dim3(256), 0, s, lo, hi, split, map, out, n);
  MI_HIP(hipGetLastError());
}
void gather(const double *x, const int *map, double *out, int n, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(gather_k, dim3((n + 255) / 256), dim3(256), 0, s, x, map, out, n);
  MI_HIP(hipGetLastError());
}
void scatter_set(double *x, const int *idx, const double *vals, int n, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(scatter_k<0>, dim3((n + 255) / 256), dim3(256), 0, s, x, idx, vals, n);
  MI_HIP(hipGetLastError());
}
void scatter_add(double *x, const int *idx, const double *vals, int n, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(scatter_k<1>, dim3((n + 255) / 256), dim3(256), 0, s, x, idx, vals, n);
  MI_HIP(hipGetLastError());
}
void two_stage_first(const double *r, const double *d, double *z, double *u, int n, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(two_stage_first_k, dim3((n + 255) / 256), dim3(256), 0, s, n, r, d, z, u);
}
void two_stage_lower(const DevCSR &A, const double *d, const double *zin, double sign, double *zout, double *u,
                     hipStream_t s) {
  if (A.nrows <= 0) return;
  MI_REQUIRE(!A.big(), "two-stage Gauss-Seidel: operators with 2^31 entries or more are not supported");
  if (A.a32.p)
    hipLaunchKernelGGL(two_stage_lower_k<float>, dim3((A.nrows + 255) / 256), dim3(256), 0, s, A.nrows, A.ia.p, A.ja.p,
                       A.a32.p, d, zin, sign, zout, u);
  else
    hipLaunchKernelGGL(two_stage_lower_k<double>, dim3((A.nrows + 255) / 256), dim3(256), 0, s, A.nrows, A.ia.p, A.ja.p,
                       A.a.p, d, zin, sign, zout, u);
}

// ---------------------------------------------------------------- fp32 value storage
namespace {
// *flag = 1 when a finite non-zero value lies outside the range of normal floats
__global__ __launch_bounds__(256) void float_range_k(long long n, const double *__restrict__ a, int *__restrict__ flag) {
  const long long stride = (long long)gridDim.x * 256;
  int bad = 0;
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n; k += stride) bad |= !fits_float(a[k]);
  if (bad) *flag = 1;  // every writer stores the same value
}
__global__ __launch_bounds__(256) void round_to_float_k(long long n, double *__restrict__ a) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n; k += stride) a[k] = (double)(float)a[k];
}
__global__ __launch_bounds__(256) void narrow_k(long long n, const double *__restrict__ a, float *__restrict__ out) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n; k += stride) out[k] = (float)a[k];
}
__global__ __launch_bounds__(256) void widen_k(long long n, const float *__restrict__ a, double *__restrict__ out) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n; k += stride) out[k] = (double)a[k];
}
unsigned value_grid(long long n) { return (unsigned)std::max<long long>(1, std::min<long long>(4096, (n + 255) / 256)); }
}  // namespace

bool values_fit_float(const double *a, long long n, hipStream_t s) {
  if (n <= 0) return true;
  DVec<int> flag(1);
  MI_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), s));
  hipLaunchKernelGGL(float_range_k, dim3(value_grid(n)), dim3(256), 0, s, n, a, flag.p);
  MI_HIP(hipGetLastError());
  int bad = 0;
  d2h(&bad, flag.p, sizeof(int), s);
  MI_HIP(hipStreamSynchronize(s));
  return bad == 0;
}

void round_values(double *a, long long n, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(round_to_float_k, dim3(value_grid(n)), dim3(256), 0, s, n, a);
  MI_HIP(hipGetLastError());
}

void narrow_values(DevCSR &A, int mode, hipStream_t s) {
  MI_REQUIRE(mode == 1 || mode == 2, "value storage: mode 1 or 2");
  MI_REQUIRE(!A.a32.p, "value storage: the operator is narrowed already");
  A.value_kind = mode;
  const bool dict = A.value_format() == ValueFormat::DICT;
  if (dict) round_values(A.vlut.p, 256, s);  // the table and the fp64 array kept beside it: the same values
  if (dict || mode == 2) {
    round_values(A.a.p, A.nnz, s);
  } else {
    A.a32.alloc((size_t)A.nnz);
    hipLaunchKernelGGL(narrow_k, dim3(value_grid(A.nnz)), dim3(256), 0, s, (long long)A.nnz, A.a.p, A.a32.p);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(s));
    A.a.release();
  }
}

const double *fp64_values(const DevCSR &A, DVec<double> &tmp, hipStream_t s) {
  if (!A.a32.p) return A.a.p;
  tmp.alloc((size_t)A.nnz);
  if (A.nnz) hipLaunchKernelGGL(widen_k, dim3(value_grid(A.nnz)), dim3(256), 0, s, (long long)A.nnz, A.a32.p, tmp.p);
  MI_HIP(hipGetLastError());
  return tmp.p;
}

long long value_stream_bytes(const DevCSR &A) {
  long long b = 0;
  if (A.a.p) b += (long long)(A.a.n + 2) * 8;
  if (A.a32.p) b += (long long)(A.a32.n + 2) * 4;
  if (A.vidx.p) b += (long long)(A.vidx.n + 2);
  if (A.vlut.p) b += (long long)(A.vlut.n + 2) * 8;
  return b;
}

void ipc_exchange(const IpcBatch &b, unsigned long long spin_limit, int *error_flag, hipStream_t s) {
  int nb = 0;
  for (int i = 0; i < b.n; i++) nb += b.t[i].nblocks;
  if (nb == 0) return;
  hipLaunchKernelGGL(ipc_exchange_k, dim3((unsigned)nb), dim3(1024), 0, s, b, spin_limit, error_flag);
  MI_HIP(hipGetLastError());
}

void ipc_allreduce(const IpcAllreduce &a, unsigned long long spin_limit, int *error_flag, hipStream_t s) {
  hipLaunchKernelGGL(ipc_allreduce_k, dim3(1), dim3(64), 0, s, a, spin_limit, error_flag);
  MI_HIP(hipGetLastError());
}

void ipc_poison(double *buf, int count, const int *error_flag, hipStream_t s) {
  // (larger counts: the first 64 values are enough to turn every sum into NaN)
  hipLaunchKernelGGL(ipc_poison_k, dim3(1), dim3(64), 0, s, buf, std::min(count, 64), error_flag);
  MI_HIP(hipGetLastError());
}

void dense_matvec_t(const double *Mt, const double *f, double *u, int n, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(dense_matvec_t_k, dim3((n + 15) / 16), dim3(1024), 0, s, Mt, f, u, n);
  MI_HIP(hipGetLastError());
}

void dense_matvec(const double *M, const double *f, double *u, int n, int m, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(dense_matvec_k, dim3((n + 255) / 256), dim3(256), 0, s, M, f, u, n, m);
  MI_HIP(hipGetLastError());
}

}  // namespace k
}  // namespace mi
