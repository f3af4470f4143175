// IJ assembly on the device.  See ij_assembly.hpp and DESIGN.md section 4.
//
// Determinism: the only atomics are integer ones (row counts, bucket cursors, list cursors, status words).  The one
// place where they decide an order -- the position of an entry inside its row's bucket of the counting sort -- is
// undone by the per-row sort on (column, submission index), a total order.  Every value is folded by ONE thread in
// submission order with a plain +, as assemble_parcsr does.
#include "ij_assembly.hpp"

#include <algorithm>
#include <cstring>

namespace mi {
namespace ij {
namespace {

constexpr int BLK = 256;
constexpr long long MAX_GRID = 1 << 20;
using ull = unsigned long long;

inline unsigned grid_for(long long n) {
  long long b = (n + BLK - 1) / BLK;
  return (unsigned)std::max<long long>(1, std::min(b, MAX_GRID));
}
#define IJ_GRID_STRIDE(i, n) \
  for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < (n); i += (long long)gridDim.x * BLK)

// status words of one assembly
enum { ST_BAD = 0, ST_UNORDERED = 1, ST_MAXLEN = 2, ST_NWAVE = 3, ST_NBLOCK = 4, ST_NLONG = 5, ST_WORDS = 8 };

__global__ __launch_bounds__(BLK) void fill_k(double *__restrict__ x, long long n, double v) {
  IJ_GRID_STRIDE(i, n) x[i] = v;
}

// ---------------------------------------------------------------- ncols / row_indexes form
__global__ __launch_bounds__(BLK) void clamp_counts_k(int n, const int *__restrict__ nc, int *__restrict__ out) {
  IJ_GRID_STRIDE(i, n) out[i] = nc[i] > 0 ? nc[i] : 0;
}
__global__ __launch_bounds__(BLK) void expand_rows_k(int n, const int *__restrict__ cnt, const long long *__restrict__ off,
                                                     const gidx *__restrict__ rows, const int *__restrict__ row_indexes,
                                                     const gidx *__restrict__ cols, const double *__restrict__ vals,
                                                     gidx *__restrict__ orow, gidx *__restrict__ ocol,
                                                     double *__restrict__ oval) {
  IJ_GRID_STRIDE(i, n) {
    const long long o = off[i], src = row_indexes ? (long long)row_indexes[i] : o;
    const gidx r = rows[i];
    for (int k = 0; k < cnt[i]; k++) {
      orow[o + k] = r;
      ocol[o + k] = cols[src + k];
      oval[o + k] = vals[src + k];
    }
  }
}

// ---------------------------------------------------------------- step 1: ownership, order, row pointers
__global__ __launch_bounds__(BLK) void validate_k(long long E, const gidx *__restrict__ R, gidx ilower, gidx iupper,
                                                  ull *__restrict__ st) {
  IJ_GRID_STRIDE(k, E) {
    const gidx r = R[k];
    if (r < ilower || r > iupper) atomicMin(&st[ST_BAD], (ull)k);
    if (k > 0 && R[k - 1] > r) atomicOr(&st[ST_UNORDERED], 1ull);
  }
}
// a batch that starts below the last row of the one before it breaks the row order
__global__ void batch_edge_k(const gidx *__restrict__ prev_last, const gidx *__restrict__ first, ull *__restrict__ st) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && *first < *prev_last) atomicOr(&st[ST_UNORDERED], 1ull);
}
// rows non-decreasing: ia[q] = first position of an entry of a row >= q
__global__ __launch_bounds__(BLK) void boundaries_k(long long E, const gidx *__restrict__ R, gidx ilower, int nrows,
                                                    long long *__restrict__ ia) {
  IJ_GRID_STRIDE(k, E) {
    const long long r = R[k] - ilower, prev = k > 0 ? (long long)(R[k - 1] - ilower) : -1;
    for (long long q = prev + 1; q <= r; q++) ia[q] = k;
    if (k == E - 1)
      for (long long q = r + 1; q <= nrows; q++) ia[q] = E;
  }
}
__global__ __launch_bounds__(BLK) void count_rows_k(long long E, const gidx *__restrict__ R, gidx ilower, int *__restrict__ cnt) {
  IJ_GRID_STRIDE(k, E) atomicAdd(&cnt[R[k] - ilower], 1);
}
// bucket positions by integer atomics (any order inside a bucket); sub[p] = submission index of the entry placed at p
__global__ __launch_bounds__(BLK) void scatter_rows_k(long long E, const gidx *__restrict__ R, gidx ilower, ull *__restrict__ pos,
                                                      long long *__restrict__ sub) {
  IJ_GRID_STRIDE(k, E) {
    const ull p = atomicAdd(&pos[R[k] - ilower], 1ull);
    sub[p] = k;
  }
}
__global__ __launch_bounds__(BLK) void gather_entries_k(long long E, const long long *__restrict__ sub, const gidx *__restrict__ cj,
                                                        const double *__restrict__ cv, gidx *__restrict__ oj,
                                                        double *__restrict__ ov) {
  IJ_GRID_STRIDE(p, E) {
    const long long k = sub[p];
    oj[p] = cj[k];
    ov[p] = cv[k];
  }
}

// ---------------------------------------------------------------- step 2: per-row sort and fold
// class of a row: 0 columns strictly ascending (nothing to do), 1 one wave, 2 one block, 3 any length
__global__ __launch_bounds__(BLK) void classify_k(int nrows, const long long *__restrict__ ia, const gidx *__restrict__ cj,
                                                  unsigned char *__restrict__ cls, int *__restrict__ rowlen,
                                                  ull *__restrict__ st) {
  IJ_GRID_STRIDE(i, nrows) {
    const long long s = ia[i], len = ia[i + 1] - s;
    bool sorted = true;
    for (long long k = 1; k < len; k++)
      if (cj[s + k] <= cj[s + k - 1]) {
        sorted = false;
        break;
      }
    rowlen[i] = (int)(len < 2147483647LL ? len : 2147483647LL);
    const int c = sorted ? 0 : len <= SORT_WAVE_CAP ? 1 : len <= SORT_LDS_CAP ? 2 : 3;
    cls[i] = (unsigned char)c;
    if (c) atomicAdd(&st[ST_NWAVE + c - 1], 1ull);
    if (len > SORT_WAVE_CAP) atomicMax(&st[ST_MAXLEN], (ull)len);
  }
}
// lists of the rows of each class (any order: the rows are independent)
__global__ __launch_bounds__(BLK) void list_rows_k(int nrows, const unsigned char *__restrict__ cls, int *__restrict__ l1,
                                                   int *__restrict__ l2, int *__restrict__ l3, unsigned *__restrict__ cur) {
  IJ_GRID_STRIDE(i, nrows) {
    const int c = cls[i];
    if (c == 0) continue;
    const unsigned p = atomicAdd(&cur[c - 1], 1u);
    (c == 1 ? l1 : c == 2 ? l2 : l3)[p] = (int)i;
  }
}

__global__ __launch_bounds__(BLK) void gather_lengths_k(int n, const int *__restrict__ list, const int *__restrict__ rowlen,
                                                        int *__restrict__ out) {
  IJ_GRID_STRIDE(q, n) out[q] = rowlen[list[q]];
}

// Number of set flags among the flags of the lanes before this one plus its own (inclusive), over the workgroup of T
// lanes; *total = the workgroup's count.  sc: T ints of LDS.  Every lane calls it.
template <int T>
__device__ __forceinline__ int block_count_inclusive(int flag, int *sc, int *total) {
  sc[threadIdx.x] = flag;
  __syncthreads();
  for (int d = 1; d < T; d <<= 1) {
    const int add = ((int)threadIdx.x >= d) ? sc[threadIdx.x - d] : 0;
    __syncthreads();
    sc[threadIdx.x] += add;
    __syncthreads();
  }
  const int mine = sc[threadIdx.x];
  *total = sc[T - 1];
  __syncthreads();
  return mine;
}

// Set or Add of the entry with submission index `sub`: the batch that holds it (boff: nb + 1 offsets)
__device__ __forceinline__ bool add_of(long long sub, int nb, const long long *__restrict__ boff,
                                       const unsigned char *__restrict__ badd, bool uniform) {
  if (nb == 0) return uniform;
  int lo = 0, hi = nb - 1;  // largest b with boff[b] <= sub
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (boff[mid] <= sub)
      lo = mid;
    else
      hi = mid - 1;
  }
  return badd[lo] != 0;
}

// One row per workgroup of T lanes, the row in LDS: rank of every entry under (column, submission index) by
// comparison with all others, placement, then one lane per run of equal columns folds it in submission order.
template <int T, int CAP>
__global__ __launch_bounds__(T) void sort_fold_lds_k(int nlist, const int *__restrict__ list, const long long *__restrict__ ia,
                                                     gidx *__restrict__ cj, double *__restrict__ cv,
                                                     const long long *__restrict__ sub, int nb,
                                                     const long long *__restrict__ boff, const unsigned char *__restrict__ badd,
                                                     bool uniform, int *__restrict__ rowlen) {
  __shared__ gidx ucol[CAP], scol[CAP];
  __shared__ long long usub[CAP];
  __shared__ double uval[CAP], sval[CAP];
  __shared__ int opos[CAP];
  __shared__ unsigned char sadd[CAP];
  __shared__ int scan[T];
  if ((int)blockIdx.x >= nlist) return;
  const int row = list[blockIdx.x];
  const long long s = ia[row];
  const int len = (int)(ia[row + 1] - s);
  if (len > CAP) return;  // (the lists are built by length: never taken)
  for (int e = threadIdx.x; e < len; e += T) {
    ucol[e] = cj[s + e];
    usub[e] = sub ? sub[s + e] : s + e;
    uval[e] = cv[s + e];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < len; e += T) {
    const gidx c = ucol[e];
    const long long q = usub[e];
    int rank = 0;
    for (int j = 0; j < len; j++) rank += (ucol[j] < c || (ucol[j] == c && usub[j] < q)) ? 1 : 0;
    scol[rank] = c;
    sval[rank] = uval[e];
    sadd[rank] = add_of(q, nb, boff, badd, uniform) ? 1 : 0;
  }
  __syncthreads();
  // output position of every sorted entry = runs of equal columns begun before it: chunks of T flags, scanned
  int m = 0;
  for (int base = 0; base < len; base += T) {
    const int r = base + (int)threadIdx.x;
    const int head = (r < len && (r == 0 || scol[r] != scol[r - 1])) ? 1 : 0;
    int chunk = 0;
    const int inc = block_count_inclusive<T>(head, scan, &chunk);
    if (r < len) opos[r] = m + inc - 1;
    m += chunk;
  }
  if (threadIdx.x == 0) rowlen[row] = m;
  __syncthreads();
  for (int r = threadIdx.x; r < len; r += T) {
    if (r > 0 && scol[r] == scol[r - 1]) continue;
    double v = sval[r];
    for (int j = r + 1; j < len && scol[j] == scol[r]; j++) v = sadd[j] ? v + sval[j] : sval[j];
    cj[s + opos[r]] = scol[r];
    cv[s + opos[r]] = v;
  }
}

// The same for a row of any length: the sorted copy lives in global scratch (toff[li]: the row's offset there)
__global__ __launch_bounds__(BLK) void sort_fold_long_k(int nlist, const int *__restrict__ list, const long long *__restrict__ toff,
                                                        const long long *__restrict__ ia, gidx *__restrict__ cj,
                                                        double *__restrict__ cv, const long long *__restrict__ sub, int nb,
                                                        const long long *__restrict__ boff, const unsigned char *__restrict__ badd,
                                                        bool uniform, gidx *__restrict__ tcol, double *__restrict__ tval,
                                                        unsigned char *__restrict__ tadd, long long *__restrict__ tpos,
                                                        int *__restrict__ rowlen) {
  if ((int)blockIdx.x >= nlist) return;
  const int row = list[blockIdx.x];
  const long long s = ia[row], len = ia[row + 1] - s, t0 = toff[blockIdx.x];
  for (long long e = threadIdx.x; e < len; e += BLK) {
    const gidx c = cj[s + e];
    const long long q = sub ? sub[s + e] : s + e;
    long long rank = 0;
    for (long long j = 0; j < len; j++) {
      const gidx cc = cj[s + j];
      const long long qq = sub ? sub[s + j] : s + j;
      rank += (cc < c || (cc == c && qq < q)) ? 1 : 0;
    }
    tcol[t0 + rank] = c;
    tval[t0 + rank] = cv[s + e];
    tadd[t0 + rank] = add_of(q, nb, boff, badd, uniform) ? 1 : 0;
  }
  __syncthreads();
  __shared__ int scan[BLK];
  long long m = 0;
  for (long long base = 0; base < len; base += BLK) {
    const long long r = base + threadIdx.x;
    const int head = (r < len && (r == 0 || tcol[t0 + r] != tcol[t0 + r - 1])) ? 1 : 0;
    int chunk = 0;
    const int inc = block_count_inclusive<BLK>(head, scan, &chunk);
    if (r < len) tpos[t0 + r] = m + inc - 1;
    m += chunk;
  }
  if (threadIdx.x == 0) rowlen[row] = (int)m;
  __syncthreads();
  for (long long r = threadIdx.x; r < len; r += BLK) {
    if (r > 0 && tcol[t0 + r] == tcol[t0 + r - 1]) continue;
    double v = tval[t0 + r];
    for (long long j = r + 1; j < len && tcol[t0 + j] == tcol[t0 + r]; j++) v = tadd[t0 + j] ? v + tval[t0 + j] : tval[t0 + j];
    cj[s + tpos[t0 + r]] = tcol[t0 + r];
    cv[s + tpos[t0 + r]] = v;
  }
}

// ---------------------------------------------------------------- step 3: diag / halo split
__global__ __launch_bounds__(BLK) void count_split_k(int nrows, const long long *__restrict__ ia, const int *__restrict__ rowlen,
                                                     const gidx *__restrict__ cj, gidx jlower, gidx jupper,
                                                     int *__restrict__ nd, int *__restrict__ no) {
  IJ_GRID_STRIDE(i, nrows) {
    const long long s = ia[i];
    const int m = rowlen[i];
    int d = 0;
    for (int k = 0; k < m; k++) {
      const gidx c = cj[s + k];
      d += (c >= jlower && c <= jupper) ? 1 : 0;
    }
    nd[i] = d;
    no[i] = m - d;
  }
}
__global__ __launch_bounds__(BLK) void write_split_k(int nrows, const long long *__restrict__ ia, const int *__restrict__ rowlen,
                                                     const gidx *__restrict__ cj, const double *__restrict__ cv, gidx jlower,
                                                     gidx jupper, const long long *__restrict__ dia,
                                                     const long long *__restrict__ oia, int *__restrict__ dja,
                                                     double *__restrict__ da, gidx *__restrict__ ogid, double *__restrict__ oa) {
  IJ_GRID_STRIDE(i, nrows) {
    const long long s = ia[i];
    const int m = rowlen[i];
    long long pd = dia[i], po = oia[i];
    for (int k = 0; k < m; k++) {
      const gidx c = cj[s + k];
      const double v = cv[s + k];
      if (c >= jlower && c <= jupper) {
        dja[pd] = (int)(c - jlower);
        da[pd] = v;
        pd++;
      } else {
        ogid[po] = c;
        oa[po] = v;
        po++;
      }
    }
  }
}

// ---------------------------------------------------------------- vector indices
__global__ __launch_bounds__(BLK) void local_ids_k(int n, const gidx *__restrict__ idx, gidx jlower, gidx jupper,
                                                   int *__restrict__ loc, ull *__restrict__ st) {
  IJ_GRID_STRIDE(i, n) {
    const gidx g = idx[i];
    if (g < jlower || g > jupper) {
      atomicMin(&st[0], (ull)i);
      loc[i] = 0;
    } else {
      loc[i] = (int)(g - jlower);
    }
  }
}

// ---------------------------------------------------------------- synthetic generator
__device__ __forceinline__ int lap_row_nnz(gidx row, int nx, int ny, int nz, int stencil) {
  const int x = (int)(row % nx), y = (int)((row / nx) % ny), z = (int)(row / ((gidx)nx * ny));
  const int cx = 1 + (x > 0) + (x < nx - 1), cy = 1 + (y > 0) + (y < ny - 1), cz = 1 + (z > 0) + (z < nz - 1);
  return (stencil == 27) ? cx * cy * cz : 1 + (cx - 1) + (cy - 1) + (cz - 1);
}
__global__ __launch_bounds__(BLK) void lap_count_k(long long nloc, gidx ilower, int nx, int ny, int nz, int stencil,
                                                   int *__restrict__ cnt) {
  IJ_GRID_STRIDE(i, nloc) cnt[i] = lap_row_nnz(ilower + i, nx, ny, nz, stencil);
}
__global__ __launch_bounds__(BLK) void lap_fill_k(long long nloc, gidx ilower, int nx, int ny, int nz, int stencil,
                                                  const long long *__restrict__ off, gidx *__restrict__ rows,
                                                  gidx *__restrict__ cols, double *__restrict__ vals, double *__restrict__ rhs) {
  const double dv = (stencil == 27) ? 26.0 : 6.0;
  IJ_GRID_STRIDE(i, nloc) {
    const gidx row = ilower + i;
    const int x = (int)(row % nx), y = (int)((row / nx) % ny), z = (int)(row / ((gidx)nx * ny));
    long long q = off[i];
    double sum = 0.0;
    for (int dz = -1; dz <= 1; dz++)
      for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
          if (stencil == 7 && ((dx != 0) + (dy != 0) + (dz != 0) > 1)) continue;
          const int X = x + dx, Y = y + dy, Z = z + dz;
          if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) continue;
          const gidx col = X + (gidx)nx * (Y + (gidx)ny * Z);
          const double v = (col == row) ? dv : -1.0;
          rows[q] = row;
          cols[q] = col;
          vals[q] = v;
          sum += v;
          q++;
        }
    rhs[i] = sum;
  }
}

// copy between device arrays, ordered against the caller's legacy-stream work and complete on return
void copy_in(void *dst, const void *src, size_t bytes) {
  if (!bytes) return;
  MI_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, nullptr));
  MI_HIP(hipStreamSynchronize(nullptr));
}

void read_status(const DVec<ull> &st, ull *h, hipStream_t s) {
  d2h(h, st.p, ST_WORDS * sizeof(ull), s);
  MI_HIP(hipStreamSynchronize(s));
}

}  // namespace

Counters &counters() {
  static Counters c;
  return c;
}

bool device_assembly_enabled() {
  static const bool on = !(getenv("MI_HYPRE_DEVICE_ASSEMBLY") && atoi(getenv("MI_HYPRE_DEVICE_ASSEMBLY")) == 0);
  return on;
}

void stage_coo(const gidx *rows, const gidx *cols, const double *vals, int64_t n, bool add, DevBatch &out) {
  ensure_init();
  out.n = n;
  out.add = add;
  out.rows.alloc((size_t)n);
  out.cols.alloc((size_t)n);
  out.vals.alloc((size_t)n);
  copy_in(out.rows.p, rows, (size_t)n * sizeof(gidx));
  copy_in(out.cols.p, cols, (size_t)n * sizeof(gidx));
  copy_in(out.vals.p, vals, (size_t)n * sizeof(double));
}

void stage_ncols(int nrows, const int *ncols, const gidx *rows, const int *row_indexes, const gidx *cols,
                 const double *vals, bool add, DevBatch &out) {
  ensure_init();
  hipStream_t s = ctx().stream;
  MI_HIP(hipStreamSynchronize(nullptr));  // the caller's arrays are final before the library stream reads them
  DVec<int> cnt((size_t)nrows);
  DVec<long long> off((size_t)nrows + 1);
  clamp_counts_k<<<grid_for(nrows), BLK, 0, s>>>(nrows, ncols, cnt.p);
  sk::exclusive_scan_counts(cnt.p, off.p, nrows, s);
  long long total = 0;
  d2h(&total, off.p + nrows, sizeof(long long), s);
  MI_HIP(hipStreamSynchronize(s));
  out.n = total;
  out.add = add;
  out.rows.alloc((size_t)total);
  out.cols.alloc((size_t)total);
  out.vals.alloc((size_t)total);
  if (total)
    expand_rows_k<<<grid_for(nrows), BLK, 0, s>>>(nrows, cnt.p, off.p, rows, row_indexes, cols, vals, out.rows.p, out.cols.p,
                                                  out.vals.p);
  MI_HIP(hipGetLastError());
  MI_HIP(hipStreamSynchronize(s));
}

void fill_values(DevBatch &b, double v) {
  if (!b.n) return;
  hipStream_t s = ctx().stream;
  fill_k<<<grid_for(b.n), BLK, 0, s>>>(b.vals.p, b.n, v);
  MI_HIP(hipGetLastError());
  MI_HIP(hipStreamSynchronize(s));
}

void assemble_parcsr_device(Comm &comm, gidx ilower, gidx iupper, gidx jlower, gidx jupper, std::vector<DevBatch> &batches,
                            ParCSR &out, sk::DCsr &diag) {
  ensure_init();
  hipStream_t s = ctx().stream;
  const double t_begin = wall_time();
  require_int32_block(iupper - ilower + 1, 0, "IJMatrixAssemble");
  const int nrows = (int)(iupper - ilower + 1);
  const int ncols_loc = (int)(jupper - jlower + 1);
  int64_t E = 0;
  for (auto &b : batches) E += b.n;

  // the entries in submission order: one batch as it is, several concatenated (each released once copied)
  DVec<gidx> R, cj;
  DVec<double> cv;
  std::vector<long long> boff_h;
  std::vector<unsigned char> badd_h;
  bool uniform_add = batches.empty() ? false : batches.front().add, mixed = false;
  for (auto &b : batches) mixed = mixed || (b.add != uniform_add);
  if (mixed) {
    long long o = 0;
    for (auto &b : batches) {
      if (!b.n) continue;
      boff_h.push_back(o);
      badd_h.push_back(b.add ? 1 : 0);
      o += b.n;
    }
    boff_h.push_back(o);
  }
  // the first pass only reads the batches: a refusal leaves them as they were
  DVec<ull> st(ST_WORDS);
  {
    ull init[ST_WORDS] = {~0ull, 0, 0, 0, 0, 0, 0, 0};
    MI_HIP(hipMemcpyAsync(st.p, init, sizeof(init), hipMemcpyHostToDevice, s));
    MI_HIP(hipStreamSynchronize(s));
  }
  ull h[ST_WORDS];
  {
    // per batch: ownership and order inside it; across batches: the first row of one against the last of the one before
    DVec<ull> stb(ST_WORDS);
    const gidx *prev_last = nullptr;
    bool unordered = false;
    for (auto &b : batches) {
      if (!b.n) continue;
      ull init[ST_WORDS] = {~0ull, 0, 0, 0, 0, 0, 0, 0};
      MI_HIP(hipMemcpyAsync(stb.p, init, sizeof(init), hipMemcpyHostToDevice, s));
      MI_HIP(hipStreamSynchronize(s));
      if (prev_last) batch_edge_k<<<1, 64, 0, s>>>(prev_last, b.rows.p, stb.p);
      prev_last = b.rows.p + (b.n - 1);
      validate_k<<<grid_for(b.n), BLK, 0, s>>>(b.n, b.rows.p, ilower, iupper, stb.p);
      MI_HIP(hipGetLastError());
      read_status(stb, h, s);
      if (h[ST_BAD] != ~0ull) {
        // the one row id that travels to the host: the message names it, as the host path's does
        gidx bad = 0;
        d2h(&bad, b.rows.p + h[ST_BAD], sizeof(gidx), s);
        MI_HIP(hipStreamSynchronize(s));
        fail(4, "IJMatrix: row " + std::to_string(bad) + " is not owned by this rank");
      }
      unordered = unordered || h[ST_UNORDERED] != 0;
    }
    h[ST_UNORDERED] = unordered ? 1 : 0;
  }
  const bool in_row_order = E > 0 && h[ST_UNORDERED] == 0;

  if (batches.size() == 1) {
    R = std::move(batches[0].rows);
    cj = std::move(batches[0].cols);
    cv = std::move(batches[0].vals);
  } else if (E > 0) {
    // one array at a time, every batch's part released once copied: the peak is the staged 24 B per entry plus
    // one concatenated array of 8 B per entry, not two whole copies
    auto concat = [&](auto &dst, auto part) {
      dst.alloc((size_t)E);
      long long o = 0;
      for (auto &b : batches) {
        auto &src = part(b);
        if (b.n) {
          MI_HIP(hipMemcpyAsync(dst.p + o, src.p, (size_t)b.n * sizeof(*dst.p), hipMemcpyDeviceToDevice, s));
          MI_HIP(hipStreamSynchronize(s));
        }
        o += b.n;
        src.release();
      }
    };
    concat(R, [](DevBatch &b) -> DVec<gidx> & { return b.rows; });
    concat(cj, [](DevBatch &b) -> DVec<gidx> & { return b.cols; });
    concat(cv, [](DevBatch &b) -> DVec<double> & { return b.vals; });
  }
  batches.clear();

  DVec<long long> ia((size_t)nrows + 1);
  DVec<long long> sub;  // submission index of every entry (counting sort only; empty: the position itself)
  if (E == 0) {
    MI_HIP(hipMemsetAsync(ia.p, 0, ((size_t)nrows + 1) * sizeof(long long), s));
  } else if (in_row_order) {
    boundaries_k<<<grid_for(E), BLK, 0, s>>>(E, R.p, ilower, nrows, ia.p);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(s));
    R.release();
  } else {
    DVec<int> cnt((size_t)nrows);
    MI_HIP(hipMemsetAsync(cnt.p, 0, (size_t)nrows * sizeof(int), s));
    count_rows_k<<<grid_for(E), BLK, 0, s>>>(E, R.p, ilower, cnt.p);
    sk::exclusive_scan_counts(cnt.p, ia.p, nrows, s);
    long long sum = 0;
    d2h(&sum, ia.p + nrows, sizeof(long long), s);
    MI_HIP(hipStreamSynchronize(s));
    // a 32-bit row count that wrapped shows in the sum
    if (sum != E) require_int32_block(0, MAX_BLOCK_ENTRIES, "IJMatrixAssemble (one row)");
    cnt.release();
    DVec<ull> pos((size_t)nrows);
    MI_HIP(hipMemcpyAsync(pos.p, ia.p, (size_t)nrows * sizeof(long long), hipMemcpyDeviceToDevice, s));
    sub.alloc((size_t)E);
    scatter_rows_k<<<grid_for(E), BLK, 0, s>>>(E, R.p, ilower, pos.p, sub.p);
    DVec<gidx> oj((size_t)E);
    DVec<double> ov((size_t)E);
    gather_entries_k<<<grid_for(E), BLK, 0, s>>>(E, sub.p, cj.p, cv.p, oj.p, ov.p);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(s));
    R.release();
    cj = std::move(oj);
    cv = std::move(ov);
  }

  // step 2
  DVec<int> rowlen((size_t)nrows);
  if (nrows) {
    DVec<unsigned char> cls((size_t)nrows);
    classify_k<<<grid_for(nrows), BLK, 0, s>>>(nrows, ia.p, cj.p, cls.p, rowlen.p, st.p);
    MI_HIP(hipGetLastError());
    read_status(st, h, s);
    require_int32_block(0, (int64_t)h[ST_MAXLEN], "IJMatrixAssemble (one row)");
    const long long n1 = (long long)h[ST_NWAVE], n2 = (long long)h[ST_NBLOCK], n3 = (long long)h[ST_NLONG];
    if (n1 + n2 + n3 > 0) {
      DVec<int> l1((size_t)n1), l2((size_t)n2), l3((size_t)n3);
      DVec<unsigned> cur(4);
      MI_HIP(hipMemsetAsync(cur.p, 0, 4 * sizeof(unsigned), s));
      list_rows_k<<<grid_for(nrows), BLK, 0, s>>>(nrows, cls.p, l1.p, l2.p, l3.p, cur.p);
      DVec<long long> boff;
      DVec<unsigned char> badd;
      int nb = 0;
      if (mixed) {
        nb = (int)badd_h.size();
        boff.alloc(boff_h.size());
        badd.alloc(badd_h.size());
        MI_HIP(hipMemcpyAsync(boff.p, boff_h.data(), boff_h.size() * sizeof(long long), hipMemcpyHostToDevice, s));
        MI_HIP(hipMemcpyAsync(badd.p, badd_h.data(), badd_h.size(), hipMemcpyHostToDevice, s));
        MI_HIP(hipStreamSynchronize(s));  // the host vectors may be pageable
      }
      // a launch takes at most 2^31 - 1 workgroups in x: far more than the rows of a rank (32-bit local row ids)
      if (n1)
        sort_fold_lds_k<64, SORT_WAVE_CAP><<<(unsigned)n1, 64, 0, s>>>((int)n1, l1.p, ia.p, cj.p, cv.p, sub.p, nb, boff.p, badd.p,
                                                                     uniform_add, rowlen.p);
      if (n2)
        sort_fold_lds_k<BLK, SORT_LDS_CAP><<<(unsigned)n2, BLK, 0, s>>>((int)n2, l2.p, ia.p, cj.p, cv.p, sub.p, nb, boff.p, badd.p,
                                                                       uniform_add, rowlen.p);
      MI_HIP(hipGetLastError());
      if (n3) {
        // scratch of the long rows: their lengths (still the unsorted ones in rowlen) gathered and scanned on the device
        DVec<int> tlen((size_t)n3);
        DVec<long long> toff((size_t)n3 + 1);
        gather_lengths_k<<<grid_for(n3), BLK, 0, s>>>((int)n3, l3.p, rowlen.p, tlen.p);
        sk::exclusive_scan_counts(tlen.p, toff.p, n3, s);
        long long tt_ll = 0;
        d2h(&tt_ll, toff.p + n3, sizeof(long long), s);
        MI_HIP(hipStreamSynchronize(s));
        const size_t tt = (size_t)tt_ll;
        DVec<gidx> tcol(tt);
        DVec<double> tval(tt);
        DVec<unsigned char> tadd(tt);
        DVec<long long> tpos(tt);
        sort_fold_long_k<<<(unsigned)n3, BLK, 0, s>>>((int)n3, l3.p, toff.p, ia.p, cj.p, cv.p, sub.p, nb, boff.p, badd.p,
                                                      uniform_add, tcol.p, tval.p, tadd.p, tpos.p, rowlen.p);
        MI_HIP(hipGetLastError());
        MI_HIP(hipStreamSynchronize(s));
      }
      MI_HIP(hipStreamSynchronize(s));
    }
  }
  sub.release();

  // step 3
  diag.release();
  diag.nrows = nrows;
  diag.ncols = ncols_loc;
  diag.ia.alloc((size_t)nrows + 1);
  DVec<long long> oia((size_t)nrows + 1);
  long long dnnz = 0, onnz = 0;
  {
    DVec<int> nd((size_t)nrows), no((size_t)nrows);
    if (nrows) count_split_k<<<grid_for(nrows), BLK, 0, s>>>(nrows, ia.p, rowlen.p, cj.p, jlower, jupper, nd.p, no.p);
    MI_HIP(hipGetLastError());
    sk::exclusive_scan_counts(nd.p, diag.ia.p, nrows, s);
    sk::exclusive_scan_counts(no.p, oia.p, nrows, s);
    d2h(&dnnz, diag.ia.p + nrows, sizeof(long long), s);
    d2h(&onnz, oia.p + nrows, sizeof(long long), s);
    MI_HIP(hipStreamSynchronize(s));
  }
  require_int32_block(nrows, onnz, "IJMatrixAssemble (off-diagonal block)");  // the diagonal block: 64-bit offsets
  diag.nnz = dnnz;
  diag.ja.alloc((size_t)dnnz);
  diag.a.alloc((size_t)dnnz);
  DVec<gidx> ogid_d((size_t)onnz);
  DVec<double> oa_d((size_t)onnz);
  if (nrows)
    write_split_k<<<grid_for(nrows), BLK, 0, s>>>(nrows, ia.p, rowlen.p, cj.p, cv.p, jlower, jupper, diag.ia.p, oia.p, diag.ja.p,
                                                  diag.a.p, ogid_d.p, oa_d.p);
  MI_HIP(hipGetLastError());
  MI_HIP(hipStreamSynchronize(s));
  cj.release();
  cv.release();
  ia.release();
  rowlen.release();
  counters().t_kernels = wall_time() - t_begin;

  // the halo block is small: its global column ids go to the host, where the column map, the compressed ids and
  // (build_halo_plan) the exchange plan are made as for a host assembly
  const double t_halo = wall_time();
  HostCSR &D = out.diag, &O = out.offd;
  D = HostCSR();
  D.nrows = O.nrows = nrows;
  D.ncols = ncols_loc;
  O.ia.resize((size_t)nrows + 1);
  d2h(O.ia.data(), oia.p, ((size_t)nrows + 1) * sizeof(long long), s);
  O.ja.resize((size_t)onnz);
  O.a.resize((size_t)onnz);
  std::vector<gidx> ogid((size_t)onnz);
  if (onnz) {
    d2h(ogid.data(), ogid_d.p, (size_t)onnz * sizeof(gidx), s);
    d2h(O.a.data(), oa_d.p, (size_t)onnz * sizeof(double), s);
  }
  MI_HIP(hipStreamSynchronize(s));
  counters().host_mirror_bytes += (long long)(((size_t)nrows + 1) * sizeof(long long) + (size_t)onnz * (sizeof(gidx) + sizeof(double)));
  assemble_halo_columns_and_partition(comm, ilower, iupper, ogid, out);
  counters().t_mirror = wall_time() - t_halo;
  counters().device_assemblies++;
}

void finish_device(ParCSR &par, sk::DCsr &diag) {
  hipStream_t s = ctx().stream;
  const double t0 = wall_time();
  diag.download(par.diag, s);
  counters().host_mirror_bytes += (long long)(((size_t)diag.nrows + 1) * sizeof(long long) + (size_t)diag.nnz * (sizeof(int) + sizeof(double)));
  const double t1 = wall_time();
  counters().t_mirror += t1 - t0;
  if (diag.nnz >= device_format_min_nnz()) {
    sk::to_solve_format(diag, par.d_diag, s);
    par.to_device_halo();
  } else {
    diag.release();
    par.to_device();
  }
  counters().t_format = wall_time() - t1;
}

void vec_local_ids(const gidx *indices, int n, gidx jlower, gidx jupper, int *loc) {
  hipStream_t s = ctx().stream;
  MI_HIP(hipStreamSynchronize(nullptr));  // the caller's array is final before the library stream reads it
  DVec<ull> st(1);
  ull h = ~0ull;
  MI_HIP(hipMemcpyAsync(st.p, &h, sizeof(ull), hipMemcpyHostToDevice, s));
  MI_HIP(hipStreamSynchronize(s));
  local_ids_k<<<grid_for(n), BLK, 0, s>>>(n, indices, jlower, jupper, loc, st.p);
  MI_HIP(hipGetLastError());
  d2h(&h, st.p, sizeof(ull), s);
  MI_HIP(hipStreamSynchronize(s));
  if (h != ~0ull) {
    gidx bad = 0;
    d2h(&bad, indices + h, sizeof(gidx), s);
    MI_HIP(hipStreamSynchronize(s));
    fail(4, "IJVector: index " + std::to_string(bad) + " outside the local range");
  }
}

void laplace3d_device(int nx, int ny, int nz, int stencil, gidx ilower, gidx iupper, int64_t *nnz_out, gidx **rows_out,
                      gidx **cols_out, double **vals_out, double **rhs_out) {
  ensure_init();
  hipStream_t s = ctx().stream;
  const long long nloc = iupper - ilower + 1;
  DVec<int> cnt((size_t)nloc);
  DVec<long long> off((size_t)nloc + 1);
  if (nloc) lap_count_k<<<grid_for(nloc), BLK, 0, s>>>(nloc, ilower, nx, ny, nz, stencil, cnt.p);
  MI_HIP(hipGetLastError());
  sk::exclusive_scan_counts(cnt.p, off.p, nloc, s);
  long long nnz = 0;
  d2h(&nnz, off.p + nloc, sizeof(long long), s);
  MI_HIP(hipStreamSynchronize(s));
  // plain device allocations: the caller owns them and hands them back as ordinary device pointers
  void *rows = nullptr, *cols = nullptr, *vals = nullptr, *rhs = nullptr;
  auto release = [&]() { (void)hipFree(rows), (void)hipFree(cols), (void)hipFree(vals), (void)hipFree(rhs); };
  const size_t ne = (size_t)std::max<long long>(nnz, 1), nr = (size_t)std::max<long long>(nloc, 1);
  if (hipMalloc(&rows, ne * sizeof(gidx)) != hipSuccess || hipMalloc(&cols, ne * sizeof(gidx)) != hipSuccess ||
      hipMalloc(&vals, ne * sizeof(double)) != hipSuccess || hipMalloc(&rhs, nr * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    release();
    fail(2, "Laplace3DDevice: out of device memory");
  }
  if (nloc)
    lap_fill_k<<<grid_for(nloc), BLK, 0, s>>>(nloc, ilower, nx, ny, nz, stencil, off.p, (gidx *)rows, (gidx *)cols, (double *)vals,
                                              (double *)rhs);
  MI_HIP(hipGetLastError());
  MI_HIP(hipStreamSynchronize(s));
  *nnz_out = nnz;
  *rows_out = (gidx *)rows;
  *cols_out = (gidx *)cols;
  *vals_out = (double *)vals;
  *rhs_out = (double *)rhs;
}

}  // namespace ij
}  // namespace mi
