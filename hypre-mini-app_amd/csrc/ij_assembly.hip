// IJ assembly on the device.  See ij_assembly.hpp and DESIGN.md section 4.
//
// Determinism: the only atomics are integer ones (row counts, bucket cursors, list cursors, status words).  The one
// place where they decide an order -- the position of an entry inside its row's bucket of the counting sort -- is
// undone by the per-row sort on (column, submission index), a total order.  Every value is folded by ONE thread in
// submission order with a plain +, as assemble_parcsr does.
#include "ij_assembly.hpp"
#include "kernels.hpp"

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
// UPD (an update round): nothing is folded -- the row goes back sorted, with the tags (submission index * 2 + Add
// bit, which order like the submission indices) in `tag` moved along; they are read in place of `sub`.
template <int T, int CAP, bool UPD>
__global__ __launch_bounds__(T) void sort_fold_lds_k(int nlist, const int *__restrict__ list, const long long *__restrict__ ia,
                                                     gidx *__restrict__ cj, double *__restrict__ cv,
                                                     const long long *__restrict__ sub, int nb,
                                                     const long long *__restrict__ boff, const unsigned char *__restrict__ badd,
                                                     bool uniform, int *__restrict__ rowlen, long long *__restrict__ tag) {
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
    usub[e] = UPD ? tag[s + e] : sub ? sub[s + e] : s + e;
    uval[e] = cv[s + e];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < len; e += T) {
    const gidx c = ucol[e];
    const long long q = usub[e];
    int rank = 0;
    for (int j = 0; j < len; j++) rank += (ucol[j] < c || (ucol[j] == c && usub[j] < q)) ? 1 : 0;
    if (UPD) {  // every lane has its entry in LDS: the row may be overwritten
      cj[s + rank] = c;
      cv[s + rank] = uval[e];
      tag[s + rank] = q;
    } else {
      scol[rank] = c;
      sval[rank] = uval[e];
      sadd[rank] = add_of(q, nb, boff, badd, uniform) ? 1 : 0;
    }
  }
  if (UPD) return;
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
template <bool UPD>
__global__ __launch_bounds__(BLK) void sort_fold_long_k(int nlist, const int *__restrict__ list, const long long *__restrict__ toff,
                                                        const long long *__restrict__ ia, gidx *__restrict__ cj,
                                                        double *__restrict__ cv, const long long *__restrict__ sub, int nb,
                                                        const long long *__restrict__ boff, const unsigned char *__restrict__ badd,
                                                        bool uniform, gidx *__restrict__ tcol, double *__restrict__ tval,
                                                        unsigned char *__restrict__ tadd, long long *__restrict__ tpos,
                                                        int *__restrict__ rowlen, long long *__restrict__ tag) {
  if ((int)blockIdx.x >= nlist) return;
  const int row = list[blockIdx.x];
  const long long s = ia[row], len = ia[row + 1] - s, t0 = toff[blockIdx.x];
  for (long long e = threadIdx.x; e < len; e += BLK) {
    const gidx c = cj[s + e];
    const long long q = UPD ? tag[s + e] : sub ? sub[s + e] : s + e;
    long long rank = 0;
    for (long long j = 0; j < len; j++) {
      const gidx cc = cj[s + j];
      const long long qq = UPD ? tag[s + j] : sub ? sub[s + j] : s + j;
      rank += (cc < c || (cc == c && qq < q)) ? 1 : 0;
    }
    tcol[t0 + rank] = c;
    tval[t0 + rank] = cv[s + e];
    if (UPD)
      tpos[t0 + rank] = q;
    else
      tadd[t0 + rank] = add_of(q, nb, boff, badd, uniform) ? 1 : 0;
  }
  __syncthreads();
  if (UPD) {  // the sorted row goes back as it is, tags (held in tpos) moved along
    for (long long e = threadIdx.x; e < len; e += BLK) {
      cj[s + e] = tcol[t0 + e];
      cv[s + e] = tval[t0 + e];
      tag[s + e] = tpos[t0 + e];
    }
    return;
  }
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

// ---------------------------------------------------------------- update round of an assembled matrix
__global__ __launch_bounds__(BLK) void tag_entries_k(long long E, const long long *__restrict__ sub, int nb,
                                                     const long long *__restrict__ boff, const unsigned char *__restrict__ badd,
                                                     bool uniform, long long *__restrict__ tag) {
  IJ_GRID_STRIDE(p, E) {
    const long long q = sub ? sub[p] : p;
    tag[p] = (q << 1) | (add_of(q, nb, boff, badd, uniform) ? 1 : 0);
  }
}
__global__ __launch_bounds__(BLK) void local_rows_k(long long E, const gidx *__restrict__ R, const long long *__restrict__ sub,
                                                    gidx ilower, int *__restrict__ prow) {
  IJ_GRID_STRIDE(p, E) prow[p] = (int)(R[sub ? sub[p] : p] - ilower);
}

template <class T>
__device__ __forceinline__ long long find_sorted(const T *__restrict__ a, long long lo, long long hi, T key) {
  const long long end = hi;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (a[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return (lo < end && a[lo] == key) ? lo : -1;
}

// The stored operator as the locate kernel sees it.  Diag block: solve format, row pointers 32-bit (dia) or, for a
// block of 2^31 entries or more, 64-bit (dia64).  Halo block: only the rows that own halo entries are stored (orows:
// their local ids, ascending); its columns are positions in the column map.
struct StoredPattern {
  const int *dia;
  const long long *dia64;
  const int *dja;
  const int *orows, *oia, *oja;
  const gidx *colmap;
  int nrows_c, next;
  gidx jlower, jupper;
};

// One lane per sorted entry; the first entry of a run of equal (row, column) finds the pair in the stored diag row or
// the stored halo row.  A pair that is not stored leaves the smallest submission index of its run in st[ST_BAD] (the
// head of a run is its first entry in submission order).  Nothing of the matrix is written.
__global__ __launch_bounds__(BLK) void locate_k(long long E, const long long *__restrict__ ia, const int *__restrict__ prow,
                                                const gidx *__restrict__ cj, const long long *__restrict__ tag,
                                                StoredPattern P, long long *__restrict__ loc, ull *__restrict__ st) {
  IJ_GRID_STRIDE(p, E) {
    const int i = prow[p];
    const gidx c = cj[p];
    if (p > ia[i] && cj[p - 1] == c) continue;
    long long at = -1;
    bool halo = false;
    if (c >= P.jlower && c <= P.jupper) {
      const long long lo = P.dia64 ? P.dia64[i] : (long long)P.dia[i], hi = P.dia64 ? P.dia64[i + 1] : (long long)P.dia[i + 1];
      at = find_sorted<int>(P.dja, lo, hi, (int)(c - P.jlower));
    } else {
      halo = true;
      const long long cid = find_sorted<gidx>(P.colmap, 0, P.next, c);
      const long long cr = cid < 0 ? -1 : find_sorted<int>(P.orows, 0, P.nrows_c, i);
      if (cr >= 0) at = find_sorted<int>(P.oja, P.oia[cr], P.oia[cr + 1], (int)cid);
    }
    if (at < 0) atomicMin(&st[ST_BAD], (ull)(tag[p] >> 1));
    loc[p] = halo ? ~at : at;
  }
}
// the refused entry, for the message: its global row and column
__global__ __launch_bounds__(BLK) void find_entry_k(long long E, const int *__restrict__ prow, const gidx *__restrict__ cj,
                                                    const long long *__restrict__ tag, long long q, gidx ilower,
                                                    gidx *__restrict__ out) {
  IJ_GRID_STRIDE(p, E)
    if ((tag[p] >> 1) == q) {
      out[0] = ilower + prow[p];
      out[1] = cj[p];
    }
}
// One lane per run: from the stored value, the run's entries in submission order -- Set replaces, Add is one plain +;
// a SetConstantValues call (cbefore[k] entries were submitted before it) takes effect between them.  The result
// goes to the head's slot of cv; the matrix is written by store_runs_k, after the constant fill.
__global__ __launch_bounds__(BLK) void walk_runs_k(long long E, const long long *__restrict__ ia, const int *__restrict__ prow,
                                                   const gidx *__restrict__ cj, double *__restrict__ cv,
                                                   const long long *__restrict__ tag, const long long *__restrict__ loc,
                                                   const double *__restrict__ da, const double *__restrict__ oa, int nc,
                                                   const long long *__restrict__ cbefore, const double *__restrict__ cval) {
  IJ_GRID_STRIDE(p, E) {
    const int i = prow[p];
    const gidx c = cj[p];
    if (p > ia[i] && cj[p - 1] == c) continue;
    const long long at = loc[p], end = ia[i + 1];
    double v = at >= 0 ? da[at] : oa[~at];
    int kc = 0;
    for (long long j = p; j < end && cj[j] == c; j++) {
      const long long t = tag[j];
      for (; kc < nc && cbefore[kc] <= (t >> 1); kc++) v = cval[kc];
      v = (t & 1) ? v + cv[j] : cv[j];
    }
    if (kc < nc) v = cval[nc - 1];
    cv[p] = v;
  }
}
__global__ __launch_bounds__(BLK) void store_runs_k(long long E, const long long *__restrict__ ia, const int *__restrict__ prow,
                                                    const gidx *__restrict__ cj, const double *__restrict__ cv,
                                                    const long long *__restrict__ loc, double *__restrict__ da,
                                                    double *__restrict__ oa) {
  IJ_GRID_STRIDE(p, E) {
    const int i = prow[p];
    if (p > ia[i] && cj[p - 1] == cj[p]) continue;
    const long long at = loc[p];
    if (at >= 0)
      da[at] = cv[p];
    else
      oa[~at] = cv[p];
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

namespace {
// The front of an assembly and of an update round: the staged batches checked, concatenated, bucketed by row and
// every row sorted by (column, submission index).
struct Staged {
  int64_t E = 0;
  int nrows = 0;
  DVec<gidx> R, cj;
  DVec<double> cv;
  DVec<long long> ia;
  DVec<long long> sub;  // submission index of every entry (counting sort only; empty: the position itself)
  DVec<int> rowlen;
  bool uniform_add = false, mixed = false;
  std::vector<long long> boff_h;
  std::vector<unsigned char> badd_h;
  DVec<long long> boff;
  DVec<unsigned char> badd;
  int nb = 0;
};

// Set / Add per batch (only when the batches differ), on the host and on the device
void batch_kinds(const std::vector<DevBatch> &batches, Staged &g, hipStream_t s) {
  g.uniform_add = batches.empty() ? false : batches.front().add;
  for (auto &b : batches) g.mixed = g.mixed || (b.add != g.uniform_add);
  if (!g.mixed) return;
  long long o = 0;
  for (auto &b : batches) {
    if (!b.n) continue;
    g.boff_h.push_back(o);
    g.badd_h.push_back(b.add ? 1 : 0);
    o += b.n;
  }
  g.boff_h.push_back(o);
  g.nb = (int)g.badd_h.size();
  g.boff.alloc(g.boff_h.size());
  g.badd.alloc(g.badd_h.size());
  MI_HIP(hipMemcpyAsync(g.boff.p, g.boff_h.data(), g.boff_h.size() * sizeof(long long), hipMemcpyHostToDevice, s));
  MI_HIP(hipMemcpyAsync(g.badd.p, g.badd_h.data(), g.badd_h.size(), hipMemcpyHostToDevice, s));
  MI_HIP(hipStreamSynchronize(s));  // the host vectors may be pageable
}

// The first pass only reads the batches.  Per batch: ownership and order inside it; across batches: the first row of
// one against the last of the one before.  false: a row is not owned (*bad_row: the first one of its batch).
bool check_rows(const std::vector<DevBatch> &batches, gidx ilower, gidx iupper, bool *in_row_order, gidx *bad_row,
                hipStream_t s) {
  ull h[ST_WORDS];
  DVec<ull> stb(ST_WORDS);
  const gidx *prev_last = nullptr;
  bool unordered = false;
  int64_t E = 0;
  for (auto &b : batches) {
    if (!b.n) continue;
    E += b.n;
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
      d2h(bad_row, b.rows.p + h[ST_BAD], sizeof(gidx), s);
      MI_HIP(hipStreamSynchronize(s));
      return false;
    }
    unordered = unordered || h[ST_UNORDERED] != 0;
  }
  *in_row_order = E > 0 && !unordered;
  return true;
}

// The entries in submission order (one batch as it is, several concatenated, each released once copied), then the
// row pointers: found at the row boundaries when the entries arrive in row order, by a counting sort otherwise.
// prow (update rounds): the local row of every bucketed entry.
void bucket_rows(std::vector<DevBatch> &batches, bool in_row_order, gidx ilower, int nrows, Staged &g, DVec<int> *prow,
                 hipStream_t s) {
  const int64_t E = g.E;
  DVec<gidx> &R = g.R, &cj = g.cj;
  DVec<double> &cv = g.cv;
  DVec<long long> &ia = g.ia, &sub = g.sub;
  g.nrows = nrows;
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

  ia.alloc((size_t)nrows + 1);
  if (E == 0) {
    MI_HIP(hipMemsetAsync(ia.p, 0, ((size_t)nrows + 1) * sizeof(long long), s));
  } else if (in_row_order) {
    boundaries_k<<<grid_for(E), BLK, 0, s>>>(E, R.p, ilower, nrows, ia.p);
    MI_HIP(hipGetLastError());
    if (prow) local_rows_k<<<grid_for(E), BLK, 0, s>>>(E, R.p, nullptr, ilower, prow->p);
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
    if (prow) local_rows_k<<<grid_for(E), BLK, 0, s>>>(E, R.p, sub.p, ilower, prow->p);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(s));
    R.release();
    cj = std::move(oj);
    cv = std::move(ov);
  }
}

// step 2: every row whose columns are not strictly ascending is sorted by (column, submission index); an assembly
// (tag null) folds the runs of equal columns and leaves the folded lengths in rowlen, an update round keeps every
// entry and moves its tag along
void sort_rows(Staged &g, long long *tag, DVec<ull> &st, hipStream_t s) {
  const int nrows = g.nrows;
  DVec<long long> &ia = g.ia, &sub = g.sub, &boff = g.boff;
  DVec<gidx> &cj = g.cj;
  DVec<double> &cv = g.cv;
  DVec<int> &rowlen = g.rowlen;
  DVec<unsigned char> &badd = g.badd;
  const int nb = g.nb;
  const bool uniform_add = g.uniform_add;
  ull h[ST_WORDS];
  rowlen.alloc((size_t)nrows);
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
      // a launch takes at most 2^31 - 1 workgroups in x: far more than the rows of a rank (32-bit local row ids)
      if (n1 && tag)
        sort_fold_lds_k<64, SORT_WAVE_CAP, true><<<(unsigned)n1, 64, 0, s>>>((int)n1, l1.p, ia.p, cj.p, cv.p, sub.p, nb, boff.p,
                                                                           badd.p, uniform_add, rowlen.p, tag);
      else if (n1)
        sort_fold_lds_k<64, SORT_WAVE_CAP, false><<<(unsigned)n1, 64, 0, s>>>((int)n1, l1.p, ia.p, cj.p, cv.p, sub.p, nb, boff.p,
                                                                            badd.p, uniform_add, rowlen.p, nullptr);
      if (n2 && tag)
        sort_fold_lds_k<BLK, SORT_LDS_CAP, true><<<(unsigned)n2, BLK, 0, s>>>((int)n2, l2.p, ia.p, cj.p, cv.p, sub.p, nb, boff.p,
                                                                             badd.p, uniform_add, rowlen.p, tag);
      else if (n2)
        sort_fold_lds_k<BLK, SORT_LDS_CAP, false><<<(unsigned)n2, BLK, 0, s>>>((int)n2, l2.p, ia.p, cj.p, cv.p, sub.p, nb, boff.p,
                                                                              badd.p, uniform_add, rowlen.p, nullptr);
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
        DVec<unsigned char> tadd(tag ? (size_t)0 : tt);
        DVec<long long> tpos(tt);
        if (tag)
          sort_fold_long_k<true><<<(unsigned)n3, BLK, 0, s>>>((int)n3, l3.p, toff.p, ia.p, cj.p, cv.p, sub.p, nb, boff.p, badd.p,
                                                            uniform_add, tcol.p, tval.p, tadd.p, tpos.p, rowlen.p, tag);
        else
          sort_fold_long_k<false><<<(unsigned)n3, BLK, 0, s>>>((int)n3, l3.p, toff.p, ia.p, cj.p, cv.p, sub.p, nb, boff.p, badd.p,
                                                             uniform_add, tcol.p, tval.p, tadd.p, tpos.p, rowlen.p, nullptr);
        MI_HIP(hipGetLastError());
        MI_HIP(hipStreamSynchronize(s));
      }
      MI_HIP(hipStreamSynchronize(s));
    }
  }
}

void new_status(DVec<ull> &st, hipStream_t s) {
  st.alloc(ST_WORDS);
  ull init[ST_WORDS] = {~0ull, 0, 0, 0, 0, 0, 0, 0};
  MI_HIP(hipMemcpyAsync(st.p, init, sizeof(init), hipMemcpyHostToDevice, s));
  MI_HIP(hipStreamSynchronize(s));
}

}  // namespace

void assemble_parcsr_device(Comm &comm, gidx ilower, gidx iupper, gidx jlower, gidx jupper, std::vector<DevBatch> &batches,
                            ParCSR &out, sk::DCsr &diag) {
  ensure_init();
  hipStream_t s = ctx().stream;
  const double t_begin = wall_time();
  require_int32_block(iupper - ilower + 1, 0, "IJMatrixAssemble");
  const int nrows = (int)(iupper - ilower + 1);
  const int ncols_loc = (int)(jupper - jlower + 1);
  Staged g;
  for (auto &b : batches) g.E += b.n;
  // a refusal leaves the batches as they were
  bool in_row_order = false;
  gidx bad = 0;
  if (!check_rows(batches, ilower, iupper, &in_row_order, &bad, s))
    fail(4, "IJMatrix: row " + std::to_string(bad) + " is not owned by this rank");
  batch_kinds(batches, g, s);
  DVec<ull> st;
  new_status(st, s);
  bucket_rows(batches, in_row_order, ilower, nrows, g, nullptr, s);
  sort_rows(g, nullptr, st, s);
  DVec<long long> &ia = g.ia, &sub = g.sub;
  DVec<gidx> &cj = g.cj;
  DVec<double> &cv = g.cv;
  DVec<int> &rowlen = g.rowlen;
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

bool update_locate(gidx ilower, gidx iupper, gidx jlower, gidx jupper, std::vector<DevBatch> &batches, const ParCSR &par,
                   UpdatePlan &plan) {
  ensure_init();
  hipStream_t s = ctx().stream;
  const double t_begin = wall_time();
  MI_REQUIRE(par.on_device, "IJMatrix update: the matrix has no device mirror");
  MI_REQUIRE(par.d_diag.a.p || par.d_diag.nnz == 0, "IJMatrix update: the device diag block holds no fp64 values");
  const int nrows = (int)(iupper - ilower + 1);
  Staged g;
  plan.batch_sizes.clear();
  for (auto &b : batches) {
    g.E += b.n;
    plan.batch_sizes.push_back(b.n);
  }
  bool in_row_order = false;
  gidx bad_row = 0;
  if (!check_rows(batches, ilower, iupper, &in_row_order, &bad_row, s)) return false;
  batch_kinds(batches, g, s);
  DVec<ull> st;
  new_status(st, s);
  const int64_t E = g.E;
  plan.E = E;
  plan.nrows = nrows;
  plan.prow.alloc((size_t)E);
  bucket_rows(batches, in_row_order, ilower, nrows, g, &plan.prow, s);
  plan.tag.alloc((size_t)E);
  if (E) tag_entries_k<<<grid_for(E), BLK, 0, s>>>(E, g.sub.p, g.nb, g.boff.p, g.badd.p, g.uniform_add, plan.tag.p);
  MI_HIP(hipGetLastError());
  sort_rows(g, plan.tag.p, st, s);
  g.sub.release();
  g.rowlen.release();
  plan.ia = std::move(g.ia);
  plan.cj = std::move(g.cj);
  plan.cv = std::move(g.cv);
  plan.loc.alloc((size_t)E);
  if (E) {
    // DevOffd stores only the rows that own halo entries, and its columns are positions in the column map: the
    // map gets a device copy for the round
    DVec<gidx> colmap;
    colmap.upload(par.col_map_offd);
    StoredPattern P;
    P.dia = par.d_diag.ia.p;
    P.dia64 = par.d_diag.ia64.p;
    P.dja = par.d_diag.ja.p;
    P.orows = par.d_offd.rows.p;
    P.oia = par.d_offd.ia.p;
    P.oja = par.d_offd.ja.p;
    P.colmap = colmap.p;
    P.nrows_c = par.d_offd.nrows_c;
    P.next = (int)par.col_map_offd.size();
    P.jlower = jlower;
    P.jupper = jupper;
    locate_k<<<grid_for(E), BLK, 0, s>>>(E, plan.ia.p, plan.prow.p, plan.cj.p, plan.tag.p, P, plan.loc.p, st.p);
    MI_HIP(hipGetLastError());
    // the whole round is located and the flag read before any value is written: a refused round changes nothing
    ull h[ST_WORDS];
    read_status(st, h, s);
    if (h[ST_BAD] != ~0ull) {
      DVec<gidx> who(2);
      find_entry_k<<<grid_for(E), BLK, 0, s>>>(E, plan.prow.p, plan.cj.p, plan.tag.p, (long long)h[ST_BAD], ilower, who.p);
      MI_HIP(hipGetLastError());
      gidx rc[2] = {0, 0};
      d2h(rc, who.p, sizeof(rc), s);
      MI_HIP(hipStreamSynchronize(s));
      fail(1, "IJMatrix: entry (row " + std::to_string(rc[0]) + ", column " + std::to_string(rc[1]) +
                  ") is not in the pattern of the assembled matrix; the pattern is frozen by the first Assemble and "
                  "the update round was discarded");
    }
  }
  counters().t_update_kernels = wall_time() - t_begin;
  return true;
}

void update_apply(UpdatePlan &plan, const std::vector<UpdateConst> &consts, ParCSR &par) {
  hipStream_t s = ctx().stream;
  const double t_begin = wall_time();
  const int64_t E = plan.E;
  const int nc = (int)consts.size();
  DevCSR &D = par.d_diag;
  DevOffd &O = par.d_offd;
  DVec<long long> cbefore;
  DVec<double> cval;
  if (nc) {
    std::vector<long long> cb;
    std::vector<double> cvl;
    for (auto &c : consts) {
      cb.push_back(c.before);
      cvl.push_back(c.value);
    }
    cbefore.upload(cb);
    cval.upload(cvl);
  }
  // every run's final value from the stored one, into the round's own arrays; then the constant (the last one is what
  // entries that no run mentions end with); then the runs' values into d_diag.a / d_offd.a, in place
  if (E)
    walk_runs_k<<<grid_for(E), BLK, 0, s>>>(E, plan.ia.p, plan.prow.p, plan.cj.p, plan.cv.p, plan.tag.p, plan.loc.p, D.a.p, O.a.p,
                                            nc, cbefore.p, cval.p);
  if (nc && D.nnz) fill_k<<<grid_for(D.nnz), BLK, 0, s>>>(D.a.p, (long long)D.nnz, consts.back().value);
  if (nc && O.nnz) fill_k<<<grid_for(O.nnz), BLK, 0, s>>>(O.a.p, (long long)O.nnz, consts.back().value);
  if (E) store_runs_k<<<grid_for(E), BLK, 0, s>>>(E, plan.ia.p, plan.prow.p, plan.cj.p, plan.cv.p, plan.loc.p, D.a.p, O.a.p);
  MI_HIP(hipGetLastError());
  MI_HIP(hipStreamSynchronize(s));
  plan = UpdatePlan();
  const double t_kernels = wall_time();
  counters().t_update_kernels += t_kernels - t_begin;
  // what depends on the values and nothing else.  The tile schedule (rb), the tile descriptors (tdesc), the x-cache
  // column lists (ucols, lcol) and the halo plan depend on the pattern alone: they are not touched.
  k::build_value_dictionary(D, s);
  const double t_dict = wall_time();
  counters().t_update_dict = t_dict - t_kernels;
  // the host mirrors (ILU, FSAI, the locality numbering and the dumps read them): the value arrays only
  if (D.nnz) d2h(par.diag.a.data(), D.a.p, (size_t)D.nnz * sizeof(double), s);
  if (O.nnz) d2h(par.offd.a.data(), O.a.p, (size_t)O.nnz * sizeof(double), s);
  MI_HIP(hipStreamSynchronize(s));
  counters().host_mirror_bytes += (long long)((size_t)(D.nnz + O.nnz) * sizeof(double));
  counters().t_update_mirror = wall_time() - t_dict;
  par.assembly_stamp = next_assembly_stamp();
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
