// IJ assembly on the device: COO batches that arrive in device memory are staged, sorted, folded
// and split into the diag / halo blocks by kernels; the result is the ParCSR that assemble_parcsr (parcsr.cpp, the
// specification) builds from the same entries, bit for bit.  Also the device side of IJVectorSetValues' index
// conversion and the synthetic generator into device memory.
#pragma once
#include "parcsr.hpp"
#include "setup_kernels.hpp"

namespace mi {
namespace ij {

// one SetValues / AddToValues call, expanded to one entry per (row, column, value), in library-owned device memory
struct DevBatch {
  DVec<gidx> rows, cols;
  DVec<double> vals;
  int64_t n = 0;
  bool add = false;
};

// rows with more entries than this are sorted by the any-length path (global memory) instead of in LDS
constexpr int SORT_LDS_CAP = 1024;
// rows up to this length get one wave, longer ones (up to SORT_LDS_CAP) a block of four
constexpr int SORT_WAVE_CAP = 256;

struct Counters {
  long long device_assemblies = 0;    // matrices assembled by assemble_parcsr_device
  long long entries_fetched = 0;      // entries of matrix batches / vector indices copied device -> host
  long long host_mirror_bytes = 0;    // bytes of the host mirrors (diag + halo block) downloaded by device assemblies
  double t_kernels = 0, t_mirror = 0, t_format = 0;  // seconds of the last device assembly, by phase
  long long value_updates = 0;         // update rounds applied to assembled matrices (host or device)
  long long device_value_updates = 0;  // those applied by kernels
  double t_update_kernels = 0, t_update_dict = 0, t_update_mirror = 0;  // seconds of the last device update round
};
Counters &counters();

// MI_HYPRE_DEVICE_ASSEMBLY (default 1)
bool device_assembly_enabled();

// copies of the caller's device arrays (complete on return: the caller may overwrite or free its arrays)
void stage_coo(const gidx *rows, const gidx *cols, const double *vals, int64_t n, bool add, DevBatch &out);
// the ncols / row_indexes form, expanded on the device (row_indexes may be null: rows packed one after the other)
void stage_ncols(int nrows, const int *ncols, const gidx *rows, const int *row_indexes, const gidx *cols,
                 const double *vals, bool add, DevBatch &out);
void fill_values(DevBatch &b, double v);

// assemble_parcsr on the device.  out gets everything but the host copy of the diag block and the device mirror;
// the diag block stays in `diag` (finish_device makes both).  Fails like assemble_parcsr; nothing is consumed then.
void assemble_parcsr_device(Comm &comm, gidx ilower, gidx iupper, gidx jlower, gidx jupper, std::vector<DevBatch> &batches,
                            ParCSR &out, sk::DCsr &diag);
// host mirror of the diag block (one download) and the solve format: sk::to_solve_format moves diag's arrays for
// blocks of at least MI_HYPRE_DEVICE_FORMAT_MIN_NNZ entries, smaller ones go through ParCSR::to_device
void finish_device(ParCSR &par, sk::DCsr &diag);

// ---- update round of an assembled matrix on the device: the result is update_parcsr_values' (parcsr.cpp), bit for bit.
// The round's entries bucketed by row and sorted by (column, submission index) like an assembly's, not folded; for
// the first entry of every run of equal (row, column) the position of that pair in the stored values.
struct UpdatePlan {
  int64_t E = 0;
  int nrows = 0;
  std::vector<long long> batch_sizes;  // entries of every staged batch, in call order
  DVec<long long> ia;    // row pointers into the sorted entries
  DVec<int> prow;        // local row of every sorted entry
  DVec<gidx> cj;         // global column
  DVec<double> cv;       // value
  DVec<long long> tag;   // submission index * 2 + (1: Add, 0: Set)
  DVec<long long> loc;   // run heads: p >= 0 position in d_diag.a, ~p < 0 position in d_offd.a
};
// SetConstantValues(value) called after `before` entries of the round had been submitted
struct UpdateConst {
  long long before = 0;
  double value = 0.0;
};
// Validation, bucketing, sort and the locate kernel; writes nothing to the matrix and consumes the batches.  Fails
// (HYPRE_ERROR_GENERIC, naming global row and column) at the first entry in submission order that is not in the
// pattern; returns false, before anything is consumed, when a row is outside [ilower, iupper].
bool update_locate(gidx ilower, gidx iupper, gidx jlower, gidx jupper, std::vector<DevBatch> &batches, const ParCSR &par,
                   UpdatePlan &plan);
// The apply kernels (every run walked by one thread in submission order from the stored value), then what depends on
// the values: d_diag.a / d_offd.a in place, the value dictionary, the host mirrors diag.a / offd.a, a new stamp.
void update_apply(UpdatePlan &plan, const std::vector<UpdateConst> &consts, ParCSR &par);

// loc[i] = indices[i] - jlower, range-checked on the device; fails naming the first index outside [jlower, jupper]
void vec_local_ids(const gidx *indices, int n, gidx jlower, gidx jupper, int *loc);

// HYPRE_MI_Laplace3D's arrays generated into device memory (hipMalloc; released with hipFree)
void laplace3d_device(int nx, int ny, int nz, int stencil, gidx ilower, gidx iupper, int64_t *nnz, gidx **rows, gidx **cols,
                      double **vals, double **rhs);

}  // namespace ij
}  // namespace mi
