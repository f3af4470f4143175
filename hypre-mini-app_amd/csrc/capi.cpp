// extern "C" boundary: the HYPRE-shaped C ABI declared in include/*.h.
// Plain pointers and sizes in, HYPRE_Int error codes out; C++ exceptions never
// cross it.  The driver ignores return codes (src/HypreSystem.cpp:723), so
// failures also print to stderr and accumulate in the HYPRE-style error flag.
#include <limits>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>

#include "HYPRE_mi_ext.h"
#include "_hypre_parcsr_ls.h"
#include "ij_assembly.hpp"
#include "kernels.hpp"
#include "profile.hpp"
#include "solvers.hpp"
#include "amg_setup_internal.hpp"
#include "capi_marshal.hpp"

using namespace mi;

namespace {

int g_error_flag = 0;
std::string g_last_error;

int record_error(int code, const std::string &msg) {
  g_error_flag |= code;
  g_last_error = msg;
  fprintf(stderr, "mi_hypre error (%d): %s\n", code, msg.c_str());
  fflush(stderr);
  return code;
}

#define API_BEGIN try {
#define API_END                                             \
  }                                                         \
  catch (const mi::Error &e) {                              \
    return record_error(e.code, e.what());                  \
  }                                                         \
  catch (const std::bad_alloc &) {                          \
    return record_error(HYPRE_ERROR_MEMORY, "out of host memory"); \
  }                                                         \
  catch (const std::exception &e) {                         \
    return record_error(HYPRE_ERROR_GENERIC, e.what());     \
  }                                                         \
  return 0;

struct IJMatrixObj {
  gidx ilower, iupper, jlower, jupper;
  std::vector<IJEntryBatch> batches;
  // batches whose arrays all arrived in device memory stay there (ij_assembly.hpp) until a host batch joins them:
  // then they are fetched and the matrix takes the host path.  At most one of the two lists is in use.
  std::vector<ij::DevBatch> dev_batches;
  bool device_path = true;  // no host batch so far
  bool device_failed = false;  // a device assembly failed: its batches may be gone, the matrix is not usable
  ParCSR par;
  bool assembled = false;
  // An update round of an assembled matrix (the pattern is frozen): the set / add calls are staged in `batches` or
  // `dev_batches` as before the first Assemble, SetConstantValues is recorded at its place among them, and the
  // next Assemble applies all of it in call order to the stored values.
  bool round_open = false;
  bool round_refused = false;  // a set call of this round was refused (N > 1 ranks: the collective Assemble reports it)
  std::vector<IJUpdateConst> consts;
  void drop_round() {
    batches.clear();
    dev_batches.clear();
    consts.clear();
    round_open = round_refused = false;
  }
};

struct IJVectorObj {
  gidx jlower, jupper;
  int ncomp = 1;
  ParVector par;
  bool initialized = false;
};

inline IJMatrixObj *M(HYPRE_IJMatrix m) { return reinterpret_cast<IJMatrixObj *>(m); }
inline IJVectorObj *V(HYPRE_IJVector v) { return reinterpret_cast<IJVectorObj *>(v); }
inline ParCSR *PM(HYPRE_ParCSRMatrix a) { return reinterpret_cast<ParCSR *>(a); }
inline ParVector *PV(HYPRE_ParVector v) { return reinterpret_cast<ParVector *>(v); }
inline SolverBase *S(HYPRE_Solver s) { return reinterpret_cast<SolverBase *>(s); }

template <class T>
T *as(HYPRE_Solver s, SolverBase::Kind k, const char *what) {
  SolverBase *b = S(s);
  if (!b) fail(HYPRE_ERROR_ARG, std::string(what) + ": NULL solver handle");
  if (b->kind != k) fail(HYPRE_ERROR_ARG, std::string(what) + ": handle is not of the expected solver type");
  return static_cast<T *>(b);
}
AmgSolver *AMG(HYPRE_Solver s) { return as<AmgSolver>(s, SolverBase::K_AMG, "BoomerAMG"); }
GmresSolver *GM(HYPRE_Solver s) { return as<GmresSolver>(s, SolverBase::K_GMRES, "GMRES"); }
BicgstabSolver *BI(HYPRE_Solver s) { return as<BicgstabSolver>(s, SolverBase::K_BICGSTAB, "BiCGSTAB"); }
PcgSolver *PC(HYPRE_Solver s) { return as<PcgSolver>(s, SolverBase::K_PCG, "PCG"); }
KrylovSolver *KR(HYPRE_Solver s) {
  SolverBase *b = S(s);
  if (!b || (b->kind != SolverBase::K_GMRES && b->kind != SolverBase::K_BICGSTAB && b->kind != SolverBase::K_PCG))
    fail(HYPRE_ERROR_ARG, "handle is not a Krylov solver");
  return static_cast<KrylovSolver *>(b);
}

// copy n elements from a host-or-device pointer into a host vector
// counted: entries of an IJ matrix batch or IJ vector indices (HYPRE_MI_GetCounter "ij_entries_fetched_to_host")
template <class T>
void fetch(const T *src, size_t n, std::vector<T> &dst, bool counted = false) {
  dst.resize(n);
  if (!n) return;
  if (is_device_pointer(src)) {
    d2h(dst.data(), src, n * sizeof(T), nullptr);
    if (counted) ij::counters().entries_fetched += (long long)n;
  } else {
    memcpy(dst.data(), src, n * sizeof(T));
  }
}

// a host batch joins device batches: they come to the host, in call order, and the matrix takes the host path
void ij_demote(IJMatrixObj *m) {
  for (auto &d : m->dev_batches) {
    IJEntryBatch b;
    b.add = d.add;
    fetch(d.rows.p, (size_t)d.n, b.rows);
    fetch(d.cols.p, (size_t)d.n, b.cols);
    fetch(d.vals.p, (size_t)d.n, b.vals, true);
    m->batches.push_back(std::move(b));
  }
  m->dev_batches.clear();
  m->device_path = false;
}

// the first call after an Assemble that touches the values opens an update round
void ij_open_round(IJMatrixObj *m) {
  if (m->round_open) return;
  if (m->device_failed) fail(HYPRE_ERROR_GENERIC, "IJMatrix: an earlier assembly of this matrix failed; create it again");
  m->round_open = true;
  m->round_refused = false;
  m->device_path = true;  // every round chooses its path anew
}

// a host batch of an update round is checked against the pattern by the call that brings it; a refusal discards
// the round (on N > 1 ranks it stays open, so that the collective Assemble fails on every rank)
void ij_check_round_batch(IJMatrixObj *m) {
  try {
    check_update_batch(m->par, m->jlower, m->jupper, m->batches.back());
  } catch (...) {
    const bool collective = current_comm().size > 1;
    m->drop_round();
    m->round_open = m->round_refused = collective;
    throw;
  }
}

void ij_stage(IJMatrixObj *m, int nrows, const int *ncols, const gidx *rows, const int *row_indexes, const gidx *cols,
              const double *vals, bool add) {
  if (m->assembled) ij_open_round(m);
  if (nrows <= 0 || m->round_refused) return;
  if (m->device_path && ij::device_assembly_enabled()) {
    const bool all_dev = is_device_pointer(rows) && is_device_pointer(cols) && is_device_pointer(vals) &&
                         (!ncols || is_device_pointer(ncols)) && (!row_indexes || is_device_pointer(row_indexes));
    if (all_dev) {
      ij::DevBatch d;
      if (!ncols)
        ij::stage_coo(rows, cols, vals, nrows, add, d);
      else
        ij::stage_ncols(nrows, ncols, rows, row_indexes, cols, vals, add, d);
      m->dev_batches.push_back(std::move(d));
      return;
    }
    if (!m->dev_batches.empty()) ij_demote(m);
  }
  m->device_path = false;
  IJEntryBatch b;
  b.add = add;
  if (!ncols) {
    // one entry per "row" (src/HypreSystem.cpp:942: ncols == NULL, row_indexes == NULL)
    fetch(rows, (size_t)nrows, b.rows);
    fetch(cols, (size_t)nrows, b.cols);
    fetch(vals, (size_t)nrows, b.vals, true);
  } else {
    std::vector<int> nc, ri;
    std::vector<gidx> r;
    fetch(ncols, (size_t)nrows, nc);
    fetch(rows, (size_t)nrows, r);
    if (row_indexes) fetch(row_indexes, (size_t)nrows, ri);
    size_t total = 0, span = 0;
    for (int i = 0; i < nrows; i++) {
      total += (size_t)nc[(size_t)i];
      const size_t endi = (row_indexes ? (size_t)ri[(size_t)i] : total - (size_t)nc[(size_t)i]) + (size_t)nc[(size_t)i];
      span = std::max(span, endi);
    }
    std::vector<gidx> c;
    std::vector<double> v;
    fetch(cols, span, c);
    fetch(vals, span, v, true);
    b.rows.reserve(total);
    b.cols.reserve(total);
    b.vals.reserve(total);
    size_t run = 0;
    for (int i = 0; i < nrows; i++) {
      const size_t start = row_indexes ? (size_t)ri[(size_t)i] : run;
      for (int k = 0; k < nc[(size_t)i]; k++) {
        b.rows.push_back(r[(size_t)i]);
        b.cols.push_back(c[start + (size_t)k]);
        b.vals.push_back(v[start + (size_t)k]);
      }
      run += (size_t)nc[(size_t)i];
    }
  }
  m->batches.push_back(std::move(b));
  if (m->round_open) ij_check_round_batch(m);
}

// Assemble of an update round.  Locate / validate first, agree on the outcome (one host all-reduce on N > 1 ranks),
// then write: a refused round changes nothing on any rank.  host_only: the host arrays alone (CPU tests).
void ij_apply_round(IJMatrixObj *m, bool host_only) {
  Comm &comm = current_comm();
  int refused = m->round_refused ? 1 : 0;
  std::string why = "IJMatrixAssemble: a set call of this update round was refused; the round was discarded";
  const bool on_device = !host_only && !refused && !m->dev_batches.empty() && m->par.on_device;
  ij::UpdatePlan plan;
  if (!refused) {
    try {
      if (!on_device && !m->dev_batches.empty()) ij_demote(m);
      if (on_device && !ij::update_locate(m->ilower, m->iupper, m->jlower, m->jupper, m->dev_batches, m->par, plan)) {
        // a row outside this rank's range: the host check words the refusal (first entry in submission order)
        ij_demote(m);
        for (auto &b : m->batches) check_update_batch(m->par, m->jlower, m->jupper, b);
        fail(HYPRE_ERROR_GENERIC, "IJMatrix: a row of the update round is not owned by this rank");
      }
      if (!on_device)  // host batches were checked when they arrived; demoted device batches are checked here
        for (auto &b : m->batches) check_update_batch(m->par, m->jlower, m->jupper, b);
    } catch (const mi::Error &e) {
      refused = 1;
      why = e.what();
    }
  }
  if (comm.size > 1) {
    int any = refused;
    comm.allreduce_host(&any, 1, CommDType::I32, CommOp::MAX);
    if (any && !refused) why = "IJMatrixAssemble: another rank refused an entry of this update round; no rank's values changed";
    refused = any;
  }
  if (refused) {
    m->drop_round();
    fail(HYPRE_ERROR_GENERIC, why);
  }
  if (on_device) {
    std::vector<ij::UpdateConst> cs;
    for (auto &c : m->consts) {
      long long before = 0;
      for (size_t b = 0; b < std::min(c.before_batch, plan.batch_sizes.size()); b++) before += plan.batch_sizes[b];
      cs.push_back({before, c.value});
    }
    ij::update_apply(plan, cs, m->par);
    ij::counters().device_value_updates++;
  } else {
    update_parcsr_values(m->par, m->jlower, m->jupper, m->batches, m->consts);
    if (!host_only) refresh_device_values(m->par);
  }
  ij::counters().value_updates++;
  m->drop_round();
}

void vec_set(IJVectorObj *v, int n, const gidx *indices, const double *values, bool add) {
  if (!v->initialized) fail(HYPRE_ERROR_GENERIC, "IJVector: SetValues before Initialize");
  if (n <= 0) return;
  ensure_init();
  hipStream_t s = ctx().stream;
  std::vector<gidx> idx;
  DVec<int> dloc;
  const bool dev_idx = indices && ij::device_assembly_enabled() && is_device_pointer(indices);
  std::vector<int> loc(dev_idx ? (size_t)0 : (size_t)n);
  if (dev_idx) {
    // device indices: range check and conversion to local ids on the device
    dloc.alloc((size_t)n);
    ij::vec_local_ids(indices, n, v->jlower, v->jupper, dloc.p);
  } else if (indices) {
    fetch(indices, (size_t)n, idx, true);
    for (int i = 0; i < n; i++) {
      const gidx g = idx[(size_t)i];
      if (g < v->jlower || g > v->jupper) fail(HYPRE_ERROR_ARG, "IJVector: index outside the local range");
      loc[(size_t)i] = (int)(g - v->jlower);
    }
  } else {
    if (n > v->par.n) fail(HYPRE_ERROR_ARG, "IJVector: more values than local entries");
    for (int i = 0; i < n; i++) loc[(size_t)i] = i;
  }
  if (!dev_idx) dloc.upload(loc);
  DVec<double> dval;
  const double *src = values;
  if (!is_device_pointer(values)) {
    dval.alloc((size_t)n);
    dval.upload(values, (size_t)n);
    src = dval.p;
  }
  if (add)
    k::scatter_add(v->par.data(), dloc.p, src, n, s);
  else
    k::scatter_set(v->par.data(), dloc.p, src, n, s);
  MI_HIP(hipStreamSynchronize(s));
}

int stub_fail(const char *family) {
  return record_error(HYPRE_ERROR_GENERIC, std::string(family) +
                                               " is outside the north-star path of this library (GMRES/BiCGSTAB + "
                                               "BoomerAMG) and is not implemented");
}

// End of every collective Setup / Solve on more than one rank: a transport whose waits are bounded (the peer-store
// exchange) latches an error flag on the device when a wait expires and the kernels run on -- the halo was not
// delivered, a sum was taken over stale slots.  The flag is read here, agreed on by all ranks (so that they leave
// together and later collectives still match), the result is poisoned and the call fails (the plain HYPRE
// API used to return 0 with a silently wrong x).
void transport_gate(ParVector *x, const char *what) {
  Ctx &c = ctx();
  if (!c.inited || !c.comm || c.comm->size <= 1) return;
  if (!comm_transport_verdict(*c.comm, c.stream)) return;
  if (x && x->d.p && x->len() > 0) {
    k::fill(x->all(), x->len(), std::numeric_limits<double>::quiet_NaN(), c.stream);
    MI_HIP(hipStreamSynchronize(c.stream));
  }
  fail(HYPRE_ERROR_GENERIC, std::string(what) + ": the peer-store transport reported an expired wait on at least one rank "
                                "(MI_HYPRE_IPC_TIMEOUT_MS); the result is invalid and has been overwritten with NaN");
}

void write_ij_matrix(const ParCSR &A, const char *filename, int rank) {
  char fn[2048];
  snprintf(fn, sizeof(fn), "%s.%05d", filename, rank);
  FILE *fp = fopen(fn, "w");
  if (!fp) fail(HYPRE_ERROR_GENERIC, std::string("cannot open ") + fn);
  fprintf(fp, "%lld %lld %lld %lld\n", (long long)A.row_start, (long long)A.row_end - 1, (long long)A.row_start,
          (long long)A.row_end - 1);
  for (int i = 0; i < A.nrows; i++) {
    // merge diag and offd in ascending global column order
    std::vector<std::pair<gidx, double>> row;
    for (int64_t k = A.diag.ia[(size_t)i]; k < A.diag.ia[(size_t)i + 1]; k++)
      row.push_back({A.row_start + A.diag.ja[(size_t)k], A.diag.a[(size_t)k]});
    for (int64_t k = A.offd.ia[(size_t)i]; k < A.offd.ia[(size_t)i + 1]; k++)
      row.push_back({A.col_map_offd[(size_t)A.offd.ja[(size_t)k]], A.offd.a[(size_t)k]});
    std::sort(row.begin(), row.end());
    for (auto &e : row) fprintf(fp, "%lld %lld %.14e\n", (long long)(A.row_start + i), (long long)e.first, e.second);
  }
  fclose(fp);
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ utilities
HYPRE_Int HYPRE_Initialize(void) {
  API_BEGIN
  ensure_init();
  API_END
}
HYPRE_Int HYPRE_Init(void) { return HYPRE_Initialize(); }
HYPRE_Int HYPRE_Initialized(void) { return ctx().inited ? 1 : 0; }
HYPRE_Int HYPRE_Finalize(void) {
  API_BEGIN
  Ctx &c = ctx();
  if (c.inited) {
    MI_HIP(hipDeviceSynchronize());
    delete c.timer;
    c.timer = nullptr;
    c.comm.reset();
    c.red_partials.release();
    c.red_out.release();
    c.red_ticket.release();
    dev_pool_trim();
    if (c.h_pinned) (void)hipHostFree(c.h_pinned);
    c.h_pinned = nullptr;
    if (c.stream) (void)hipStreamDestroy(c.stream);
    c.stream = nullptr;
    c.inited = false;
  }
  API_END
}
HYPRE_Int HYPRE_GetError(void) { return g_error_flag; }
HYPRE_Int HYPRE_ClearAllErrors(void) {
  g_error_flag = 0;
  g_last_error.clear();
  return 0;
}
const char *HYPRE_MI_LastErrorMessage(void) { return g_last_error.c_str(); }
void HYPRE_DescribeError(HYPRE_Int errorcode, char *descr) {
  if (!descr) return;
  std::string t;
  if (errorcode == 0) t = "[No error] ";
  if (errorcode & HYPRE_ERROR_GENERIC) t += "[Generic error] ";
  if (errorcode & HYPRE_ERROR_MEMORY) t += "[Memory error] ";
  if (errorcode & HYPRE_ERROR_ARG) t += "[Error in argument] ";
  if (errorcode & HYPRE_ERROR_CONV) t += "[Method did not converge] ";
  // HYPRE's own texts are short fixed strings (its longest fits 128 bytes): a caller's HYPRE-sized buffer must not
  // overflow, so the appended message of the last failure is cut to what is left of 128 bytes
  if (errorcode != 0 && !g_last_error.empty()) t += g_last_error;
  snprintf(descr, 128, "%s", t.c_str());
}

HYPRE_Int HYPRE_SetMemoryLocation(HYPRE_MemoryLocation loc) {
  if (loc != HYPRE_MEMORY_DEVICE)
    return record_error(HYPRE_ERROR_ARG, "HYPRE_SetMemoryLocation: only HYPRE_MEMORY_DEVICE is implemented (no CPU path)");
  return 0;
}
HYPRE_Int HYPRE_SetExecutionPolicy(HYPRE_ExecutionPolicy pol) {
  if (pol != HYPRE_EXEC_DEVICE)
    return record_error(HYPRE_ERROR_ARG, "HYPRE_SetExecutionPolicy: only HYPRE_EXEC_DEVICE is implemented (no CPU path)");
  return 0;
}
HYPRE_Int HYPRE_SetGPUMemoryPoolSize(HYPRE_Int, HYPRE_Int, HYPRE_Int, size_t) { return 0; }
HYPRE_Int hypre_SetCubMemPoolSize(unsigned, unsigned, unsigned, size_t) { return 0; }
HYPRE_Int HYPRE_SetUmpireDevicePoolName(const char *) { return 0; }
// the reference's device pool (umpire_device_pool_mbs, src/main.cpp:107-114): its initial size is what this library's arena
// maps ahead of demand, in the background (runtime.cpp); before HYPRE_Init (no device yet) the call does nothing
HYPRE_Int HYPRE_SetUmpireDevicePoolSize(size_t nbytes) {
  API_BEGIN
  if (ctx().inited) dev_arena_reserve(nbytes);
  API_END
}
HYPRE_Int HYPRE_SetSpGemmUseVendor(HYPRE_Int) { return 0; }
HYPRE_Int HYPRE_SetSpMVUseVendor(HYPRE_Int) { return 0; }
HYPRE_Int HYPRE_SetSpTransUseVendor(HYPRE_Int) { return 0; }
HYPRE_Int hypre_ResetDeviceRandGenerator(unsigned long long, unsigned long long) { return 0; }

void *hypre_MAlloc(size_t bytes, HYPRE_MemoryLocation loc) {
  if (bytes == 0) return nullptr;
  if (loc == HYPRE_MEMORY_DEVICE) {
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
      record_error(HYPRE_ERROR_MEMORY, "hypre_MAlloc: hipMalloc of " + std::to_string(bytes) + " bytes failed");
      return nullptr;
    }
    return p;
  }
  return malloc(bytes);
}
void *hypre_CAlloc(size_t count, size_t elt, HYPRE_MemoryLocation loc) {
  void *p = hypre_MAlloc(count * elt, loc);
  if (!p) return p;
  if (loc == HYPRE_MEMORY_DEVICE) {
    (void)hipMemset(p, 0, count * elt);
    (void)hipDeviceSynchronize();  // the caller may hand the buffer to any stream next
  } else
    memset(p, 0, count * elt);
  return p;
}
void hypre_Free(void *ptr, HYPRE_MemoryLocation loc) {
  if (!ptr) return;
  if (loc == HYPRE_MEMORY_DEVICE)
    (void)hipFree(ptr);
  else
    free(ptr);
}
void hypre_Memcpy(void *dst, const void *src, size_t bytes, HYPRE_MemoryLocation, HYPRE_MemoryLocation) {
  if (!bytes) return;
  if (ctx().inited) (void)hipStreamSynchronize(ctx().stream);  // library kernels may still be producing src
  if (hipMemcpy(dst, src, bytes, hipMemcpyDefault) != hipSuccess)
    record_error(HYPRE_ERROR_GENERIC, "hypre_Memcpy failed");
}

// ------------------------------------------------------------------ IJ matrix
HYPRE_Int HYPRE_IJMatrixCreate(MPI_Comm, HYPRE_BigInt ilower, HYPRE_BigInt iupper, HYPRE_BigInt jlower,
                               HYPRE_BigInt jupper, HYPRE_IJMatrix *matrix) {
  API_BEGIN
  if (!matrix) fail(HYPRE_ERROR_ARG, "IJMatrixCreate: NULL output");
  if (iupper < ilower - 1 || jupper < jlower - 1) fail(HYPRE_ERROR_ARG, "IJMatrixCreate: bad range");
  IJMatrixObj *m = new IJMatrixObj();
  m->ilower = ilower;
  m->iupper = iupper;
  m->jlower = jlower;
  m->jupper = jupper;
  m->par.row_start = ilower;
  m->par.row_end = iupper + 1;
  m->par.nrows = (int)(iupper - ilower + 1);
  *matrix = reinterpret_cast<HYPRE_IJMatrix>(m);
  // The row count is the first thing known about the problem: the arena's grow-ahead thread starts mapping now (1 KiB per
  // row -- a 7-point operator with its hierarchy, work vectors and a GMRES(50) basis ends at 1.3 KiB per row; Assemble and
  // Setup refine the figure), while the caller is still generating or reading the entries.  On a device whose memory the
  // driver has to clear first (30 ms per GiB, the first process on a box) that is 4 s of driver time which otherwise runs
  // beside the setup and slows it by a third (setup_s 3.0 against 2.3 s at 512^3).
  if (m->par.nrows > 0) dev_arena_hint((size_t)m->par.nrows * 1024);
  API_END
}
HYPRE_Int HYPRE_IJMatrixDestroy(HYPRE_IJMatrix matrix) {
  API_BEGIN
  delete M(matrix);
  API_END
}
HYPRE_Int HYPRE_IJMatrixSetObjectType(HYPRE_IJMatrix, HYPRE_Int type) {
  if (type != HYPRE_PARCSR) return record_error(HYPRE_ERROR_ARG, "IJMatrixSetObjectType: only HYPRE_PARCSR");
  return 0;
}
HYPRE_Int HYPRE_IJMatrixInitialize(HYPRE_IJMatrix matrix) {
  API_BEGIN
  if (!matrix) fail(HYPRE_ERROR_ARG, "IJMatrixInitialize: NULL handle");
  // on an assembled matrix: an update round opens and the stored values stay (as in HYPRE)
  if (M(matrix)->assembled)
    ij_open_round(M(matrix));
  else
    ensure_init();
  API_END
}
HYPRE_Int HYPRE_IJMatrixGetObject(HYPRE_IJMatrix matrix, void **object) {
  API_BEGIN
  if (!matrix || !object) fail(HYPRE_ERROR_ARG, "IJMatrixGetObject: NULL argument");
  *object = &M(matrix)->par;
  API_END
}
HYPRE_Int HYPRE_IJMatrixSetConstantValues(HYPRE_IJMatrix matrix, HYPRE_Complex value) {
  API_BEGIN
  IJMatrixObj *m = M(matrix);
  if (!m) fail(HYPRE_ERROR_ARG, "IJMatrixSetConstantValues: NULL handle");
  if (m->assembled) {
    ij_open_round(m);
    if (!m->round_refused) m->consts.push_back({m->batches.size() + m->dev_batches.size(), value});
    return 0;
  }
  for (auto &b : m->batches) std::fill(b.vals.begin(), b.vals.end(), value);
  for (auto &d : m->dev_batches) ij::fill_values(d, value);
  API_END
}
HYPRE_Int HYPRE_IJMatrixSetValues2(HYPRE_IJMatrix matrix, HYPRE_Int nrows, HYPRE_Int *ncols, const HYPRE_BigInt *rows,
                                   const HYPRE_Int *row_indexes, const HYPRE_BigInt *cols,
                                   const HYPRE_Complex *values) {
  API_BEGIN
  ij_stage(M(matrix), nrows, ncols, rows, row_indexes, cols, values, false);
  API_END
}
HYPRE_Int HYPRE_IJMatrixAddToValues2(HYPRE_IJMatrix matrix, HYPRE_Int nrows, HYPRE_Int *ncols,
                                     const HYPRE_BigInt *rows, const HYPRE_Int *row_indexes,
                                     const HYPRE_BigInt *cols, const HYPRE_Complex *values) {
  API_BEGIN
  ij_stage(M(matrix), nrows, ncols, rows, row_indexes, cols, values, true);
  API_END
}
HYPRE_Int HYPRE_IJMatrixSetValues(HYPRE_IJMatrix matrix, HYPRE_Int nrows, HYPRE_Int *ncols, const HYPRE_BigInt *rows,
                                  const HYPRE_BigInt *cols, const HYPRE_Complex *values) {
  return HYPRE_IJMatrixSetValues2(matrix, nrows, ncols, rows, nullptr, cols, values);
}
HYPRE_Int HYPRE_IJMatrixAddToValues(HYPRE_IJMatrix matrix, HYPRE_Int nrows, HYPRE_Int *ncols,
                                    const HYPRE_BigInt *rows, const HYPRE_BigInt *cols, const HYPRE_Complex *values) {
  return HYPRE_IJMatrixAddToValues2(matrix, nrows, ncols, rows, nullptr, cols, values);
}
HYPRE_Int HYPRE_IJMatrixAssemble(HYPRE_IJMatrix matrix) {
  API_BEGIN
  IJMatrixObj *m = M(matrix);
  if (!m) fail(HYPRE_ERROR_ARG, "IJMatrixAssemble: NULL handle");
  if (m->device_failed)
    fail(HYPRE_ERROR_GENERIC, "IJMatrixAssemble: an earlier assembly of this matrix failed and its entries are gone; "
                              "create the matrix and set its values again");
  if (m->assembled && m->round_open) {
    ij_apply_round(m, false);
    return 0;
  }
  if (!m->assembled && !m->dev_batches.empty()) {
    // every batch arrived in device memory: sorted, folded and split there (ij_assembly.hip); the diag block is
    // already on the device when its solve format is built.  The matrix counts as assembled only when all of it
    // succeeded; a failure (a refusal, out of memory) leaves it unusable instead of half built -- a second Assemble
    // must not find consumed batches and build an empty matrix.
    Comm &comm = current_comm();
    try {
      sk::DCsr diag;
      ij::assemble_parcsr_device(comm, m->ilower, m->iupper, m->jlower, m->jupper, m->dev_batches, m->par, diag);
      m->par.build_halo_plan(comm);
      dev_arena_hint((size_t)13 * 12 * (size_t)(diag.nnz + m->par.offd.nnz()));
      ij::finish_device(m->par, diag);
    } catch (...) {
      m->device_failed = true;
      m->dev_batches.clear();
      throw;
    }
    m->assembled = true;
    return 0;
  }
  if (!m->assembled) {
    Comm &comm = current_comm();
    assemble_parcsr(comm, m->ilower, m->iupper, m->jlower, m->jupper, m->batches, m->par);
    m->par.build_halo_plan(comm);
    m->assembled = true;
  }
  // what a BoomerAMG hierarchy of this operator will need (operator complexity 3-4, sub-operators, transfer operators,
  // the setup's transients: ~13x the operator's bytes at 512^3): mapped in the background from now on
  dev_arena_hint((size_t)13 * 12 * (size_t)(m->par.diag.nnz() + m->par.offd.nnz()));
  if (!m->par.on_device) m->par.to_device();
  API_END
}
HYPRE_Int HYPRE_MI_IJMatrixAssembleHostOnly(HYPRE_IJMatrix matrix) {
  API_BEGIN
  IJMatrixObj *m = M(matrix);
  if (!m) fail(HYPRE_ERROR_ARG, "IJMatrixAssembleHostOnly: NULL handle");
  if (m->assembled && m->round_open) {
    ij_apply_round(m, true);
    return 0;
  }
  if (!m->assembled) {
    if (!m->dev_batches.empty()) ij_demote(m);
    Comm &comm = current_comm();
    assemble_parcsr(comm, m->ilower, m->iupper, m->jlower, m->jupper, m->batches, m->par);
    m->par.build_halo_plan(comm);
    m->assembled = true;
  }
  API_END
}
// inspection of an assembled matrix: which 0 host diag block, 1 host offd block (compressed columns: GetColMapOffd),
// 2 the diag block as the device solve format holds it
static void parcsr_block(ParCSR &A, int which, HostCSR &tmp, const HostCSR *&blk) {
  if (which == 0)
    blk = &A.diag;
  else if (which == 1)
    blk = &A.offd;
  else if (which == 2) {
    if (!A.on_device) fail(HYPRE_ERROR_GENERIC, "ParCSRGetCSR: the matrix has no device mirror");
    sk::solve_format_to_host(A.d_diag, tmp, ctx().stream);
    blk = &tmp;
  } else
    fail(HYPRE_ERROR_ARG, "ParCSRGetCSR: which must be 0, 1 or 2");
}
HYPRE_Int HYPRE_MI_ParCSRGetAssemblyStamp(HYPRE_ParCSRMatrix A, unsigned long long *stamp) {
  API_BEGIN
  if (!A || !stamp) fail(HYPRE_ERROR_ARG, "ParCSRGetAssemblyStamp: NULL argument");
  *stamp = PM(A)->assembly_stamp;
  API_END
}
HYPRE_Int HYPRE_MI_ParCSRGetValueKind(HYPRE_ParCSRMatrix A, HYPRE_Int *kind) {
  API_BEGIN
  if (!A || !kind) fail(HYPRE_ERROR_ARG, "ParCSRGetValueKind: NULL argument");
  if (!PM(A)->on_device) fail(HYPRE_ERROR_GENERIC, "ParCSRGetValueKind: the matrix has no device mirror");
  *kind = PM(A)->d_diag.reported_value_kind();
  API_END
}
HYPRE_Int HYPRE_MI_ParCSRGetCSRSize(HYPRE_ParCSRMatrix A, HYPRE_Int which, HYPRE_Int *nrows, HYPRE_Int *ncols,
                                    HYPRE_BigInt *nnz) {
  API_BEGIN
  if (!A) fail(HYPRE_ERROR_ARG, "ParCSRGetCSRSize: NULL matrix");
  ParCSR &P = *PM(A);
  if (which == 2) {
    if (!P.on_device) fail(HYPRE_ERROR_GENERIC, "ParCSRGetCSRSize: the matrix has no device mirror");
    *nrows = P.d_diag.nrows, *ncols = P.d_diag.ncols, *nnz = P.d_diag.nnz;
    return 0;
  }
  if (which != 0 && which != 1) fail(HYPRE_ERROR_ARG, "ParCSRGetCSRSize: which must be 0, 1 or 2");
  const HostCSR &h = which == 0 ? P.diag : P.offd;
  *nrows = h.nrows, *ncols = h.ncols, *nnz = h.nnz();
  API_END
}
HYPRE_Int HYPRE_MI_ParCSRGetCSR(HYPRE_ParCSRMatrix A, HYPRE_Int which, HYPRE_BigInt *ia, HYPRE_Int *ja, HYPRE_Complex *a) {
  API_BEGIN
  if (!A) fail(HYPRE_ERROR_ARG, "ParCSRGetCSR: NULL matrix");
  HostCSR tmp;
  const HostCSR *h = nullptr;
  parcsr_block(*PM(A), which, tmp, h);
  if (ia) {
    if (h->ia.empty())
      std::fill(ia, ia + h->nrows + 1, (HYPRE_BigInt)0);
    else
      std::copy(h->ia.begin(), h->ia.end(), ia);
  }
  if (ja) std::copy(h->ja.begin(), h->ja.begin() + h->nnz(), ja);
  if (a) std::copy(h->a.begin(), h->a.begin() + h->nnz(), a);
  API_END
}
HYPRE_Int HYPRE_MI_ParCSRGetColMapOffd(HYPRE_ParCSRMatrix A, HYPRE_BigInt *col_map_offd) {
  API_BEGIN
  if (!A || !col_map_offd) fail(HYPRE_ERROR_ARG, "ParCSRGetColMapOffd: NULL argument");
  std::copy(PM(A)->col_map_offd.begin(), PM(A)->col_map_offd.end(), col_map_offd);
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGSetupHostOnly(HYPRE_Solver solver, HYPRE_ParCSRMatrix A) {
  API_BEGIN
  if (!A) fail(HYPRE_ERROR_ARG, "BoomerAMGSetupHostOnly: NULL matrix");
  AMG(solver)->amg.setup_entry(*PM(A), true);  // host threads only
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGSetSetupReuse(HYPRE_Solver solver, HYPRE_Int mode) {
  API_BEGIN
  if (mode != 0 && mode != 1)
    fail(HYPRE_ERROR_ARG, "BoomerAMGSetSetupReuse: mode " + std::to_string(mode) + " is not implemented (0 = every Setup builds from "
                          "scratch and 1 = refresh the values on the kept structure are)");
  AMG(solver)->amg.setup_reuse = mode;
  API_END
}
const char *HYPRE_MI_SetupReuseReasonText(HYPRE_Int reason) { return setup_reuse_reason_text((int)reason); }
HYPRE_Int HYPRE_MI_BoomerAMGGetSetupKind(HYPRE_Solver solver, HYPRE_Int *kind, HYPRE_Int *reason) {
  API_BEGIN
  if (!kind || !reason) fail(HYPRE_ERROR_ARG, "BoomerAMGGetSetupKind: NULL output");
  *kind = AMG(solver)->amg.setup_kind;
  *reason = AMG(solver)->amg.setup_reason;
  API_END
}
// The setup-reuse kernels on caller (host) CSR arrays (64-bit row pointers, columns ascending).
// op 0: c_a[stored entry (i, j) of C] = (P^T (A P))_ij in the order contract of the refresh; B = P, R = P^T is formed
//       here (sk::transpose); `lanes` (0, 1, 2, ... 64) = lanes per coarse row, 0 = the library's choice.
// op 1: c_a[stored entry (r, c) of C] = A[rowmap[r], colmap[c]] (null maps: identity).
// *bad_row = -1, or the first row of C that does not fit (then c_a is untouched and the call returns an error).
HYPRE_Int HYPRE_MI_CSRReuseOp(HYPRE_Int op, HYPRE_Int a_nrows, HYPRE_Int a_ncols, const HYPRE_BigInt *a_ia, const HYPRE_Int *a_ja,
                              const HYPRE_Complex *a_a, HYPRE_Int b_nrows, HYPRE_Int b_ncols, const HYPRE_BigInt *b_ia,
                              const HYPRE_Int *b_ja, const HYPRE_Complex *b_a, const HYPRE_Int *rowmap, const HYPRE_Int *colmap,
                              HYPRE_Int lanes, HYPRE_Int c_nrows, HYPRE_Int c_ncols, const HYPRE_BigInt *c_ia,
                              const HYPRE_Int *c_ja, HYPRE_Complex *c_a, HYPRE_Int *bad_row) {
  API_BEGIN
  const std::string who = "CSRReuseOp";
  if (!a_ia || !c_ia || !c_a || !bad_row) fail(HYPRE_ERROR_ARG, who + ": NULL argument");
  check_lanes(who, lanes);
  ensure_init();
  hipStream_t s = ctx().stream;
  sk::DCsr dA, dC;
  dA.upload(csr_of(who, "A", a_nrows, a_ncols, a_ia, a_ja, a_a), s);
  dC.upload(csr_of(who, "C", c_nrows, c_ncols, c_ia, c_ja, nullptr), s);
  int bad = -1;
  if (op == 0) {
    if (!b_ia) fail(HYPRE_ERROR_ARG, "CSRReuseOp: the product needs P");
    if (a_ncols != b_nrows || a_nrows != b_nrows || c_nrows != b_ncols || c_ncols != b_ncols)
      fail(HYPRE_ERROR_ARG, "CSRReuseOp: the dimensions of A, P and C do not fit");
    sk::DCsr dP, dR;
    dP.upload(csr_of(who, "P", b_nrows, b_ncols, b_ia, b_ja, b_a), s);
    sk::transpose(dP, dR, s);
    bad = sk::galerkin_values(sk::ref_of(dA), sk::ref_of(dP), sk::ref_of(dR), nullptr, sk::ref_of(dC), dC.a.p, lanes, s);
  } else if (op == 1) {
    if (c_nrows > 0 && rowmap)
      for (HYPRE_Int r = 0; r < c_nrows; r++)
        if (rowmap[r] < 0 || rowmap[r] >= a_nrows) fail(HYPRE_ERROR_ARG, "CSRReuseOp: rowmap out of range");
    if (!rowmap && c_nrows > a_nrows) fail(HYPRE_ERROR_ARG, "CSRReuseOp: C has more rows than A");
    DVec<int> drow, dcol;
    if (rowmap) drow.upload(std::vector<int>(rowmap, rowmap + c_nrows));
    if (colmap) dcol.upload(std::vector<int>(colmap, colmap + c_ncols));
    bad = sk::value_lookup(sk::ref_of(dC), dC.a.p, rowmap ? drow.p : nullptr, colmap ? dcol.p : nullptr, sk::ref_of(dA), s);
  } else {
    fail(HYPRE_ERROR_ARG, "CSRReuseOp: op must be 0 (Galerkin values) or 1 (value lookup)");
  }
  *bad_row = bad;
  if (bad >= 0)
    fail(HYPRE_ERROR_GENERIC, "CSRReuseOp: internal error: row " + std::to_string(bad) + " of the pattern does not fit the source");
  if (dC.nnz) d2h(c_a, dC.a.p, (size_t)dC.nnz * sizeof(double), s);
  MI_HIP(hipStreamSynchronize(s));
  API_END
}
// The device routine of interp_type 16 / 17 (sk::mm_interp) on caller (host) arrays: A as CSR with ascending columns,
// the pattern of S (rows ascending), the marker (+1 C, -1 F, -3 special F).  P is malloc'ed (HYPRE_MI_Free).
// *bad_row = -1, or the first row with a zero denominator and a non-empty numerator: the call then fails, P is not made.
HYPRE_Int HYPRE_MI_MMInterpOp(HYPRE_Int type, HYPRE_Int n, const HYPRE_BigInt *a_ia, const HYPRE_Int *a_ja,
                              const HYPRE_Complex *a_a, const HYPRE_BigInt *s_ia, const HYPRE_Int *s_ja, const HYPRE_Int *cf,
                              HYPRE_Real trunc_factor, HYPRE_Int pmax, HYPRE_Int lanes, HYPRE_Int *p_ncols,
                              HYPRE_BigInt **p_ia, HYPRE_Int **p_ja, HYPRE_Complex **p_a, HYPRE_Int *bad_row) {
  API_BEGIN
  const std::string who = "MMInterpOp";
  if (!a_ia || !s_ia || !p_ncols || !p_ia || !p_ja || !p_a || !bad_row) fail(HYPRE_ERROR_ARG, who + ": NULL argument");
  if (type != 16 && type != 17) fail(HYPRE_ERROR_ARG, who + ": type must be 16 (extended) or 17 (extended+i)");
  check_lanes(who, lanes);
  if (n < 0 || a_ia[0] != 0 || s_ia[0] != 0) fail(HYPRE_ERROR_ARG, who + ": bad dimensions");
  if (a_ia[n] > 0 && !a_a) fail(HYPRE_ERROR_ARG, who + ": NULL values of A");
  check_marker(who, cf, n, true);
  const HostCSR hA = csr_of(who, "A", n, n, a_ia, a_ja, a_a), hS = csr_of(who, "S", n, n, s_ia, s_ja, nullptr);
  ensure_init();
  hipStream_t s = ctx().stream;
  sk::DCsr dA, dS, dP;
  dA.upload(hA, s);
  dS.upload(hS, s);
  DVec<int> dcf;
  dcf.upload(std::vector<int>(cf, cf + n));
  int nc = 0;
  const int bad = sk::mm_interp(dA, dS, dcf, type, trunc_factor, pmax, dP, nc, s, lanes);
  *bad_row = bad;
  if (bad >= 0)
    fail(HYPRE_ERROR_ARG, who + ": interp_type " + std::to_string(type) + ": row " + std::to_string(bad) +
                              " has a zero denominator d_i with a non-empty numerator");
  HostCSR hp;
  if (n > 0) dP.download(hp, s);
  *p_ncols = nc;
  csr_to_caller(hp, n, p_ia, p_ja, p_a);
  API_END
}
// The approximate ideal restriction (restriction 1) on caller (host) arrays: the device routine sk::air_restriction
// (on_host = 0) or the host routine hs::build_air_restriction (on_host = 1, no device needed).  info[8]: status (0 built,
// 1 not built -- a neighbourhood above 64 entries, the device routine only --, 2 singular local system), the largest
// |N_i|, the C rows with an empty N_i, the entries the filter dropped, the rows of the 16- / 32- / 64-lane
// instantiation, the first singular row (-1).  Status 2 fails the call; status 1 does not, and R stays NULL.
HYPRE_Int HYPRE_MI_AIRRestrictionOp(HYPRE_Int on_host, HYPRE_Int n, const HYPRE_BigInt *a_ia, const HYPRE_Int *a_ja,
                                    const HYPRE_Complex *a_a, const HYPRE_Int *cf, HYPRE_Real strong_threshold_r,
                                    HYPRE_Real filter_threshold_r, HYPRE_Int *r_nrows, HYPRE_BigInt **r_ia, HYPRE_Int **r_ja,
                                    HYPRE_Complex **r_a, HYPRE_Int info[8]) {
  API_BEGIN
  const std::string who = "AIRRestrictionOp";
  if (!a_ia || !cf || !r_nrows || !r_ia || !r_ja || !r_a || !info) fail(HYPRE_ERROR_ARG, who + ": NULL argument");
  if (n < 1 || a_ia[0] != 0) fail(HYPRE_ERROR_ARG, who + ": bad dimensions");
  if (a_ia[n] > 0 && !a_a) fail(HYPRE_ERROR_ARG, who + ": NULL values of A");
  if (!(strong_threshold_r >= 0.0) || !(filter_threshold_r >= 0.0)) fail(HYPRE_ERROR_ARG, who + ": thresholds must be >= 0");
  const int nc = check_marker(who, cf, n, false);
  if (nc == 0) fail(HYPRE_ERROR_ARG, who + ": the marker has no C point");
  const HostCSR hA = csr_of(who, "A", n, n, a_ia, a_ja, a_a);
  *r_nrows = nc;
  *r_ia = nullptr, *r_ja = nullptr, *r_a = nullptr;
  sk::AirInfo ai;
  HostCSR hr;
  int status = 0;
  if (on_host) {
    status = hs::build_air_restriction(hA, std::vector<int>(cf, cf + n), strong_threshold_r, filter_threshold_r, hr, ai) >= 0 ? 2 : 0;
  } else {
    ensure_init();
    hipStream_t s = ctx().stream;
    sk::DCsr dA, dR;
    dA.upload(hA, s);
    DVec<int> dcf;
    dcf.upload(std::vector<int>(cf, cf + n));
    status = sk::air_restriction(dA, dcf.p, strong_threshold_r, filter_threshold_r, dR, ai, s);
    if (status == 0) dR.download(hr, s);
  }
  const HYPRE_Int v[8] = {status, ai.max_m, ai.zero_rows, (HYPRE_Int)ai.dropped, ai.group_rows[0], ai.group_rows[1],
                          ai.group_rows[2], ai.bad_row};
  for (int i = 0; i < 8; i++) info[i] = v[i];
  if (status == 2)
    fail(HYPRE_ERROR_ARG, who + ": row " + std::to_string(ai.bad_row) + " has a singular local system A[N_i, N_i]");
  if (status == 0) csr_to_caller(hr, nc, r_ia, r_ja, r_a);
  API_END
}
// FSAI with the adaptive pattern (fsai_algo_type 4) on caller (host) arrays: the device routine sk::fsai_adaptive
// (on_host = 0) or the host routine hs::build_fsai_adaptive (on_host = 1, no device needed).  table_slots: the slots of a
// row's candidate table in LDS (0 = the library's choice; a small power of two sends rows through the global-memory
// table; the result never depends on it).  info[8]: status (0 built, 2 a row failed), the largest row of G, the
// largest candidate count met, the rows that took the global-memory table, the rows stopped by the tolerance / for
// want of candidates / by max_steps, the first failing row (-1).  Status 2 fails the call and names the row.
HYPRE_Int HYPRE_MI_FSAIAdaptiveOp(HYPRE_Int on_host, HYPRE_Int n, const HYPRE_BigInt *b_ia, const HYPRE_Int *b_ja,
                                  const HYPRE_Complex *b_a, HYPRE_Int max_steps, HYPRE_Int max_step_size,
                                  HYPRE_Real kap_tolerance, HYPRE_Int table_slots, HYPRE_BigInt **g_ia, HYPRE_Int **g_ja,
                                  HYPRE_Complex **g_a, HYPRE_Int info[8]) {
  API_BEGIN
  const std::string who = "FSAIAdaptiveOp";
  if (!b_ia || !g_ia || !g_ja || !g_a || !info) fail(HYPRE_ERROR_ARG, who + ": NULL argument");
  if (n < 1 || b_ia[0] != 0) fail(HYPRE_ERROR_ARG, who + ": bad dimensions");
  if (b_ia[n] > 0 && !b_a) fail(HYPRE_ERROR_ARG, who + ": NULL values of B");
  if (table_slots < 0 || (table_slots & (table_slots - 1)) != 0)
    fail(HYPRE_ERROR_ARG, who + ": table_slots must be 0 or a power of two");
  FsaiSolver::check_adaptive(who, max_steps, max_step_size, kap_tolerance);
  const HostCSR hB = csr_of(who, "B", n, n, b_ia, b_ja, b_a);
  *g_ia = nullptr, *g_ja = nullptr, *g_a = nullptr;
  sk::FsaiAdaptiveInfo ai;
  HostCSR hg;
  if (on_host) {
    hs::build_fsai_adaptive(hB, max_steps, max_step_size, kap_tolerance, hg, ai);
  } else {
    ensure_init();
    hipStream_t s = ctx().stream;
    sk::DCsr dB, dG;
    dB.upload(hB, s);
    if (sk::fsai_adaptive(dB, max_steps, max_step_size, kap_tolerance, table_slots, dG, ai, s) == 0) dG.download(hg, s);
  }
  const HYPRE_Int v[8] = {ai.status, ai.max_row, ai.max_candidates, ai.overflow_rows, ai.stop_tolerance,
                          ai.stop_no_candidate, ai.stop_max_steps, ai.bad_row};
  for (int i = 0; i < 8; i++) info[i] = v[i];
  if (ai.status == 2)
    fail(HYPRE_ERROR_GENERIC, who + ": FSAI local solve failed in row " + std::to_string(ai.bad_row) +
                                  (ai.bad_kind == 1 ? " (singular local matrix)"
                                                    : " (y_last <= 0: the diagonal block is not positive definite there)"));
  csr_to_caller(hg, n, g_ia, g_ja, g_a);
  API_END
}
// One-point interpolation (interp_type 100) on caller (host) arrays: the device routine sk::one_point_interp (on_host = 0)
// or the host routine hs::build_one_point_interp (on_host = 1, no device needed).  The marker: +1 C, -1 F, -3 special F.
HYPRE_Int HYPRE_MI_OnePointInterpOp(HYPRE_Int on_host, HYPRE_Int n, const HYPRE_BigInt *a_ia, const HYPRE_Int *a_ja,
                                    const HYPRE_Complex *a_a, const HYPRE_BigInt *s_ia, const HYPRE_Int *s_ja,
                                    const HYPRE_Int *cf, HYPRE_Int *p_ncols, HYPRE_BigInt **p_ia, HYPRE_Int **p_ja,
                                    HYPRE_Complex **p_a) {
  API_BEGIN
  const std::string who = "OnePointInterpOp";
  if (!a_ia || !s_ia || !cf || !p_ncols || !p_ia || !p_ja || !p_a) fail(HYPRE_ERROR_ARG, who + ": NULL argument");
  if (n < 1 || a_ia[0] != 0 || s_ia[0] != 0) fail(HYPRE_ERROR_ARG, who + ": bad dimensions");
  if (a_ia[n] > 0 && !a_a) fail(HYPRE_ERROR_ARG, who + ": NULL values of A");
  check_marker(who, cf, n, true);
  const HostCSR hA = csr_of(who, "A", n, n, a_ia, a_ja, a_a), hS = csr_of(who, "S", n, n, s_ia, s_ja, nullptr);
  HostCSR hp;
  int nc = 0;
  if (on_host) {
    hs::Strength S;
    S.ia = hS.ia;
    S.ja = hS.ja;
    std::vector<int> m(cf, cf + n);
    hs::build_one_point_interp(hA, S, m, hp, nc);
  } else {
    ensure_init();
    hipStream_t s = ctx().stream;
    sk::DCsr dA, dS, dP;
    dA.upload(hA, s);
    dS.upload(hS, s);
    DVec<int> dcf;
    dcf.upload(std::vector<int>(cf, cf + n));
    sk::one_point_interp(dA, dS, dcf, dP, nc, s);
    dP.download(hp, s);
  }
  *p_ncols = nc;
  csr_to_caller(hp, n, p_ia, p_ja, p_a);
  API_END
}
// The same-function operator of a system with several unknowns on caller (host) arrays: the device kernel
// sk::same_function_filter (on_host = 0) or the host routine hs::filter_same_function (on_host = 1, no device needed)
HYPRE_Int HYPRE_MI_SameFunctionFilterOp(HYPRE_Int on_host, HYPRE_Int n, const HYPRE_BigInt *a_ia, const HYPRE_Int *a_ja,
                                        const HYPRE_Complex *a_a, const HYPRE_Int *dof, HYPRE_BigInt **out_ia,
                                        HYPRE_Int **out_ja, HYPRE_Complex **out_a) {
  API_BEGIN
  const std::string who = "SameFunctionFilterOp";
  if (!a_ia || !dof || !out_ia || !out_ja || !out_a) fail(HYPRE_ERROR_ARG, who + ": NULL argument");
  if (n < 1 || a_ia[0] != 0) fail(HYPRE_ERROR_ARG, who + ": bad dimensions");
  if (a_ia[n] > 0 && !a_a) fail(HYPRE_ERROR_ARG, who + ": NULL values of A");
  const HostCSR hA = csr_of(who, "A", n, n, a_ia, a_ja, a_a);
  HostCSR hf;
  if (on_host) {
    hs::filter_same_function(hA, std::vector<int>(dof, dof + n), hf);
  } else {
    ensure_init();
    hipStream_t s = ctx().stream;
    sk::DCsr dA, dF;
    dA.upload(hA, s);
    DVec<int> ddof;
    ddof.upload(std::vector<int>(dof, dof + n));
    sk::same_function_filter(dA, ddof.p, dF, s);
    dF.download(hf, s);
  }
  csr_to_caller(hf, n, out_ia, out_ja, out_a);
  API_END
}
// setup-phase sparse kernels on caller (host) CSR arrays; results are malloc'ed (HYPRE_MI_Free)
HYPRE_Int HYPRE_MI_CSRDeviceOp(HYPRE_Int op, HYPRE_Int a_nrows, HYPRE_Int a_ncols, const HYPRE_BigInt *a_ia,
                               const HYPRE_Int *a_ja, const HYPRE_Complex *a_a, HYPRE_Int b_nrows, HYPRE_Int b_ncols,
                               const HYPRE_BigInt *b_ia, const HYPRE_Int *b_ja, const HYPRE_Complex *b_a,
                               const HYPRE_Int *perm, const HYPRE_Int *colpos, HYPRE_Int *c_nrows, HYPRE_Int *c_ncols,
                               HYPRE_BigInt **c_ia, HYPRE_Int **c_ja, HYPRE_Complex **c_a) {
  API_BEGIN
  const std::string who = "CSRDeviceOp";
  if (!a_ia || !c_nrows || !c_ncols || !c_ia || !c_ja || !c_a) fail(HYPRE_ERROR_ARG, who + ": NULL argument");
  const HostCSR hA = csr_of(who, "A", a_nrows, a_ncols, a_ia, a_ja, a_a);
  ensure_init();
  hipStream_t s = ctx().stream;
  sk::DCsr dA, dB, dC;
  dA.upload(hA, s);
  switch (op) {
    case 0:
      if (!b_ia) fail(HYPRE_ERROR_ARG, "CSRDeviceOp: product needs B");
      dB.upload(csr_of(who, "B", b_nrows, b_ncols, b_ia, b_ja, b_a), s);
      sk::spgemm(dA, dB, dC, s);
      break;
    case 1: sk::transpose(dA, dC, s); break;
    case 2: {
      DVec<int> dperm, dpos;
      if (perm) dperm.upload(std::vector<int>(perm, perm + a_nrows));
      if (colpos) dpos.upload(std::vector<int>(colpos, colpos + a_ncols));
      sk::permute(dA, perm ? dperm.p : nullptr, colpos ? dpos.p : nullptr, dC, s);
      break;
    }
    default: fail(HYPRE_ERROR_ARG, "CSRDeviceOp: op must be 0 (A*B), 1 (A^T) or 2 (row permutation)");
  }
  HostCSR hc;
  dC.download(hc, s);
  *c_nrows = hc.nrows;
  *c_ncols = hc.ncols;
  csr_to_caller(hc, hc.nrows, c_ia, c_ja, c_a);
  API_END
}
HYPRE_Int HYPRE_MI_ParCSRGetHaloPlan(HYPRE_ParCSRMatrix A, HYPRE_Int *nsend_peers, HYPRE_Int *send_peers,
                                     HYPRE_Int *send_starts, HYPRE_Int *send_map, HYPRE_Int *nrecv_peers,
                                     HYPRE_Int *recv_peers, HYPRE_Int *recv_starts) {
  API_BEGIN
  if (!A) fail(HYPRE_ERROR_ARG, "ParCSRGetHaloPlan: NULL matrix");
  const HaloPlan &h = PM(A)->halo;
  *nsend_peers = (HYPRE_Int)h.send_peers.size();
  *nrecv_peers = (HYPRE_Int)h.recv_peers.size();
  if (send_peers) std::copy(h.send_peers.begin(), h.send_peers.end(), send_peers);
  if (send_starts) std::copy(h.send_starts.begin(), h.send_starts.end(), send_starts);
  if (send_map) std::copy(h.send_map.begin(), h.send_map.end(), send_map);
  if (recv_peers) std::copy(h.recv_peers.begin(), h.recv_peers.end(), recv_peers);
  if (recv_starts) std::copy(h.recv_starts.begin(), h.recv_starts.end(), recv_starts);
  API_END
}
HYPRE_Int HYPRE_IJMatrixPrint(HYPRE_IJMatrix matrix, const char *filename) {
  API_BEGIN
  IJMatrixObj *m = M(matrix);
  if (!m || !m->assembled) fail(HYPRE_ERROR_GENERIC, "IJMatrixPrint: matrix is not assembled");
  write_ij_matrix(m->par, filename, current_comm().rank);
  API_END
}
HYPRE_Int HYPRE_IJMatrixGetLocalRange(HYPRE_IJMatrix matrix, HYPRE_BigInt *ilower, HYPRE_BigInt *iupper,
                                      HYPRE_BigInt *jlower, HYPRE_BigInt *jupper) {
  API_BEGIN
  IJMatrixObj *m = M(matrix);
  if (!m) fail(HYPRE_ERROR_ARG, "IJMatrixGetLocalRange: NULL handle");
  *ilower = m->ilower;
  *iupper = m->iupper;
  *jlower = m->jlower;
  *jupper = m->jupper;
  API_END
}
HYPRE_Int HYPRE_IJMatrixSetMaxOnProcElmts(HYPRE_IJMatrix, HYPRE_Int) { return 0; }
HYPRE_Int HYPRE_IJMatrixSetOffProcSendElmts(HYPRE_IJMatrix, HYPRE_Int) { return 0; }
HYPRE_Int HYPRE_IJMatrixSetOffProcRecvElmts(HYPRE_IJMatrix, HYPRE_Int) { return 0; }
HYPRE_Int HYPRE_IJMatrixRead(const char *, MPI_Comm, HYPRE_Int, HYPRE_IJMatrix *) {
  return stub_fail("HYPRE_IJMatrixRead (dead code in the driver, src/HypreSystem.cpp:1086-1133)");
}

// ------------------------------------------------------------------ IJ vector
HYPRE_Int HYPRE_IJVectorCreate(MPI_Comm, HYPRE_BigInt jlower, HYPRE_BigInt jupper, HYPRE_IJVector *vector) {
  API_BEGIN
  if (!vector) fail(HYPRE_ERROR_ARG, "IJVectorCreate: NULL output");
  IJVectorObj *v = new IJVectorObj();
  v->jlower = jlower;
  v->jupper = jupper;
  *vector = reinterpret_cast<HYPRE_IJVector>(v);
  API_END
}
HYPRE_Int HYPRE_IJVectorDestroy(HYPRE_IJVector vector) {
  API_BEGIN
  delete V(vector);
  API_END
}
HYPRE_Int HYPRE_IJVectorSetObjectType(HYPRE_IJVector, HYPRE_Int type) {
  if (type != HYPRE_PARCSR) return record_error(HYPRE_ERROR_ARG, "IJVectorSetObjectType: only HYPRE_PARCSR");
  return 0;
}
HYPRE_Int HYPRE_IJVectorSetNumComponents(HYPRE_IJVector vector, HYPRE_Int n) {
  API_BEGIN
  IJVectorObj *v = V(vector);
  if (!v || n < 1) fail(HYPRE_ERROR_ARG, "IJVectorSetNumComponents: bad argument");
  if (v->initialized) fail(HYPRE_ERROR_GENERIC, "IJVectorSetNumComponents after Initialize");
  v->ncomp = n;
  API_END
}
HYPRE_Int HYPRE_IJVectorSetComponent(HYPRE_IJVector vector, HYPRE_Int c) {
  API_BEGIN
  IJVectorObj *v = V(vector);
  if (!v || c < 0 || c >= v->ncomp) fail(HYPRE_ERROR_ARG, "IJVectorSetComponent: component out of range");
  v->par.cur = c;
  API_END
}
HYPRE_Int HYPRE_IJVectorInitialize(HYPRE_IJVector vector) {
  API_BEGIN
  IJVectorObj *v = V(vector);
  if (!v) fail(HYPRE_ERROR_ARG, "IJVectorInitialize: NULL handle");
  ensure_init();
  v->par.init(v->jlower, v->jupper + 1, v->ncomp);
  v->initialized = true;
  API_END
}
HYPRE_Int HYPRE_IJVectorGetObject(HYPRE_IJVector vector, void **object) {
  API_BEGIN
  if (!vector || !object) fail(HYPRE_ERROR_ARG, "IJVectorGetObject: NULL argument");
  *object = &V(vector)->par;
  API_END
}
HYPRE_Int HYPRE_IJVectorSetValues(HYPRE_IJVector vector, HYPRE_Int nvalues, const HYPRE_BigInt *indices,
                                  const HYPRE_Complex *values) {
  API_BEGIN
  vec_set(V(vector), nvalues, indices, values, false);
  API_END
}
HYPRE_Int HYPRE_IJVectorAddToValues(HYPRE_IJVector vector, HYPRE_Int nvalues, const HYPRE_BigInt *indices,
                                    const HYPRE_Complex *values) {
  API_BEGIN
  vec_set(V(vector), nvalues, indices, values, true);
  API_END
}
HYPRE_Int HYPRE_IJVectorGetValues(HYPRE_IJVector vector, HYPRE_Int nvalues, const HYPRE_BigInt *indices,
                                  HYPRE_Complex *values) {
  API_BEGIN
  IJVectorObj *v = V(vector);
  if (!v || !v->initialized) fail(HYPRE_ERROR_GENERIC, "IJVectorGetValues: vector not initialised");
  if (nvalues <= 0) return 0;
  hipStream_t s = ctx().stream;
  const bool dev_out = is_device_pointer(values);
  if (!indices) {
    if (nvalues > v->par.n) fail(HYPRE_ERROR_ARG, "IJVectorGetValues: more values than local entries");
    MI_HIP(hipMemcpyAsync(values, v->par.data(), (size_t)nvalues * sizeof(double),
                          dev_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    return 0;
  }
  std::vector<gidx> idx;
  fetch(indices, (size_t)nvalues, idx);
  std::vector<int> loc((size_t)nvalues);
  for (int i = 0; i < nvalues; i++) {
    if (idx[(size_t)i] < v->jlower || idx[(size_t)i] > v->jupper)
      fail(HYPRE_ERROR_ARG, "IJVectorGetValues: index outside the local range");
    loc[(size_t)i] = (int)(idx[(size_t)i] - v->jlower);
  }
  DVec<int> dloc;
  dloc.upload(loc);
  DVec<double> tmp((size_t)nvalues);
  k::gather(v->par.data(), dloc.p, tmp.p, nvalues, s);
  MI_HIP(hipMemcpyAsync(values, tmp.p, (size_t)nvalues * sizeof(double),
                        dev_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
  MI_HIP(hipStreamSynchronize(s));
  API_END
}
HYPRE_Int HYPRE_IJVectorAssemble(HYPRE_IJVector vector) {
  API_BEGIN
  if (!vector) fail(HYPRE_ERROR_ARG, "IJVectorAssemble: NULL handle");
  API_END
}
HYPRE_Int HYPRE_IJVectorPrint(HYPRE_IJVector vector, const char *filename) {
  API_BEGIN
  IJVectorObj *v = V(vector);
  if (!v || !v->initialized) fail(HYPRE_ERROR_GENERIC, "IJVectorPrint: vector not initialised");
  std::vector<double> h((size_t)v->par.n);
  if (v->par.n) {
    MI_HIP(hipStreamSynchronize(ctx().stream));  // blocking copies are not ordered against the library stream
    d2h(h.data(), v->par.data(), h.size() * sizeof(double), nullptr);
  }
  char fn[2048];
  snprintf(fn, sizeof(fn), "%s.%05d", filename, current_comm().rank);
  FILE *fp = fopen(fn, "w");
  if (!fp) fail(HYPRE_ERROR_GENERIC, std::string("cannot open ") + fn);
  fprintf(fp, "%lld %lld\n", (long long)v->jlower, (long long)v->jupper);
  for (int i = 0; i < v->par.n; i++) fprintf(fp, "%lld %.14e\n", (long long)(v->jlower + i), h[(size_t)i]);
  fclose(fp);
  API_END
}
HYPRE_Int HYPRE_IJVectorSetMaxOnProcElmts(HYPRE_IJVector, HYPRE_Int) { return 0; }
HYPRE_Int HYPRE_IJVectorSetOffProcSendElmts(HYPRE_IJVector, HYPRE_Int) { return 0; }
HYPRE_Int HYPRE_IJVectorSetOffProcRecvElmts(HYPRE_IJVector, HYPRE_Int) { return 0; }
HYPRE_Int HYPRE_IJVectorRead(const char *, MPI_Comm, HYPRE_Int, HYPRE_IJVector *) {
  return stub_fail("HYPRE_IJVectorRead (dead code in the driver, src/HypreSystem.cpp:1086-1133)");
}

// ------------------------------------------------------------------ ParCSR / ParVector
HYPRE_Int HYPRE_ParCSRMatrixMatvec(HYPRE_Complex alpha, HYPRE_ParCSRMatrix A, HYPRE_ParVector x, HYPRE_Complex beta,
                                   HYPRE_ParVector y) {
  API_BEGIN
  if (!A || !x || !y) fail(HYPRE_ERROR_ARG, "ParCSRMatrixMatvec: NULL argument");
  ParCSR *a = PM(A);
  if (PV(x)->n != a->nrows || PV(y)->n != a->nrows) fail(HYPRE_ERROR_ARG, "ParCSRMatrixMatvec: size mismatch");
  a->matvec(current_comm(), alpha, PV(x)->data(), beta, PV(y)->data(), PV(y)->data(), ctx().stream, k::PROF_SPMV_L0);
  MI_HIP(hipStreamSynchronize(ctx().stream));
  API_END
}
HYPRE_Int HYPRE_MI_ParCSRMatrixMatvecMulti(HYPRE_Complex alpha, HYPRE_ParCSRMatrix A, HYPRE_ParVector x, HYPRE_Complex beta,
                                           HYPRE_ParVector y) {
  API_BEGIN
  if (!A || !x || !y) fail(HYPRE_ERROR_ARG, "ParCSRMatrixMatvecMulti: NULL argument");
  ParCSR *a = PM(A);
  if (PV(x)->n != a->nrows || PV(y)->n != a->nrows) fail(HYPRE_ERROR_ARG, "ParCSRMatrixMatvecMulti: size mismatch");
  if (PV(x)->ncomp != PV(y)->ncomp) fail(HYPRE_ERROR_ARG, "ParCSRMatrixMatvecMulti: x and y differ in their number of components");
  if (PV(x) == PV(y)) fail(HYPRE_ERROR_ARG, "ParCSRMatrixMatvecMulti: x and y are the same vector");
  const long long n = a->nrows;
  a->matvec_multi(current_comm(), PV(x)->ncomp, alpha, PV(x)->all(), n, beta, PV(y)->all(), n, PV(y)->all(), n, ctx().stream,
                  k::PROF_SPMV_L0);
  MI_HIP(hipStreamSynchronize(ctx().stream));
  API_END
}
HYPRE_Int HYPRE_ParCSRMatrixGetDims(HYPRE_ParCSRMatrix A, HYPRE_BigInt *Mr, HYPRE_BigInt *Nc) {
  API_BEGIN
  if (!A) fail(HYPRE_ERROR_ARG, "ParCSRMatrixGetDims: NULL handle");
  *Mr = *Nc = PM(A)->global_rows();
  API_END
}
HYPRE_Int HYPRE_ParCSRMatrixGetLocalRange(HYPRE_ParCSRMatrix A, HYPRE_BigInt *rs, HYPRE_BigInt *re, HYPRE_BigInt *cs,
                                          HYPRE_BigInt *ce) {
  API_BEGIN
  if (!A) fail(HYPRE_ERROR_ARG, "ParCSRMatrixGetLocalRange: NULL handle");
  *rs = *cs = PM(A)->row_start;
  *re = *ce = PM(A)->row_end - 1;
  API_END
}
HYPRE_Int hypre_ParCSRMatrixPrintIJ(const hypre_ParCSRMatrix *A, HYPRE_Int, HYPRE_Int, const char *filename) {
  API_BEGIN
  if (!A) fail(HYPRE_ERROR_ARG, "ParCSRMatrixPrintIJ: NULL handle");
  write_ij_matrix(*reinterpret_cast<const ParCSR *>(A), filename, current_comm().rank);
  API_END
}
HYPRE_Int HYPRE_ParVectorSetConstantValues(HYPRE_ParVector v, HYPRE_Complex value) {
  API_BEGIN
  if (!v) fail(HYPRE_ERROR_ARG, "ParVectorSetConstantValues: NULL handle");
  ParVector *p = PV(v);
  k::fill(p->d.p, p->n * p->ncomp, value, ctx().stream);
  MI_HIP(hipStreamSynchronize(ctx().stream));
  API_END
}
HYPRE_Int HYPRE_ParVectorInnerProd(HYPRE_ParVector x, HYPRE_ParVector y, HYPRE_Real *prod) {
  API_BEGIN
  if (!x || !y || !prod) fail(HYPRE_ERROR_ARG, "ParVectorInnerProd: NULL argument");
  *prod = par_dot_host(current_comm(), PV(x)->data(), PV(y)->data(), PV(x)->n, ctx().stream);
  API_END
}
HYPRE_Int HYPRE_ParVectorAxpy(HYPRE_Complex alpha, HYPRE_ParVector x, HYPRE_ParVector y) {
  API_BEGIN
  if (!x || !y) fail(HYPRE_ERROR_ARG, "ParVectorAxpy: NULL argument");
  k::axpy(alpha, PV(x)->data(), PV(y)->data(), PV(x)->n, ctx().stream);
  MI_HIP(hipStreamSynchronize(ctx().stream));
  API_END
}
HYPRE_Int HYPRE_ParVectorScale(HYPRE_Complex alpha, HYPRE_ParVector y) {
  API_BEGIN
  if (!y) fail(HYPRE_ERROR_ARG, "ParVectorScale: NULL argument");
  k::scale(alpha, PV(y)->data(), PV(y)->n, ctx().stream);
  MI_HIP(hipStreamSynchronize(ctx().stream));
  API_END
}
HYPRE_Int HYPRE_ParVectorCopy(HYPRE_ParVector x, HYPRE_ParVector y) {
  API_BEGIN
  if (!x || !y) fail(HYPRE_ERROR_ARG, "ParVectorCopy: NULL argument");
  k::copy(PV(x)->data(), PV(y)->data(), PV(x)->n, ctx().stream);
  MI_HIP(hipStreamSynchronize(ctx().stream));
  API_END
}

// ------------------------------------------------------------------ BoomerAMG
static void set_value_storage(AmgParams &p, int mode, int first_level) {
  if (mode < 0 || mode > 2)
    fail(HYPRE_ERROR_ARG, "value storage mode " + std::to_string(mode) + " is not implemented: 0 (fp64), 1 (fp32) or 2 (fp64 holding fp32-rounded values)");
  if (first_level < 1)
    fail(HYPRE_ERROR_ARG, "value storage first_level " + std::to_string(first_level) +
                              " < 1: level 0 is the operator the Krylov solver multiplies by and is never narrowed");
  p.value_storage = mode;
  p.value_first_level = first_level;
}
HYPRE_Int HYPRE_MI_BoomerAMGSetValueStorage(HYPRE_Solver solver, HYPRE_Int mode, HYPRE_Int first_level) {
  API_BEGIN
  set_value_storage(AMG(solver)->amg.p, mode, first_level);
  API_END
}
HYPRE_Int HYPRE_BoomerAMGCreate(HYPRE_Solver *solver) {
  API_BEGIN
  if (!solver) fail(HYPRE_ERROR_ARG, "BoomerAMGCreate: NULL output");
  std::unique_ptr<AmgSolver> a(new AmgSolver());
  const char *vs = getenv("MI_HYPRE_VALUE_STORAGE"), *vl = getenv("MI_HYPRE_VALUE_STORAGE_FIRST_LEVEL");
  set_value_storage(a->amg.p, vs ? atoi(vs) : 0, vl ? atoi(vl) : 1);
  *solver = reinterpret_cast<HYPRE_Solver>(static_cast<SolverBase *>(a.release()));
  API_END
}
HYPRE_Int HYPRE_BoomerAMGDestroy(HYPRE_Solver solver) {
  API_BEGIN
  delete S(solver);
  API_END
}
HYPRE_Int HYPRE_BoomerAMGSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector, HYPRE_ParVector) {
  API_BEGIN
  if (!A) fail(HYPRE_ERROR_ARG, "BoomerAMGSetup: NULL matrix");
  AMG(solver)->amg.setup(*PM(A));
  transport_gate(nullptr, "BoomerAMGSetup");
  API_END
}
HYPRE_Int HYPRE_BoomerAMGSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) {
  API_BEGIN
  if (!A || !b || !x) fail(HYPRE_ERROR_ARG, "BoomerAMGSolve: NULL argument");
  AMG(solver)->amg.solve(*PM(A), *PV(b), *PV(x));
  transport_gate(PV(x), "BoomerAMGSolve");
  API_END
}
// a setting this implementation accepts but does not act on: said once per key, on stderr, whatever print_level
static void warn_ignored(const char *key, double v) {
  static std::vector<std::string> seen;
  for (const auto &k : seen)
    if (k == key) return;
  seen.push_back(key);
  if (current_comm().rank == 0)
    fprintf(stderr, "mi_hypre BoomerAMG: %s = %g is accepted but NOT implemented; the setting has no effect\n", key, v);
}
// non_galerkin_tol / non_galerkin_level_tols (src/HypreSystem.cpp:161-176) select THIS library's drop-and-lump rule
// (DESIGN.md section 3), not the algorithm of HYPRE's par_nongalerkin.c, which is not restated (its source is not in the
// tree and the recollection of it is not reliable enough to claim it): the same YAML key builds another hierarchy than
// libHYPRE would.  Said once, on stderr, whatever print_level -- a user of the reference's inputs should not have to read
// DESIGN.md to learn it.
static void note_non_galerkin_rule(double v) {
  static bool said = false;
  if (said || !(v > 0.0)) return;
  said = true;
  if (current_comm().rank == 0)
    fprintf(stderr, "mi_hypre BoomerAMG: non-Galerkin tolerance %g: coarse operators are sparsified by this library's rule (an "
                    "entry below tol * min(row maxima) is lumped onto the diagonal), NOT by HYPRE's par_nongalerkin.c algorithm -- "
                    "hierarchy and iteration counts differ from libHYPRE's for this setting\n", v);
}
#define AMG_SET(NAME, TYPE, STMT)                               \
  HYPRE_Int HYPRE_BoomerAMGSet##NAME(HYPRE_Solver solver, TYPE v) { \
    API_BEGIN                                                   \
    AmgParams &p = AMG(solver)->amg.p;                          \
    (void)p;                                                    \
    STMT;                                                       \
    API_END                                                     \
  }
AMG_SET(PrintLevel, HYPRE_Int, p.print_level = v)
AMG_SET(DebugFlag, HYPRE_Int, p.debug_flag = v)
AMG_SET(CoarsenType, HYPRE_Int, p.coarsen_type = v)
AMG_SET(CycleType, HYPRE_Int, if (v != 1 && v != 2) fail(HYPRE_ERROR_ARG, "cycle_type must be 1 or 2"); p.cycle_type = v)
AMG_SET(RelaxType, HYPRE_Int, p.relax_type[0] = p.relax_type[1] = v; p.relax_type[2] = 9)
AMG_SET(NumSweeps, HYPRE_Int, if (v < 1) fail(HYPRE_ERROR_ARG, "num_sweeps < 1"); p.num_sweeps[0] = p.num_sweeps[1] = v; p.num_sweeps[2] = 1)
AMG_SET(SmoothNumSweeps, HYPRE_Int, p.smooth_num_sweeps = v)
AMG_SET(Tol, HYPRE_Real, p.tol = v)
AMG_SET(MaxIter, HYPRE_Int, p.max_iter = v)
AMG_SET(RelaxOrder, HYPRE_Int, p.relax_order = v)
AMG_SET(MaxLevels, HYPRE_Int, if (v < 1) fail(HYPRE_ERROR_ARG, "max_levels < 1"); p.max_levels = v)
AMG_SET(StrongThreshold, HYPRE_Real, p.strong_threshold = v)
AMG_SET(MaxRowSum, HYPRE_Real, p.max_row_sum = v)
/* num_functions < 1 is refused at Setup, like the combinations unknown-based AMG is not built for */
AMG_SET(NumFunctions, HYPRE_Int, p.num_functions = v)
HYPRE_Int HYPRE_BoomerAMGGetNumFunctions(HYPRE_Solver solver, HYPRE_Int *num_functions) {
  API_BEGIN
  if (!num_functions) fail(HYPRE_ERROR_ARG, "BoomerAMGGetNumFunctions: NULL argument");
  *num_functions = AMG(solver)->amg.p.num_functions;
  API_END
}
/* host or device memory, read and copied at every Setup with num_functions > 1; never freed here (NULL: the default) */
HYPRE_Int HYPRE_BoomerAMGSetDofFunc(HYPRE_Solver solver, HYPRE_Int *dof_func) {
  API_BEGIN
  AMG(solver)->amg.dof_func_user = dof_func;
  API_END
}
AMG_SET(InterpType, HYPRE_Int, p.interp_type = v)  /* unknown types are refused at Setup, like every other choice */
/* restriction: values the library does not build (2 and above, negative thresholds) are refused at Setup, by name */
AMG_SET(Restriction, HYPRE_Int, p.restriction = v)
AMG_SET(StrongThresholdR, HYPRE_Real, p.strong_threshold_r = v)
AMG_SET(FilterThresholdR, HYPRE_Real, p.filter_threshold_r = v)
AMG_SET(TruncFactor, HYPRE_Real, p.trunc_factor = v)
AMG_SET(PMaxElmts, HYPRE_Int, p.pmax_elmts = v)
AMG_SET(MinCoarseSize, HYPRE_Int, p.min_coarse_size = v)
AMG_SET(MaxCoarseSize, HYPRE_Int, p.max_coarse_size = v)
AMG_SET(SeqThreshold, HYPRE_Int, p.redundant_rows = (v < 0 ? 0 : v))
AMG_SET(RelaxWt, HYPRE_Real, p.relax_weight = v)
AMG_SET(OuterWt, HYPRE_Real, p.outer_weight = v)
AMG_SET(AggNumLevels, HYPRE_Int, p.agg_num_levels = v)
AMG_SET(AggInterpType, HYPRE_Int, p.agg_interp_type = v)
AMG_SET(AggPMaxElmts, HYPRE_Int, p.agg_pmax_elmts = v)
AMG_SET(AggTruncFactor, HYPRE_Real, p.agg_trunc_factor = v)
AMG_SET(AggP12MaxElmts, HYPRE_Int, p.agg_p12_max_elmts = v)
AMG_SET(AggP12TruncFactor, HYPRE_Real, p.agg_p12_trunc_factor = v)
HYPRE_Int HYPRE_MI_BoomerAMGSetKeepAggMarkers(HYPRE_Solver solver, HYPRE_Int keep) {
  API_BEGIN
  AMG(solver)->amg.p.keep_agg_markers = keep ? 1 : 0;
  API_END
}
AMG_SET(KeepTranspose, HYPRE_Int, p.keep_transpose = v)
AMG_SET(RAP2, HYPRE_Int, p.rap2 = v)
AMG_SET(Variant, HYPRE_Int, if (v != 0) warn_ignored("variant", v))
AMG_SET(NonGalerkinTol, HYPRE_Real, if (v < 0.0 || v > 1.0) fail(HYPRE_ERROR_ARG, "non_galerkin_tol must be in [0, 1]"); p.non_galerkin_tol = v; note_non_galerkin_rule(v))
AMG_SET(SmoothType, HYPRE_Int, p.smooth_type = v)  /* acts through smooth_num_levels > 0; checked at Setup */
AMG_SET(SmoothNumLevels, HYPRE_Int, p.smooth_num_levels = v)
AMG_SET(ILUType, HYPRE_Int, p.ilu_type = v)
AMG_SET(ILULevel, HYPRE_Int, p.ilu_level = v)
/* 2 = multicolour ordering (this library's number); HYPRE's 1 = RCM and anything else is ignored */
AMG_SET(ILULocalReordering, HYPRE_Int, if (v != 0 && v != 2) warn_ignored("ilu_reordering_type", v); p.ilu_reordering = v)
AMG_SET(ILUMaxRowNnz, HYPRE_Int, warn_ignored("ilu_max_row_nnz", v))
AMG_SET(ILUMaxIter, HYPRE_Int, if (v < 1) fail(HYPRE_ERROR_ARG, "ilu_max_iter < 1"); p.ilu_max_iter = v)
AMG_SET(ILUDroptol, HYPRE_Real, if (v != 0.0) warn_ignored("ilu_droptol", v))
AMG_SET(ILUIterSetupType, HYPRE_Int, p.ilu_iter_type = v)  /* 0 ... 4 with ILU(0); other combinations are refused at Setup */
AMG_SET(ILUIterSetupOption, HYPRE_Int, p.ilu_iter_option = v)
AMG_SET(ILUIterSetupMaxIter, HYPRE_Int, p.ilu_iter_max_iter = v)
AMG_SET(ILUIterSetupTolerance, HYPRE_Real, p.ilu_iter_tol = v)
AMG_SET(ILUTriSolve, HYPRE_Int, p.ilu_tri_solve = v)
AMG_SET(ILULowerJacobiIters, HYPRE_Int, p.ilu_lower_it = v)
AMG_SET(ILUUpperJacobiIters, HYPRE_Int, p.ilu_upper_it = v)
AMG_SET(FSAIAlgoType, HYPRE_Int, p.fsai_algo_type = v)  /* 3 (static pattern) and 4 (adaptive pattern, this library's number) are built: others are refused at Setup */
AMG_SET(FSAILocalSolveType, HYPRE_Int, (void)v)
AMG_SET(FSAINumLevels, HYPRE_Int, p.fsai_num_levels = v)
AMG_SET(FSAIThreshold, HYPRE_Real, if (v < 0.0) fail(HYPRE_ERROR_ARG, "fsai_threshold < 0"); p.fsai_threshold = v)
AMG_SET(FSAIEigMaxIters, HYPRE_Int, if (v < 0) fail(HYPRE_ERROR_ARG, "fsai_eig_max_iters < 0"); p.fsai_eig_max_iters = v)
/* the adaptive pattern's values (algo type 4), checked at Setup; with the static pattern they still do nothing, which is said once */
AMG_SET(FSAIMaxSteps, HYPRE_Int, p.fsai_max_steps = v; if (p.fsai_algo_type != 4) warn_ignored("fsai_max_steps", v))
/* relax type 16: stored here, checked at Setup like every other choice (order 1 ... 4, fraction in (0, 1), eig_est >= 0,
 * variant 0 and scale 1 are built) */
AMG_SET(ChebyOrder, HYPRE_Int, p.cheby_order = v)
AMG_SET(ChebyFraction, HYPRE_Real, p.cheby_fraction = v)
AMG_SET(ChebyEigEst, HYPRE_Int, p.cheby_eig_est = v)
AMG_SET(ChebyVariant, HYPRE_Int, p.cheby_variant = v)
AMG_SET(ChebyScale, HYPRE_Int, p.cheby_scale = v)
AMG_SET(FSAIMaxStepSize, HYPRE_Int, p.fsai_max_step_size = v; if (p.fsai_algo_type != 4) warn_ignored("fsai_max_step_size", v))
AMG_SET(FSAIMaxNnzRow, HYPRE_Int, warn_ignored("fsai_max_nnz_row", v))
AMG_SET(FSAIKapTolerance, HYPRE_Real, p.fsai_kap_tolerance = v; if (p.fsai_algo_type != 4) warn_ignored("fsai_kap_tolerance", v))
#undef AMG_SET
HYPRE_Int HYPRE_BoomerAMGSetLevelNonGalerkinTol(HYPRE_Solver solver, HYPRE_Real tol, HYPRE_Int level) {
  API_BEGIN
  AmgParams &p = AMG(solver)->amg.p;
  if (tol < 0.0 || tol > 1.0) fail(HYPRE_ERROR_ARG, "non_galerkin_level_tols: a tolerance must be in [0, 1]");
  if (level < 0 || level > 1000) fail(HYPRE_ERROR_ARG, "non_galerkin_level_tols: bad level");
  if ((int)p.non_galerkin_level_tol.size() <= level) p.non_galerkin_level_tol.resize((size_t)level + 1, -1.0);
  p.non_galerkin_level_tol[(size_t)level] = tol;
  note_non_galerkin_rule(tol);
  API_END
}
HYPRE_Int HYPRE_BoomerAMGSetCycleRelaxType(HYPRE_Solver solver, HYPRE_Int relax_type, HYPRE_Int k) {
  API_BEGIN
  if (k < 1 || k > 3) fail(HYPRE_ERROR_ARG, "SetCycleRelaxType: k must be 1, 2 or 3");
  AMG(solver)->amg.p.relax_type[k - 1] = relax_type;
  API_END
}
HYPRE_Int HYPRE_BoomerAMGSetCycleNumSweeps(HYPRE_Solver solver, HYPRE_Int num_sweeps, HYPRE_Int k) {
  API_BEGIN
  if (k < 1 || k > 3) fail(HYPRE_ERROR_ARG, "SetCycleNumSweeps: k must be 1, 2 or 3");
  if (num_sweeps < 0) fail(HYPRE_ERROR_ARG, "SetCycleNumSweeps: negative sweeps");
  AMG(solver)->amg.p.num_sweeps[k - 1] = num_sweeps;
  API_END
}
HYPRE_Int HYPRE_BoomerAMGGetNumIterations(HYPRE_Solver solver, HYPRE_Int *n) {
  API_BEGIN
  *n = AMG(solver)->amg.num_iterations;
  API_END
}
HYPRE_Int HYPRE_BoomerAMGGetFinalRelativeResidualNorm(HYPRE_Solver solver, HYPRE_Real *r) {
  API_BEGIN
  *r = AMG(solver)->amg.final_rel_res;
  API_END
}

// ------------------------------------------------------------------ GMRES / BiCGSTAB
HYPRE_Int HYPRE_ParCSRGMRESCreate(MPI_Comm, HYPRE_Solver *solver) {
  API_BEGIN
  if (!solver) fail(HYPRE_ERROR_ARG, "GMRESCreate: NULL output");
  *solver = reinterpret_cast<HYPRE_Solver>(static_cast<SolverBase *>(new GmresSolver()));
  API_END
}
HYPRE_Int HYPRE_ParCSRGMRESDestroy(HYPRE_Solver solver) {
  API_BEGIN
  delete S(solver);
  API_END
}
HYPRE_Int HYPRE_ParCSRGMRESSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) {
  API_BEGIN
  if (!A || !b || !x) fail(HYPRE_ERROR_ARG, "GMRESSetup: NULL argument");
  GM(solver)->setup(*PM(A), *PV(b), *PV(x));
  transport_gate(nullptr, "GMRESSetup");
  API_END
}
HYPRE_Int HYPRE_ParCSRGMRESSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) {
  try {
    if (!A || !b || !x) fail(HYPRE_ERROR_ARG, "GMRESSolve: NULL argument");
    const int rc = GM(solver)->solve(*PM(A), *PV(b), *PV(x));
    transport_gate(PV(x), "GMRESSolve");
    if (rc) g_error_flag |= rc;  // HYPRE_ERROR_CONV: reported, never fatal
    return rc;
  } catch (const std::exception &e) {
    return record_error(HYPRE_ERROR_GENERIC, e.what());
  }
}
#define KRYLOV_COMMON(NAME, GET)                                                                                  \
  HYPRE_Int HYPRE_ParCSR##NAME##SetPrecond(HYPRE_Solver solver, HYPRE_PtrToParSolverFcn precond,                  \
                                           HYPRE_PtrToParSolverFcn precond_setup, HYPRE_Solver precond_solver) {  \
    API_BEGIN                                                                                                     \
    KrylovSolver *k_ = GET(solver);                                                                               \
    k_->precond_solve = reinterpret_cast<ParSolverFcn>(precond);                                                  \
    k_->precond_setup = reinterpret_cast<ParSolverFcn>(precond_setup);                                            \
    k_->precond_data = precond_solver;                                                                            \
    API_END                                                                                                       \
  }                                                                                                               \
  HYPRE_Int HYPRE_ParCSR##NAME##SetTol(HYPRE_Solver solver, HYPRE_Real v) {                                       \
    API_BEGIN GET(solver)->tol = v;                                                                               \
    API_END                                                                                                       \
  }                                                                                                               \
  HYPRE_Int HYPRE_ParCSR##NAME##SetAbsoluteTol(HYPRE_Solver solver, HYPRE_Real v) {                               \
    API_BEGIN GET(solver)->atol = v;                                                                              \
    API_END                                                                                                       \
  }                                                                                                               \
  HYPRE_Int HYPRE_ParCSR##NAME##SetMaxIter(HYPRE_Solver solver, HYPRE_Int v) {                                    \
    API_BEGIN GET(solver)->max_iter = v;                                                                          \
    API_END                                                                                                       \
  }                                                                                                               \
  HYPRE_Int HYPRE_ParCSR##NAME##SetMinIter(HYPRE_Solver solver, HYPRE_Int v) {                                    \
    API_BEGIN GET(solver)->min_iter = v;                                                                          \
    API_END                                                                                                       \
  }                                                                                                               \
  HYPRE_Int HYPRE_ParCSR##NAME##SetKDim(HYPRE_Solver solver, HYPRE_Int v) {                                       \
    API_BEGIN if (v < 1) fail(HYPRE_ERROR_ARG, "k_dim < 1");                                                      \
    GET(solver)->k_dim = v;                                                                                       \
    API_END                                                                                                       \
  }                                                                                                               \
  HYPRE_Int HYPRE_ParCSR##NAME##SetPrintLevel(HYPRE_Solver solver, HYPRE_Int v) {                                 \
    API_BEGIN GET(solver)->print_level = v;                                                                       \
    API_END                                                                                                       \
  }                                                                                                               \
  HYPRE_Int HYPRE_ParCSR##NAME##SetLogging(HYPRE_Solver solver, HYPRE_Int v) {                                    \
    API_BEGIN GET(solver)->logging = v;                                                                           \
    API_END                                                                                                       \
  }                                                                                                               \
  HYPRE_Int HYPRE_ParCSR##NAME##GetNumIterations(HYPRE_Solver solver, HYPRE_Int *n) {                             \
    API_BEGIN *n = GET(solver)->num_iterations;                                                                   \
    API_END                                                                                                       \
  }                                                                                                               \
  HYPRE_Int HYPRE_ParCSR##NAME##GetFinalRelativeResidualNorm(HYPRE_Solver solver, HYPRE_Real *r) {                \
    API_BEGIN *r = GET(solver)->rel_residual_norm;                                                                \
    API_END                                                                                                       \
  }
KRYLOV_COMMON(GMRES, GM)
KRYLOV_COMMON(BiCGSTAB, BI)
KRYLOV_COMMON(FlexGMRES, GM)
KRYLOV_COMMON(PCG, PC)
KRYLOV_COMMON(COGMRES, GM)
#undef KRYLOV_COMMON
HYPRE_Int HYPRE_ParCSRGMRESSetCGS(HYPRE_Solver solver, HYPRE_Int) {
  API_BEGIN(void) GM(solver);
  API_END
}

#define KRYLOV_LIFECYCLE(NAME, TYPE, GET, INIT)                                                                   \
  HYPRE_Int HYPRE_ParCSR##NAME##Create(MPI_Comm, HYPRE_Solver *solver) {                                        \
    API_BEGIN                                                                                                   \
    if (!solver) fail(HYPRE_ERROR_ARG, #NAME "Create: NULL output");                                             \
    TYPE *obj = new TYPE();                                                                                     \
    INIT;                                                                                                       \
    *solver = reinterpret_cast<HYPRE_Solver>(static_cast<SolverBase *>(obj));                                   \
    API_END                                                                                                     \
  }                                                                                                             \
  HYPRE_Int HYPRE_ParCSR##NAME##Destroy(HYPRE_Solver solver) {                                                  \
    API_BEGIN delete S(solver);                                                                                 \
    API_END                                                                                                     \
  }                                                                                                             \
  HYPRE_Int HYPRE_ParCSR##NAME##Setup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b,             \
                                      HYPRE_ParVector x) {                                                      \
    API_BEGIN                                                                                                   \
    if (!A || !b || !x) fail(HYPRE_ERROR_ARG, #NAME "Setup: NULL argument");                                     \
    GET(solver)->setup(*PM(A), *PV(b), *PV(x));                                                                 \
    transport_gate(nullptr, #NAME "Setup");                                                                      \
    API_END                                                                                                     \
  }                                                                                                             \
  HYPRE_Int HYPRE_ParCSR##NAME##Solve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b,             \
                                      HYPRE_ParVector x) {                                                      \
    try {                                                                                                       \
      if (!A || !b || !x) fail(HYPRE_ERROR_ARG, #NAME "Solve: NULL argument");                                   \
      const int rc = GET(solver)->solve(*PM(A), *PV(b), *PV(x));                                                \
      transport_gate(PV(x), #NAME "Solve");                                                                      \
      if (rc) g_error_flag |= rc;                                                                               \
      return rc;                                                                                                \
    } catch (const std::exception &e) {                                                                         \
      return record_error(HYPRE_ERROR_GENERIC, e.what());                                                       \
    }                                                                                                           \
  }
KRYLOV_LIFECYCLE(FlexGMRES, GmresSolver, GM, obj->flexible = true)
KRYLOV_LIFECYCLE(PCG, PcgSolver, PC, (void)obj)
KRYLOV_LIFECYCLE(COGMRES, GmresSolver, GM, obj->ortho = 1)
#undef KRYLOV_LIFECYCLE
// cgs <= 1: one classical Gram-Schmidt pass per Arnoldi step, cgs >= 2: two
HYPRE_Int HYPRE_ParCSRCOGMRESSetCGS(HYPRE_Solver solver, HYPRE_Int cgs) {
  API_BEGIN GM(solver)->ortho = (cgs >= 2) ? 2 : 1;
  API_END
}
HYPRE_Int HYPRE_ParCSRPCGSetTwoNorm(HYPRE_Solver solver, HYPRE_Int two_norm) {
  API_BEGIN PC(solver)->two_norm = two_norm;
  API_END
}

HYPRE_Int HYPRE_ParCSRBiCGSTABCreate(MPI_Comm, HYPRE_Solver *solver) {
  API_BEGIN
  if (!solver) fail(HYPRE_ERROR_ARG, "BiCGSTABCreate: NULL output");
  *solver = reinterpret_cast<HYPRE_Solver>(static_cast<SolverBase *>(new BicgstabSolver()));
  API_END
}
HYPRE_Int HYPRE_ParCSRBiCGSTABDestroy(HYPRE_Solver solver) {
  API_BEGIN
  delete S(solver);
  API_END
}
HYPRE_Int HYPRE_ParCSRBiCGSTABSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) {
  API_BEGIN
  if (!A || !b || !x) fail(HYPRE_ERROR_ARG, "BiCGSTABSetup: NULL argument");
  BI(solver)->setup(*PM(A), *PV(b), *PV(x));
  transport_gate(nullptr, "BiCGSTABSetup");
  API_END
}
HYPRE_Int HYPRE_ParCSRBiCGSTABSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) {
  try {
    if (!A || !b || !x) fail(HYPRE_ERROR_ARG, "BiCGSTABSolve: NULL argument");
    const int rc = BI(solver)->solve(*PM(A), *PV(b), *PV(x));
    transport_gate(PV(x), "BiCGSTABSolve");
    if (rc) g_error_flag |= rc;
    return rc;
  } catch (const std::exception &e) {
    return record_error(HYPRE_ERROR_GENERIC, e.what());
  }
}

// ------------------------------------------------------------------ stubs
static IluSolver *ILU(HYPRE_Solver s) {
  SolverBase *b = S(s);
  if (b->kind != SolverBase::K_ILU) fail(HYPRE_ERROR_ARG, "handle is not an ILU solver");
  return static_cast<IluSolver *>(b);
}
HYPRE_Int HYPRE_ILUCreate(HYPRE_Solver *solver) {
  API_BEGIN
  if (!solver) fail(HYPRE_ERROR_ARG, "ILUCreate: NULL output");
  *solver = reinterpret_cast<HYPRE_Solver>(static_cast<SolverBase *>(new IluSolver()));
  API_END
}
HYPRE_Int HYPRE_ILUDestroy(HYPRE_Solver solver) {
  API_BEGIN delete S(solver);
  API_END
}
HYPRE_Int HYPRE_ILUSetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector, HYPRE_ParVector) {
  API_BEGIN
  if (!A) fail(HYPRE_ERROR_ARG, "ILUSetup: NULL matrix");
  ILU(solver)->setup(*PM(A), current_comm());
  transport_gate(nullptr, "ILUSetup");
  API_END
}
HYPRE_Int HYPRE_ILUSolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) {
  API_BEGIN
  if (!A || !b || !x) fail(HYPRE_ERROR_ARG, "ILUSolve: NULL argument");
  ILU(solver)->solve(*PM(A), *PV(b), *PV(x));
  transport_gate(PV(x), "ILUSolve");
  API_END
}
HYPRE_Int HYPRE_ILUGetNumIterations(HYPRE_Solver solver, HYPRE_Int *n) {
  API_BEGIN *n = ILU(solver)->num_iterations;
  API_END
}
HYPRE_Int HYPRE_ILUGetFinalRelativeResidualNorm(HYPRE_Solver solver, HYPRE_Real *r) {
  API_BEGIN *r = ILU(solver)->final_rel_res;
  API_END
}
#define ILU_SET(NAME, TYPE, STMT)                           \
  HYPRE_Int HYPRE_ILUSet##NAME(HYPRE_Solver solver, TYPE v) { \
    API_BEGIN IluSolver *o = ILU(solver);                   \
    (void)o;                                                \
    STMT;                                                   \
    API_END                                                 \
  }
ILU_SET(Type, HYPRE_Int, o->ilu_type = v)
ILU_SET(MaxIter, HYPRE_Int, o->max_iter = v)
ILU_SET(Tol, HYPRE_Real, o->tol = v)
ILU_SET(LocalReordering, HYPRE_Int, o->reordering = v)  /* 2 = multicolour ordering; every other value: none */
ILU_SET(PrintLevel, HYPRE_Int, o->print_level = v)
ILU_SET(LevelOfFill, HYPRE_Int, o->level_of_fill = v)
ILU_SET(MaxNnzPerRow, HYPRE_Int, (void)v)        /* ILUT only */
ILU_SET(DropThreshold, HYPRE_Real, (void)v)      /* ILUT only */
ILU_SET(IterativeSetupType, HYPRE_Int, o->iter_type = v)  /* 0 ... 4 with ILU(0); other combinations are refused at Setup */
ILU_SET(IterativeSetupOption, HYPRE_Int, o->iter_option = v)
ILU_SET(IterativeSetupMaxIter, HYPRE_Int, o->iter_max_iter = v)
ILU_SET(IterativeSetupTolerance, HYPRE_Real, o->iter_tol = v)
ILU_SET(LowerJacobiIters, HYPRE_Int, o->lower_it = v)
ILU_SET(UpperJacobiIters, HYPRE_Int, o->upper_it = v)
#undef ILU_SET
// the driver also calls this one on a BoomerAMG handle (src/HypreSystem.cpp:306): accepted and ignored there
HYPRE_Int HYPRE_ILUSetTriSolve(HYPRE_Solver solver, HYPRE_Int v) {
  API_BEGIN
  if (S(solver)->kind == SolverBase::K_ILU) ILU(solver)->tri_solve = v ? 1 : 0;
  API_END
}
HYPRE_Int HYPRE_MI_ILUGetIterativeSetupInfo(HYPRE_Solver solver, HYPRE_Int *sweeps, HYPRE_Real *correction,
                                            HYPRE_Real *residual) {
  API_BEGIN
  IluSolver *o = ILU(solver);
  if (sweeps) *sweeps = o->iter_sweeps;
  if (correction) *correction = o->iter_correction;
  if (residual) *residual = o->iter_residual;
  API_END
}
HYPRE_Int HYPRE_MI_ILUGetIterativeSetupHistory(HYPRE_Solver solver, HYPRE_Int *ncorr, HYPRE_Real *corr, HYPRE_Int *nres,
                                               HYPRE_Real *res) {
  API_BEGIN
  IluSolver *o = ILU(solver);
  if (ncorr) *ncorr = (HYPRE_Int)o->iter_corr_hist.size();
  if (nres) *nres = (HYPRE_Int)o->iter_res_hist.size();
  if (corr && !o->iter_corr_hist.empty()) memcpy(corr, o->iter_corr_hist.data(), o->iter_corr_hist.size() * sizeof(double));
  if (res && !o->iter_res_hist.empty()) memcpy(res, o->iter_res_hist.data(), o->iter_res_hist.size() * sizeof(double));
  API_END
}
HYPRE_Int HYPRE_MI_ILUGetFactorsSize(HYPRE_Solver solver, HYPRE_Int *nrows, HYPRE_BigInt *nnz) {
  API_BEGIN
  IluSolver *o = ILU(solver);
  if (!o->is_setup) fail(HYPRE_ERROR_GENERIC, "ILUGetFactors: the ILU is not set up");
  *nrows = o->LU.nrows;
  *nnz = (HYPRE_BigInt)o->LU.nnz;
  API_END
}
HYPRE_Int HYPRE_MI_ILUGetFactors(HYPRE_Solver solver, HYPRE_BigInt *ia, HYPRE_Int *ja, HYPRE_Complex *a) {
  API_BEGIN
  IluSolver *o = ILU(solver);
  if (!o->is_setup) fail(HYPRE_ERROR_GENERIC, "ILUGetFactors: the ILU is not set up");
  HostCSR h;
  o->LU.download(h, ctx().stream);
  if (ia)
    for (int i = 0; i <= h.nrows; i++) ia[i] = h.ia.empty() ? 0 : h.ia[(size_t)i];
  if (ja && !h.ja.empty()) memcpy(ja, h.ja.data(), h.ja.size() * sizeof(int));
  if (a && !h.a.empty()) memcpy(a, h.a.data(), h.a.size() * sizeof(double));
  API_END
}
// info[5]: the reordering in force (0 or 2), colours, colouring rounds, lower and upper level sets; perm / colour: n
// entries each, left untouched without the ordering
static void ilu_ordering_out(IluSolver *o, HYPRE_Int *info, HYPRE_Int *perm, HYPRE_Int *colour) {
  if (!o->is_setup) fail(HYPRE_ERROR_GENERIC, "ILUGetOrdering: the ILU is not set up");
  if (info)
    for (int q = 0; q < 5; q++) info[q] = o->ordering_info[q];
  if (o->ordering_info[0] != 2 || o->n == 0) return;
  if (perm) memcpy(perm, o->perm_h.data(), (size_t)o->n * sizeof(int));
  if (colour) o->colour.download(colour, (size_t)o->n);
}
HYPRE_Int HYPRE_MI_ILUGetOrdering(HYPRE_Solver solver, HYPRE_Int info[5], HYPRE_Int *perm, HYPRE_Int *colour) {
  API_BEGIN
  ilu_ordering_out(ILU(solver), info, perm, colour);
  API_END
}

// ------------------------------------------------------------------ FSAI (fsai.cpp)
static FsaiSolver *FSAI(HYPRE_Solver s) {
  SolverBase *b = S(s);
  if (b->kind != SolverBase::K_FSAI) fail(HYPRE_ERROR_ARG, "handle is not an FSAI solver");
  return static_cast<FsaiSolver *>(b);
}
HYPRE_Int HYPRE_FSAICreate(HYPRE_Solver *solver) {
  API_BEGIN
  if (!solver) fail(HYPRE_ERROR_ARG, "FSAICreate: NULL output");
  *solver = reinterpret_cast<HYPRE_Solver>(static_cast<SolverBase *>(new FsaiSolver()));
  API_END
}
HYPRE_Int HYPRE_FSAIDestroy(HYPRE_Solver solver) {
  API_BEGIN
  FSAI(solver);
  delete S(solver);
  API_END
}
HYPRE_Int HYPRE_FSAISetup(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector, HYPRE_ParVector) {
  API_BEGIN
  if (!A) fail(HYPRE_ERROR_ARG, "FSAISetup: NULL matrix");
  FSAI(solver)->setup(*PM(A), current_comm(), "HYPRE_FSAISetup");
  transport_gate(nullptr, "FSAISetup");
  API_END
}
HYPRE_Int HYPRE_FSAISolve(HYPRE_Solver solver, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) {
  API_BEGIN
  if (!A || !b || !x) fail(HYPRE_ERROR_ARG, "FSAISolve: NULL argument");
  FSAI(solver)->solve(*PM(A), *PV(b), *PV(x));
  transport_gate(PV(x), "FSAISolve");
  API_END
}
#define FSAI_SET(NAME, TYPE, STMT)                            \
  HYPRE_Int HYPRE_FSAISet##NAME(HYPRE_Solver solver, TYPE v) { \
    API_BEGIN FsaiSolver *o = FSAI(solver);                   \
    (void)o;                                                  \
    STMT;                                                     \
    API_END                                                   \
  }
FSAI_SET(AlgoType, HYPRE_Int, o->algo_type = v)  /* 3 (static pattern) and 4 (adaptive pattern) are built: others are refused at Setup */
FSAI_SET(LocalSolveType, HYPRE_Int, (void)v)
FSAI_SET(NumLevels, HYPRE_Int, o->num_levels = v)
FSAI_SET(Threshold, HYPRE_Real, if (v < 0.0) fail(HYPRE_ERROR_ARG, "FSAI threshold < 0"); o->threshold = v)
FSAI_SET(EigMaxIters, HYPRE_Int, if (v < 0) fail(HYPRE_ERROR_ARG, "FSAI eig_max_iters < 0"); o->eig_max_iters = v)
FSAI_SET(Omega, HYPRE_Real, o->omega_user = v)
FSAI_SET(MaxIterations, HYPRE_Int, if (v < 0) fail(HYPRE_ERROR_ARG, "FSAI max_iterations < 0"); o->max_iter = v)
FSAI_SET(Tolerance, HYPRE_Real, o->tol = v)
FSAI_SET(ZeroGuess, HYPRE_Int, o->zero_guess = v != 0)
FSAI_SET(PrintLevel, HYPRE_Int, o->print_level = v)
FSAI_SET(MaxSteps, HYPRE_Int, o->max_steps = v; if (o->algo_type != 4) warn_ignored("fsai_max_steps", v))
FSAI_SET(MaxStepSize, HYPRE_Int, o->max_step_size = v; if (o->algo_type != 4) warn_ignored("fsai_max_step_size", v))
FSAI_SET(MaxNnzRow, HYPRE_Int, warn_ignored("fsai_max_nnz_row", v))
FSAI_SET(KapTolerance, HYPRE_Real, o->kap_tolerance = v; if (o->algo_type != 4) warn_ignored("fsai_kap_tolerance", v))
#undef FSAI_SET
HYPRE_Int HYPRE_MI_FSAIGetSetupInfo(HYPRE_Solver solver, HYPRE_Int out[8]) {
  API_BEGIN
  FsaiSolver *o = FSAI(solver);
  if (!out) fail(HYPRE_ERROR_ARG, "FSAIGetSetupInfo: no buffer");
  if (!o->is_setup) fail(HYPRE_ERROR_GENERIC, "FSAIGetSetupInfo: the solver is not set up");
  for (int q = 0; q < 8; q++) out[q] = o->setup_info[q];
  API_END
}

// ------------------------------------------------------------------ AMG internals used by the driver's level dump
static thread_local std::vector<hypre_ParCSRMatrix *> g_level_ptrs;
hypre_ParCSRMatrix **hypre_ParAMGDataAArray(hypre_ParAMGData *amg_data) {
  try {
    AmgSolver *a = AMG(reinterpret_cast<HYPRE_Solver>(amg_data));
    g_level_ptrs.clear();
    for (int l = 0; l < a->amg.total_levels(); l++) {
      int loc = 0;
      BoomerAMG &o = a->amg.owner_of(l, loc);
      o.ensure_host(loc);
      g_level_ptrs.push_back(reinterpret_cast<hypre_ParCSRMatrix *>(o.L[(size_t)loc].A));
    }
    return g_level_ptrs.data();
  } catch (const std::exception &e) {
    record_error(HYPRE_ERROR_ARG, e.what());
    return nullptr;
  }
}
HYPRE_Int hypre_ParAMGDataNumLevels(hypre_ParAMGData *amg_data) {
  try {
    return (HYPRE_Int)AMG(reinterpret_cast<HYPRE_Solver>(amg_data))->amg.total_levels();
  } catch (const std::exception &e) {
    record_error(HYPRE_ERROR_ARG, e.what());
    return 0;
  }
}

// ------------------------------------------------------------------ extensions
HYPRE_Int HYPRE_MI_CommGetUniqueId(void *id128) {
  API_BEGIN
  ensure_init();
  rccl_get_unique_id(id128);
  API_END
}
HYPRE_Int HYPRE_MI_CommInitRCCL(const void *id128, HYPRE_Int rank, HYPRE_Int size) {
  API_BEGIN
  ensure_init();
  if (size < 1 || rank < 0 || rank >= size) fail(HYPRE_ERROR_ARG, "CommInitRCCL: bad rank/size");
  if (size == 1)
    ctx().comm = make_self_comm();
  else
    ctx().comm = make_rccl_comm(id128, rank, size);
  API_END
}
HYPRE_Int HYPRE_MI_CommInitFromEnv(void) {
  API_BEGIN
  // (the TCP mesh is a host transport: it can be bound without a device, e.g. for the host-only setup entry points)
  const char *tr = getenv("MI_HYPRE_TRANSPORT");
  if (!(tr && std::string(tr) == "tcp")) ensure_init();
  ctx().comm = make_comm_from_env();
  API_END
}
HYPRE_Int HYPRE_MI_CommSelfTestRCCL(void) {
  // a world of one rank through the real RCCL entry points: dlopen + symbols,
  // CommInitRank, AllReduce, AllGather and a grouped Send/Recv to self
  API_BEGIN
  ensure_init();
  unsigned char id[128];
  rccl_get_unique_id(id);
  std::unique_ptr<Comm> rc = make_rccl_comm(id, 0, 1);
  hipStream_t s = ctx().stream;
  std::vector<double> h = {1.5, -2.0, 3.25, 4.0};
  DVec<double> a, b(4), g(4);
  a.upload(h);
  rc->allreduce_dev(a.p, 4, CommDType::F64, CommOp::SUM, s);
  rc->allgather_dev(a.p, g.p, 4 * sizeof(double), s);
  rc->exchange_dev({{0, a.p, 4 * sizeof(double)}}, {{0, b.p, 4 * sizeof(double)}}, s);
  MI_HIP(hipStreamSynchronize(s));
  std::vector<double> ha = a.to_host(), hb = b.to_host(), hg = g.to_host();
  for (int i = 0; i < 4; i++)
    if (ha[(size_t)i] != h[(size_t)i] || hb[(size_t)i] != h[(size_t)i] || hg[(size_t)i] != h[(size_t)i])
      fail(HYPRE_ERROR_GENERIC, "RCCL self test: wrong data");
  long long v = 7;
  rc->allreduce_host(&v, 1, CommDType::I64, CommOp::MAX);
  if (v != 7) fail(HYPRE_ERROR_GENERIC, "RCCL self test: host all-reduce");
  API_END
}
HYPRE_Int HYPRE_MI_CommInitCallbacks(void *cctx, HYPRE_MI_AllreduceFn ar, HYPRE_MI_AllgatherFn ag,
                                     HYPRE_MI_ExchangeFn ex, HYPRE_Int rank, HYPRE_Int size) {
  API_BEGIN
  if (!ar || !ag || !ex) fail(HYPRE_ERROR_ARG, "CommInitCallbacks: NULL callback");
  CommCallbacks cb{cctx, ar, ag, ex};
  ctx().comm = make_callback_comm(cb, rank, size);
  API_END
}
HYPRE_Int HYPRE_MI_CommEnablePeerStoreExchange(HYPRE_BigInt slot_bytes) {
  API_BEGIN
  ensure_init();
  if (!ctx().comm || ctx().comm->size == 1) return 0;
  if (slot_bytes <= 0) slot_bytes = getenv("MI_HYPRE_IPC_SLOT_BYTES") ? atoll(getenv("MI_HYPRE_IPC_SLOT_BYTES")) : (4 << 20);
  if (slot_bytes % 16) fail(HYPRE_ERROR_ARG, "CommEnablePeerStoreExchange: the slot size must be a multiple of 16 bytes");
  MI_HIP(hipDeviceSynchronize());
  // (a refusal throws before the communicator changes hands: ctx().comm keeps its transport and the call returns an error)
  std::unique_ptr<Comm> wrapped = make_ipc_exchange_comm(ctx().comm, (size_t)slot_bytes);
  ctx().comm = std::move(wrapped);
  API_END
}
HYPRE_Int HYPRE_MI_CommExchangeDevice(HYPRE_Int nsend, const HYPRE_Int *send_peers, void *const *send_ptrs,
                                      const size_t *send_bytes, HYPRE_Int nrecv, const HYPRE_Int *recv_peers,
                                      void *const *recv_ptrs, const size_t *recv_bytes) {
  API_BEGIN
  ensure_init();
  std::vector<PeerBuf> sb, rb;
  for (int i = 0; i < nsend; i++) sb.push_back({send_peers[i], send_ptrs[i], send_bytes[i]});
  for (int i = 0; i < nrecv; i++) rb.push_back({recv_peers[i], recv_ptrs[i], recv_bytes[i]});
  hipStream_t s = ctx().stream;
  current_comm().exchange_dev(sb, rb, s);
  MI_HIP(hipStreamSynchronize(s));
  comm_check_transport_error(current_comm(), s);
  API_END
}
HYPRE_Int HYPRE_MI_CommAllreduceDevice(HYPRE_Real *dev_buf, HYPRE_Int count) {
  API_BEGIN
  ensure_init();
  if (!dev_buf || count < 1) fail(HYPRE_ERROR_ARG, "CommAllreduceDevice: bad argument");
  hipStream_t s = ctx().stream;
  current_comm().allreduce_dev(dev_buf, (size_t)count, CommDType::F64, CommOp::SUM, s);
  MI_HIP(hipStreamSynchronize(s));
  comm_check_transport_error(current_comm(), s);
  API_END
}
HYPRE_Int HYPRE_MI_CommCheck(void) {
  API_BEGIN
  if (ctx().inited && ctx().comm) comm_check_transport_error(*ctx().comm, ctx().stream);
  API_END
}
HYPRE_Int HYPRE_MI_CommName(char *name, HYPRE_Int max_len) {
  API_BEGIN
  if (!name || max_len < 1) fail(HYPRE_ERROR_ARG, "CommName: no buffer");
  snprintf(name, (size_t)max_len, "%s", current_comm().name());
  API_END
}
HYPRE_Int HYPRE_MI_CommFinalize(void) {
  API_BEGIN
  if (ctx().inited) MI_HIP(hipDeviceSynchronize());
  ctx().comm = make_self_comm();
  API_END
}
HYPRE_Int HYPRE_MI_CommRank(HYPRE_Int *rank) {
  *rank = current_comm().rank;
  return 0;
}
HYPRE_Int HYPRE_MI_CommSize(HYPRE_Int *size) {
  *size = current_comm().size;
  return 0;
}
HYPRE_Int HYPRE_MI_CommBarrier(void) {
  API_BEGIN
  current_comm().barrier();
  API_END
}
HYPRE_Int HYPRE_MI_CommAllreduce(void *buf, size_t count, int dtype, int op) {
  API_BEGIN
  if (dtype < 0 || dtype > 3 || op < 0 || op > 2) fail(HYPRE_ERROR_ARG, "CommAllreduce: bad dtype/op");
  current_comm().allreduce_host(buf, count, (CommDType)dtype, (CommOp)op);
  API_END
}
HYPRE_Int HYPRE_MI_GetStream(void **hip_stream) {
  API_BEGIN
  ensure_init();
  *hip_stream = (void *)ctx().stream;
  API_END
}
HYPRE_Int HYPRE_MI_StreamSynchronize(void) {
  API_BEGIN
  ensure_init();
  MI_HIP(hipStreamSynchronize(ctx().stream));
  API_END
}
HYPRE_Int HYPRE_MI_SetGSChunk(HYPRE_Int rows) {
  API_BEGIN
  if (rows < 1 || rows > k::GS_MAX_CHUNK) fail(HYPRE_ERROR_ARG, "SetGSChunk: 1..32");
  ctx().gs_chunk = rows;
  API_END
}
// the size check HYPRE_IJMatrixAssemble and the solve format apply to one rank's diagonal block, on a caller-supplied
// row-pointer array (tests exercise the boundaries without building a 2^31-entry matrix): 32-bit local row ids,
// 64-bit entry offsets, but no single row of 2^31 entries or more
HYPRE_Int HYPRE_MI_CheckBlockRowPointers(HYPRE_BigInt nrows, const HYPRE_BigInt *row_ptr) {
  API_BEGIN
  if (nrows < 0 || (nrows > 0 && !row_ptr)) fail(HYPRE_ERROR_ARG, "CheckBlockRowPointers: bad argument");
  require_int32_block(nrows, 0, "IJMatrixAssemble");
  for (HYPRE_BigInt i = 0; i < nrows; i++) require_int32_block(0, row_ptr[i + 1] - row_ptr[i], "IJMatrixAssemble (one row)");
  API_END
}
HYPRE_Int HYPRE_MI_GetCounter(const char *name, long long *value) {
  API_BEGIN
  const std::string n(name ? name : "");
  if (n == "pool_cached_bytes" || n == "pool_hits" || n == "pool_misses") {
    long long cb = 0, h = 0, m = 0;
    dev_pool_stats(&cb, &h, &m);
    *value = n == "pool_cached_bytes" ? cb : n == "pool_hits" ? h : m;
    return 0;
  }
  if (n.rfind("arena_", 0) == 0) {
    long long mp = 0, iu = 0, pm = 0, pu = 0;
    dev_arena_stats(&mp, &iu, &pm, &pu);
    if (n == "arena_mapped_bytes") *value = mp;
    else if (n == "arena_in_use_bytes") *value = iu;
    else if (n == "arena_peak_mapped_bytes") *value = pm;
    else if (n == "arena_peak_in_use_bytes") *value = pu;
    else fail(HYPRE_ERROR_ARG, "GetCounter: unknown counter " + n);
    return 0;
  }
  if (n == "ij_device_assemblies")
    *value = ij::counters().device_assemblies;
  else if (n == "ij_value_updates")
    *value = ij::counters().value_updates;
  else if (n == "ij_device_value_updates")
    *value = ij::counters().device_value_updates;
  else if (n == "ij_update_kernels_us" || n == "ij_update_dictionary_us" || n == "ij_update_mirror_us")
    *value = (long long)(1e6 * (n == "ij_update_kernels_us" ? ij::counters().t_update_kernels
                                : n == "ij_update_dictionary_us" ? ij::counters().t_update_dict : ij::counters().t_update_mirror));
  else if (n == "ij_entries_fetched_to_host")
    *value = ij::counters().entries_fetched;
  else if (n == "ij_host_mirror_bytes")
    *value = ij::counters().host_mirror_bytes;
  else if (n == "ij_device_sort_lds_capacity")
    *value = ij::SORT_LDS_CAP;
  else if (n == "ij_last_kernels_us" || n == "ij_last_mirror_us" || n == "ij_last_format_us")
    *value = (long long)(1e6 * (n == "ij_last_kernels_us" ? ij::counters().t_kernels
                                : n == "ij_last_mirror_us" ? ij::counters().t_mirror : ij::counters().t_format));
  else if (n == "matvec_overlapped")
    *value = ctx().n_matvec_overlapped;
  else if (n == "gs_overlapped")
    *value = ctx().n_gs_overlapped;
  else if (n == "gs_in_order")
    *value = ctx().n_gs_in_order;
  else if (n == "allreduce")
    *value = ctx().n_allreduce;
  else if (n == "halo_exchange")
    *value = ctx().n_halo_exchange;
  else if (n == "allgather")
    *value = ctx().n_allgather;
  else if (n == "value_storage_row_mapped")
    *value = ctx().n_value_row_mapped;
  else if (n == "precond_cycles")
    *value = ctx().n_precond_cycles;
  else if (n == "gmres_direction_vectors")
    *value = ctx().n_gmres_z_allocated;
  else if (n == "krylov_basis_fp32_vectors")
    *value = ctx().n_krylov_basis_fp32;
  else if (n == "krylov_basis_bytes")
    *value = ctx().krylov_basis_bytes;
  else if (n == "handover_matvecs")
    *value = ctx().n_handover_matvecs;
  else if (n == "handover_tiles_skipped")
    *value = ctx().n_handover_tiles_skipped;
  else if (n == "mv_batched_cycles")
    *value = ctx().n_mv_batched_cycles;
  else if (n == "mv_batched_matvecs")
    *value = ctx().n_mv_batched_matvecs;
  else if (n == "mv_fallback_cycles")
    *value = ctx().n_mv_fallback_cycles;
  else if (setup_reuse_counter(n.c_str()) >= 0)
    *value = setup_reuse_counter(n.c_str());
  else if (dist_setup_counter(n.c_str()) >= 0)
    *value = dist_setup_counter(n.c_str());
  else
    fail(HYPRE_ERROR_ARG, "GetCounter: unknown counter " + n);
  API_END
}
HYPRE_Int HYPRE_MI_SetZeroGuessMode(HYPRE_Int mode) {
  API_BEGIN
  if (mode < 0 || mode > 3) fail(HYPRE_ERROR_ARG, "SetZeroGuessMode: 0..3");
  set_zero_skip_mode(mode);
  API_END
}
HYPRE_Int HYPRE_MI_SetCRowHandover(HYPRE_Int mode) {
  API_BEGIN
  if (mode < 0 || mode > 2) fail(HYPRE_ERROR_ARG, "SetCRowHandover: 0..2");
  set_c_handover_mode(mode);
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetCRowHandoverCensus(HYPRE_Solver solver, HYPRE_Int level, HYPRE_BigInt *census) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  if (!a->amg.is_setup) fail(HYPRE_ERROR_GENERIC, "GetCRowHandoverCensus: AMG is not set up");
  if (level < 0 || level >= (int)a->amg.L.size()) fail(HYPRE_ERROR_ARG, "AMG level out of range");
  const AmgLevel &Lv = a->amg.L[(size_t)level];
  const bool built = Lv.mv_tdesc.p != nullptr;
  census[0] = Lv.A->d_diag.nblocks;
  census[1] = built ? Lv.handover.listed : Lv.A->d_diag.nblocks;
  census[2] = built ? Lv.handover.handed : 0;
  census[3] = Lv.handover.flagged_c_rows;
  census[4] = built ? Lv.handover.w_upto : 0;
  API_END
}
// One cycle from a zero guess as a Krylov loop in level order asks for it, with the hand-over target set, then the
// mat-vec that follows it: z = M^-1 f, w = A z by the path the current mode takes (raised: the C pass handed rows over
// and the mat-vec ran on the tile list), w_full = A z by the full mat-vec.  Host arrays in level 0's ordering.
HYPRE_Int HYPRE_MI_BoomerAMGCycleThenMatvec(HYPRE_Solver solver, const HYPRE_Real *f_host, HYPRE_Real *z_host,
                                            HYPRE_Real *w_host, HYPRE_Real *w_full_host, HYPRE_Int *raised) {
  API_BEGIN
  BoomerAMG &amg = AMG(solver)->amg;
  if (!amg.is_setup || amg.L.empty()) fail(HYPRE_ERROR_GENERIC, "CycleThenMatvec: AMG is not set up");
  AmgLevel &L0 = amg.L[0];
  const int n = L0.n;
  hipStream_t s = ctx().stream;
  DVec<double> f((size_t)n), w((size_t)n), wf((size_t)n);
  f.upload(f_host, (size_t)n);
  MI_HIP(hipStreamSynchronize(s));
  k::fill(w.p, n, std::numeric_limits<double>::quiet_NaN(), s);  // a row nobody writes shows
  k::copy(f.p, L0.f.p, n, s);
  if (!amg.zero_cycle_ignores_u(0)) k::fill(L0.u.p, n, 0.0, s);
  amg.handover_w = amg.handover_wanted() ? w.p : nullptr;
  try {
    amg.cycle(0, true);
  } catch (...) {
    amg.handover_w = nullptr;
    throw;
  }
  amg.handover_w = nullptr;
  const bool handed = amg.handover_done;
  amg.handover_done = false;
  if (handed)
    L0.A->matvec_listed_tiles(L0.mv_tdesc.p, L0.handover.listed, L0.u.p, w.p, s);
  else
    L0.A->matvec(amg.my_comm(), 1.0, L0.u.p, 0.0, nullptr, w.p, s);
  L0.A->matvec(amg.my_comm(), 1.0, L0.u.p, 0.0, nullptr, wf.p, s);
  MI_HIP(hipStreamSynchronize(s));
  if (n) {
    d2h(z_host, L0.u.p, (size_t)n * sizeof(double), nullptr);
    d2h(w_host, w.p, (size_t)n * sizeof(double), nullptr);
    d2h(w_full_host, wf.p, (size_t)n * sizeof(double), nullptr);
  }
  *raised = handed ? 1 : 0;
  API_END
}
// test hook (tests/test_gpu_amg.py): every level's solution and scratch vectors of the hierarchy become NaN.  A cycle from
// a zero guess that skips its zero-fills (BoomerAMG::zero_cycle_ignores_u) must still give the bits it gives on clean
// vectors -- "never read" is checked, not assumed
HYPRE_Int HYPRE_MI_BoomerAMGPoisonWorkVectors(HYPRE_Solver solver) {
  API_BEGIN
  BoomerAMG &a = AMG(solver)->amg;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  hipStream_t s = ctx().stream;
  for (BoomerAMG *h = &a; h; h = h->tail.get())
    for (AmgLevel &Lv : h->L) {
      if (Lv.u.p && Lv.n) k::fill(Lv.u.p, Lv.n, nan, s);
      if (Lv.tmp.p && Lv.n) k::fill(Lv.tmp.p, Lv.n, nan, s);
      if (Lv.snap.p && Lv.n) k::fill(Lv.snap.p, Lv.n, nan, s);
    }
  MI_HIP(hipStreamSynchronize(s));
  API_END
}
// test hook (tests/test_gpu_kernels.py): a seeded storm of allocations and releases of every size class through
// dev_alloc / dev_free, every live block filled with its own byte pattern and checked before it is released -- two
// blocks that overlap, a block handed out twice or a trim that unmaps live memory show up as a wrong byte (or a fault).
// Returns the number of blocks that were verified; *peak_bytes = the most bytes live at once.
HYPRE_Int HYPRE_MI_TileScheduleCheck(HYPRE_Int n, const HYPRE_BigInt *row_ptr, HYPRE_Int row_cap, HYPRE_Int tile_entries,
                                     HYPRE_Int *ntiles, HYPRE_Int *mismatch) {
  API_BEGIN
  ensure_init();
  MI_REQUIRE(n >= 0 && row_ptr && mismatch, "TileScheduleCheck: arguments");
  MI_REQUIRE(tile_entries == k::SPMV_TILE || tile_entries == k::SPMV_TILE_WIDE, "TileScheduleCheck: tile_entries is 2048 or 4096");
  static_assert(sizeof(HYPRE_BigInt) == sizeof(long long), "row pointer width");
  bool aligned_h = true, aligned_d = true;
  const std::vector<int> host = k::build_row_blocks((int)n, reinterpret_cast<const int64_t *>(row_ptr), &aligned_h, (int)row_cap,
                                                    (int)tile_entries);
  DVec<long long> ia((size_t)n + 1);
  MI_HIP(hipMemcpy(ia.p, row_ptr, ((size_t)n + 1) * sizeof(long long), hipMemcpyHostToDevice));
  DVec<int> rb;
  std::vector<int> dev;
  sk::tile_schedule_device((int)n, ia.p, (int)row_cap, (int)tile_entries, rb, dev, aligned_d, ctx().stream);
  if (ntiles) *ntiles = (HYPRE_Int)host.size() - 1;
  *mismatch = 0;
  const size_t m = std::min(host.size(), dev.size());
  for (size_t t = 0; t < m && !*mismatch; t++)
    if (host[t] != dev[t]) *mismatch = (HYPRE_Int)t + 1;
  if (!*mismatch && host.size() != dev.size()) *mismatch = (HYPRE_Int)m + 1;
  if (!*mismatch && aligned_h != aligned_d) *mismatch = (HYPRE_Int)m + 2;
  API_END
}

// test hook (tests/test_gpu_krylov_paths.py): exactly one launch sequence of one of the Krylov loops' vector kernels, on
// this rank's part of the given ParVectors (all components of a multivector; no collective).  Device coefficients go
// into the context's scalar slots the way GmresSolver::solve leaves them there; scalar results come back in out.
//   op 0  k::mass_dot            out[j] = <vecs[j], w>, j < m                                   (1 <= m <= 120)
//   op 1  k::mass_axpy           w += sum_j (scale * coef[j]) vecs[j], coef in device slots     (1 <= m <= 120)
//   op 2  k::lin_comb            w = (init) / w += sum_j coef[j] vecs[j], coef passed by value  (1 <= m <= 250)
//   op 3  k::axpy_dot            w += (scale * coef[0]) vecs[0]; out[0] = <xd, w> (xd NULL: <w, w>)
//   op 4  k::scale_inv_sqrt_post w *= 1 / sqrt(coef[0]) when coef[0] > 0; the m slots coef[0 .. m) are posted into
//         pinned host memory, then the sequence number: out[0 .. m) = the posted doubles, out[m] = the flag word after
//         the kernel, out[m + 1] = the sequence number the kernel was given                    (1 <= m <= 255)
//   op 5  k::mgs_block_pass      one pass of the blocked MGS step with NB = k::MGS_NB: scale = m_prev, the first m_prev
//         vectors are the block subtracted, the other m - m_prev the block measured (none when init != 0, the last pass);
//         coef = NB raw inner products c, then NB raw Gram rows of NB + 1 doubles.  out[0 .. NB] = the pass's sums,
//         out[NB + 1 .. 2 NB] = the coefficients h (0 beyond m_prev), out[2 NB + 1] = the last pass's second copy of
//         ||w||^2 (else 0); w is updated                                                        (1 <= m <= 2 NB)
HYPRE_Int HYPRE_MI_VectorKernelOp(HYPRE_Int op, HYPRE_Int m, HYPRE_ParVector *vecs, const HYPRE_Real *coef,
                                  HYPRE_Real scale, HYPRE_ParVector w, HYPRE_ParVector xd, HYPRE_Int init,
                                  HYPRE_Real *out) {
  API_BEGIN
  ensure_init();
  Ctx &c = ctx();
  hipStream_t s = c.stream;
  MI_REQUIRE(w, "VectorKernelOp: NULL vector w");
  MI_REQUIRE(op >= 0 && op <= 5, "VectorKernelOp: op must be 0 .. 5");
  const int mmax = (op <= 1) ? 120 : (op == 2 ? 250 : (op == 3 ? 1 : (op == 4 ? 255 : 2 * k::MGS_NB)));
  MI_REQUIRE(m >= 1 && m <= mmax, "VectorKernelOp: m out of range for this op");
  MI_REQUIRE(op == 0 || coef, "VectorKernelOp: NULL coefficients");
  MI_REQUIRE(op == 1 || op == 2 || out, "VectorKernelOp: NULL output");
  const int n = PV(w)->len();
  std::vector<const double *> vp;
  if (op != 4) {
    MI_REQUIRE(vecs, "VectorKernelOp: NULL vector list");
    for (int j = 0; j < m; j++) {
      MI_REQUIRE(vecs[j] && PV(vecs[j])->len() == n, "VectorKernelOp: vecs[j] is NULL or differs from w in length");
      MI_REQUIRE(vecs[j] != w, "VectorKernelOp: w among vecs");
      vp.push_back(PV(vecs[j])->all());
    }
  }
  MI_REQUIRE(!xd || (op == 3 && PV(xd)->len() == n && xd != w), "VectorKernelOp: xd goes with op 3 and has w's length");
  double *slots = c.red_out.p;
  if (op == 1 || op == 3 || op == 4)
    MI_HIP(hipMemcpyAsync(slots, coef, (size_t)(op == 3 ? 1 : m) * sizeof(double), hipMemcpyHostToDevice, s));
  switch (op) {
    case 0:
      k::mass_dot(vp.data(), m, PV(w)->all(), n, slots, s);
      d2h(out, slots, (size_t)m * sizeof(double), s);
      break;
    case 1: k::mass_axpy(vp.data(), m, slots, scale, PV(w)->all(), n, s); break;
    case 2: k::lin_comb(vp.data(), coef, m, init != 0, PV(w)->all(), n, s); break;
    case 3:
      k::axpy_dot(slots, scale, vp[0], PV(w)->all(), xd ? PV(xd)->all() : nullptr, n, slots + 1, s);
      d2h(out, slots + 1, sizeof(double), s);
      break;
    case 5: {
      constexpr int NB = k::MGS_NB;
      const int m_prev = (int)scale, m_next = init ? 0 : m - m_prev;
      MI_REQUIRE(m_prev >= 0 && m_prev <= NB && m_prev <= m && m - m_prev <= NB && (!init || m_prev == m),
                 "VectorKernelOp: op 5 takes at most MGS_NB vectors per block, and none to measure in the last pass");
      DVec<double> buf((size_t)NB * (NB + 2) + 3 * (NB + 1));  // c, Gram rows | sums, h, ||w||^2
      double *sums = buf.p + NB * (NB + 2), *h = sums + NB + 1;
      MI_HIP(hipMemcpyAsync(buf.p, coef, (size_t)NB * (NB + 2) * sizeof(double), hipMemcpyHostToDevice, s));
      MI_HIP(hipMemsetAsync(sums, 0, (size_t)3 * (NB + 1) * sizeof(double), s));
      k::mgs_block_pass(vp.data(), m_prev, vp.data() + m_prev, m_next, init != 0, buf.p, buf.p + NB, h, PV(w)->all(), n,
                        sums, init ? h + NB : nullptr, s);
      d2h(out, sums, (size_t)(2 * NB + 2) * sizeof(double), s);
      break;
    }
    default: {
      const unsigned long long seq = ++c.post_seq;
      k::scale_inv_sqrt_post(slots, PV(w)->all(), n, slots, m, c.h_pinned + 256, c.h_post_flag, seq, s);
      MI_HIP(hipStreamSynchronize(s));
      for (int j = 0; j < m; j++) out[j] = c.h_pinned[256 + j];
      out[m] = (double)__atomic_load_n(c.h_post_flag, __ATOMIC_ACQUIRE);
      out[m + 1] = (double)seq;
    }
  }
  MI_HIP(hipStreamSynchronize(s));
  API_END
}

// The same hook for the kernels' instantiations on float basis vectors (Krylov basis storage mode 1): `vecs` are
// converted to float storage (round to nearest even, on the host) and ops 0, 1, 2 and 5 run the float instantiation on
// them; w, the coefficients and every result stay double.  Op 4 runs the rounding variant of the posting scaling:
// w = rd(w / sqrt(coef[0])), and the float slot the kernel also writes starts as xd's values converted and comes back
// widened in xd (xd NULL: the slot starts as zeros and is dropped).  Op 3 has no float instantiation.
HYPRE_Int HYPRE_MI_VectorKernelOpF32(HYPRE_Int op, HYPRE_Int m, HYPRE_ParVector *vecs, const HYPRE_Real *coef,
                                     HYPRE_Real scale, HYPRE_ParVector w, HYPRE_ParVector xd, HYPRE_Int init,
                                     HYPRE_Real *out) {
  API_BEGIN
  ensure_init();
  Ctx &c = ctx();
  hipStream_t s = c.stream;
  MI_REQUIRE(w, "VectorKernelOpF32: NULL vector w");
  MI_REQUIRE(op >= 0 && op <= 5 && op != 3, "VectorKernelOpF32: op must be 0, 1, 2, 4 or 5");
  const int mmax = (op <= 1) ? 120 : (op == 2 ? 250 : (op == 4 ? 255 : 2 * k::MGS_NB));
  MI_REQUIRE(m >= 1 && m <= mmax, "VectorKernelOpF32: m out of range for this op");
  MI_REQUIRE(op == 0 || coef, "VectorKernelOpF32: NULL coefficients");
  MI_REQUIRE(op == 1 || op == 2 || out, "VectorKernelOpF32: NULL output");
  const int n = PV(w)->len();
  MI_HIP(hipStreamSynchronize(s));
  // device doubles -> a float copy on the device, converted on the host
  auto narrowed = [&](const double *dev) {
    std::vector<double> h((size_t)n);
    if (n) d2h(h.data(), dev, (size_t)n * sizeof(double), s);
    std::vector<float> f((size_t)n);
    for (int i = 0; i < n; i++) f[(size_t)i] = (float)h[(size_t)i];
    DVec<float> d((size_t)n);
    if (n) d.upload(f.data(), (size_t)n);
    return d;
  };
  std::vector<DVec<float>> store;
  std::vector<const float *> vp;
  if (op != 4) {
    MI_REQUIRE(vecs, "VectorKernelOpF32: NULL vector list");
    for (int j = 0; j < m; j++) {
      MI_REQUIRE(vecs[j] && PV(vecs[j])->len() == n, "VectorKernelOpF32: vecs[j] is NULL or differs from w in length");
      MI_REQUIRE(vecs[j] != w, "VectorKernelOpF32: w among vecs");
      store.push_back(narrowed(PV(vecs[j])->all()));
      vp.push_back(store.back().p);
    }
  }
  MI_REQUIRE(!xd || (op == 4 && PV(xd)->len() == n && xd != w), "VectorKernelOpF32: xd goes with op 4 and has w's length");
  double *slots = c.red_out.p;
  if (op == 1 || op == 4) MI_HIP(hipMemcpyAsync(slots, coef, (size_t)m * sizeof(double), hipMemcpyHostToDevice, s));
  switch (op) {
    case 0:
      k::mass_dot(vp.data(), m, PV(w)->all(), n, slots, s);
      d2h(out, slots, (size_t)m * sizeof(double), s);
      break;
    case 1: k::mass_axpy(vp.data(), m, slots, scale, PV(w)->all(), n, s); break;
    case 2: k::lin_comb(vp.data(), coef, m, init != 0, PV(w)->all(), n, s); break;
    case 5: {
      constexpr int NB = k::MGS_NB;
      const int m_prev = (int)scale, m_next = init ? 0 : m - m_prev;
      MI_REQUIRE(m_prev >= 0 && m_prev <= NB && m_prev <= m && m - m_prev <= NB && (!init || m_prev == m),
                 "VectorKernelOpF32: op 5 takes at most MGS_NB vectors per block, and none to measure in the last pass");
      DVec<double> buf((size_t)NB * (NB + 2) + 3 * (NB + 1));  // c, Gram rows | sums, h, ||w||^2
      double *sums = buf.p + NB * (NB + 2), *h = sums + NB + 1;
      MI_HIP(hipMemcpyAsync(buf.p, coef, (size_t)NB * (NB + 2) * sizeof(double), hipMemcpyHostToDevice, s));
      MI_HIP(hipMemsetAsync(sums, 0, (size_t)3 * (NB + 1) * sizeof(double), s));
      k::mgs_block_pass(vp.data(), m_prev, vp.data() + m_prev, m_next, init != 0, buf.p, buf.p + NB, h, PV(w)->all(), n,
                        sums, init ? h + NB : nullptr, s);
      d2h(out, sums, (size_t)(2 * NB + 2) * sizeof(double), s);
      break;
    }
    default: {
      DVec<float> slot;
      if (xd) {
        slot = narrowed(PV(xd)->all());
      } else {
        slot.alloc((size_t)n);
        if (n) MI_HIP(hipMemsetAsync(slot.p, 0, (size_t)n * sizeof(float), s));
      }
      const unsigned long long seq = ++c.post_seq;
      k::scale_inv_sqrt_post_round(slots, PV(w)->all(), slot.p, n, slots, m, c.h_pinned + 256, c.h_post_flag, seq, s);
      MI_HIP(hipStreamSynchronize(s));
      for (int j = 0; j < m; j++) out[j] = c.h_pinned[256 + j];
      out[m] = (double)__atomic_load_n(c.h_post_flag, __ATOMIC_ACQUIRE);
      out[m + 1] = (double)seq;
      if (xd && n) {
        std::vector<float> f((size_t)n);
        d2h(f.data(), slot.p, (size_t)n * sizeof(float), s);
        std::vector<double> h(f.begin(), f.end());
        MI_HIP(hipMemcpy(PV(xd)->all(), h.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice));
      }
    }
  }
  MI_HIP(hipStreamSynchronize(s));
  API_END
}

HYPRE_Int HYPRE_MI_ArenaSelfTest(HYPRE_Int seed, HYPRE_Int rounds, HYPRE_BigInt max_block_bytes, HYPRE_BigInt *verified,
                                 HYPRE_BigInt *peak_bytes) {
  API_BEGIN
  ensure_init();
  struct Blk {
    unsigned char *p;
    size_t n;
    unsigned char tag;
  };
  std::vector<Blk> live;
  unsigned long long x = 88172645463325252ull ^ (unsigned long long)seed;
  auto rnd = [&]() {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return x;
  };
  long long ok = 0;
  size_t cur = 0, peak = 0;
  hipStream_t s = ctx().stream;
  DVec<unsigned long long> dres(3);
  auto differing = [&](const Blk &b, unsigned long long res[3]) {
    const unsigned long long init[3] = {0ull, ~0ull, 0ull};
    MI_HIP(hipMemcpyAsync(dres.p, init, sizeof(init), hipMemcpyHostToDevice, s));
    k::bytes_differ(b.p, b.n, b.tag, dres.p, s);
    d2h(res, dres.p, 3 * sizeof(unsigned long long), s);
  };
  auto check_and_free = [&](size_t idx) {
    Blk b = live[idx];
    live[idx] = live.back();
    live.pop_back();
    unsigned long long res[3];
    differing(b, res);  // EVERY byte of the block
    if (res[0])
      fail(HYPRE_ERROR_GENERIC, "arena self-test: a live block was overwritten: " + std::to_string(res[0]) + " of " + std::to_string(b.n) +
                                    " bytes differ, first at " + std::to_string(res[1]) + ", last at " + std::to_string(res[2]) +
                                    "; block at arena offset " + std::to_string((unsigned long long)(b.p - (unsigned char *)nullptr) & 0xffffffffffull));
    dev_free(b.p);
    cur -= b.n;
    ok++;
  };
  for (int r = 0; r < rounds; r++) {
    const unsigned long long v = rnd();
    const bool grow = live.empty() || (v & 3) != 0 || live.size() < 8;
    if (grow && live.size() < 4096) {
      // sizes spread over the classes: bytes .. max_block_bytes, log-uniform
      const int bits = 1 + (int)(rnd() % 34);
      size_t n = (size_t)(rnd() & ((1ull << bits) - 1)) + 1;
      n = std::min<size_t>(n, (size_t)std::max<HYPRE_BigInt>(1, max_block_bytes));
      Blk b{(unsigned char *)dev_alloc(n), n, (unsigned char)(1 + (rnd() % 250))};
      for (const Blk &o : live)  // the allocator's own bookkeeping first: no two live blocks may intersect
        if (b.p < o.p + o.n && o.p < b.p + b.n)
          fail(HYPRE_ERROR_GENERIC, "arena self-test: the allocator handed out a block that intersects a live one (round " +
                                        std::to_string(r) + ", " + std::to_string(n) + " bytes)");
      if (getenv("MI_ARENA_TEST_OWN_FILL"))
        k::fill_bytes(b.p, n, b.tag, s);
      else
        MI_HIP(hipMemsetAsync(b.p, b.tag, n, s));
      if (getenv("MI_ARENA_TEST_VERIFY_FILL")) {  // (diagnosis: is the fill itself complete?)
        unsigned long long res[3];
        differing(b, res);
        if (res[0])
          fail(HYPRE_ERROR_GENERIC, "arena self-test: the fill of a fresh block is incomplete: " + std::to_string(res[0]) + " of " +
                                        std::to_string(n) + " bytes, first " + std::to_string(res[1]) + ", last " + std::to_string(res[2]));
      }
      live.push_back(b);
      cur += n;
      peak = std::max(peak, cur);
    } else {
      check_and_free((size_t)(rnd() % live.size()));
    }
    if ((r & 255) == 255 && !getenv("MI_ARENA_TEST_NO_TRIM")) dev_pool_trim();  // unmap free chunks from the top in the middle of it all
  }
  MI_HIP(hipStreamSynchronize(s));
  while (!live.empty()) check_and_free(live.size() - 1);
  dev_pool_trim();
  if (verified) *verified = ok;
  if (peak_bytes) *peak_bytes = (HYPRE_BigInt)peak;
  API_END
}
HYPRE_Int HYPRE_MI_SetValueDictionary(HYPRE_Int on) {
  API_BEGIN
  k::set_value_dictionary(on != 0);
  API_END
}
HYPRE_Int HYPRE_MI_SetMultivectorBatch(HYPRE_Int width) {
  API_BEGIN
  if (width < 1 || width > k::MV_MAX_BATCH)
    fail(HYPRE_ERROR_ARG, "SetMultivectorBatch: the width is 1 (component by component), 2, 3 or 4 components per pass");
  k::set_multivector_batch(width);
  API_END
}
HYPRE_Int HYPRE_MI_GetMultivectorBatch(HYPRE_Int *width) {
  API_BEGIN
  if (!width) fail(HYPRE_ERROR_ARG, "GetMultivectorBatch: NULL argument");
  *width = k::multivector_batch();
  API_END
}
HYPRE_Int HYPRE_MI_SetGmresKeepDirections(HYPRE_Int on) {
  API_BEGIN
  gmres_keep_directions() = on != 0;
  API_END
}
HYPRE_Int HYPRE_MI_SetKrylovBasisStorage(HYPRE_Int mode) {
  API_BEGIN
  if (mode < 0 || mode > 2)
    fail(HYPRE_ERROR_ARG, "SetKrylovBasisStorage: the mode is 0 (fp64), 1 (float) or 2 (fp64 storage of float-rounded values)");
  krylov_basis_storage() = (int)mode;
  API_END
}
HYPRE_Int HYPRE_MI_GetKrylovBasisStorage(HYPRE_Int *mode) {
  API_BEGIN
  if (!mode) fail(HYPRE_ERROR_ARG, "GetKrylovBasisStorage: NULL argument");
  *mode = krylov_basis_storage();
  API_END
}
HYPRE_Int HYPRE_MI_TestGmresDirectionAllocFailsAt(HYPRE_Int at) {
  API_BEGIN
  gmres_keep_fail_at() = at < 0 ? -1 : (int)at;
  API_END
}
HYPRE_Int HYPRE_MI_GetGSChunk(HYPRE_Int *rows) {
  *rows = ctx().gs_chunk;
  return 0;
}
HYPRE_Int HYPRE_MI_KrylovGetResidualHistory(HYPRE_Solver solver, HYPRE_Real *norms, HYPRE_Int max_n, HYPRE_Int *n) {
  API_BEGIN
  KrylovSolver *kk = KR(solver);
  const int m = std::min<int>(max_n, (int)kk->norms.size());
  for (int i = 0; i < m; i++) norms[i] = kk->norms[(size_t)i];
  if (n) *n = (int)kk->norms.size();
  API_END
}
HYPRE_Int HYPRE_MI_KrylovGetSolveSeconds(HYPRE_Solver solver, HYPRE_Real *seconds) {
  API_BEGIN
  *seconds = KR(solver)->solve_seconds;
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetNumLevels(HYPRE_Solver solver, HYPRE_Int *n) {
  API_BEGIN
  *n = (HYPRE_Int)AMG(solver)->amg.total_levels();
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetOperatorComplexity(HYPRE_Solver solver, HYPRE_Real *cx) {
  API_BEGIN
  *cx = AMG(solver)->amg.operator_complexity();
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetSetupSeconds(HYPRE_Solver solver, HYPRE_Real *seconds) {
  API_BEGIN
  *seconds = AMG(solver)->amg.setup_seconds;
  API_END
}
// level of the whole hierarchy: the distributed levels, then the redundant tail's (its fine level replaces the stub)
static AmgLevel &level_ref(AmgSolver *a, int level, BoomerAMG **owner = nullptr, int *local = nullptr) {
  if (level < 0 || level >= a->amg.total_levels()) fail(HYPRE_ERROR_ARG, "AMG level out of range");
  int loc = 0;
  BoomerAMG &o = a->amg.owner_of(level, loc);
  if (owner) *owner = &o;
  if (local) *local = loc;
  return o.L[(size_t)loc];
}
static const HostCSR &level_csr(AmgSolver *a, int level, int which) {
  BoomerAMG *o = nullptr;
  int loc = 0;
  AmgLevel &L = level_ref(a, level, &o, &loc);
  o->ensure_host(loc);
  switch (which) {
    case 0: return L.A->diag;
    case 1: return L.A->offd;
    case 2:
    case 3:
    case 4:
    case 5: {
      const ParCSR *M = (which == 2 || which == 4) ? L.Pm.get() : L.Rm.get();
      static const HostCSR empty;
      if (!M) return empty;  // coarsest level has no transfer operators
      return which <= 3 ? M->diag : M->offd;
    }
    default: fail(HYPRE_ERROR_ARG, "which must be 0..5");
  }
}
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelCSRSize(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int which, HYPRE_Int *nrows,
                                            HYPRE_Int *ncols, HYPRE_BigInt *nnz) {
  API_BEGIN
  // sizes come from the level's metadata: no host copy of a device-resident level is made for them
  AmgLevel &L = level_ref(AMG(solver), level);
  if (which == 6) {  // the level's zero-guess sub-operator (0 x 0 when the level has none)
    *nrows = L.has_Az ? L.Az.nrows : 0;
    *ncols = L.has_Az ? L.Az.ncols : 0;
    *nnz = L.has_Az ? L.Az.nnz : 0;
    return 0;
  }
  if (which == 8) {  // operator of the residual after a zero-guess sweep (0 x 0 when the level has none)
    *nrows = L.has_Ar ? L.Ar.nrows : 0;
    *ncols = L.has_Ar ? L.Ar.ncols : 0;
    *nnz = L.has_Ar ? L.Ar.nnz : 0;
    return 0;
  }
  if (which == 9) {  // the C rows of the diag block (the level's C-first ordering: rows [0, nc))
    *nrows = L.nc;
    *ncols = L.A->diag.ncols;
    int e = 0;
    long long e64 = -1;
    if (L.nc > 0 && L.A->d_diag.ia64.p) d2h(&e64, L.A->d_diag.ia64.p + L.nc, sizeof(long long), nullptr);
    else if (L.nc > 0 && L.A->d_diag.ia.p) d2h(&e, L.A->d_diag.ia.p + L.nc, sizeof(int), nullptr);
    else if (L.nc > 0 && !L.A->diag.ia.empty()) e64 = (long long)L.A->diag.ia[(size_t)L.nc];
    *nnz = e64 >= 0 ? e64 : e;
    return 0;
  }
  if (which == 7) {  // x cache of the level operator: tiles, 0, total unique columns over the tiles
    *nrows = L.A->d_diag.nblocks;
    *ncols = 0;
    *nnz = (HYPRE_BigInt)L.A->d_diag.ucols.n;
    return 0;
  }
  const ParCSR *M = nullptr;
  switch (which) {
    case 0:
    case 1: M = L.A; break;
    case 2:
    case 4: M = L.Pm.get(); break;
    case 3:
    case 5: M = L.Rm.get(); break;
    default: fail(HYPRE_ERROR_ARG, "which must be 0..9");
  }
  if (!M) {
    *nrows = *ncols = 0;
    *nnz = 0;
  } else if (which == 0 || which == 2 || which == 3) {
    *nrows = M->diag.nrows;
    *ncols = M->diag.ncols;
    *nnz = M->diag_nnz();
  } else {
    *nrows = M->offd.nrows;
    *ncols = M->offd.ncols;
    *nnz = M->offd.nnz();
  }
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelCSR(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int which, HYPRE_BigInt *ia,
                                        HYPRE_Int *ja, HYPRE_Complex *a) {
  API_BEGIN
  if (which == 6 || which == 8) {  // the zero-guess sub-operators live on the device only
    AmgLevel &L = level_ref(AMG(solver), level);
    if (!(which == 6 ? L.has_Az : L.has_Ar)) {
      ia[0] = 0;
      return 0;
    }
    HostCSR h;
    sk::solve_format_to_host(which == 6 ? L.Az : L.Ar, h, ctx().stream);
    for (int i = 0; i <= h.nrows; i++) ia[i] = h.ia[(size_t)i];
    if (!h.ja.empty()) memcpy(ja, h.ja.data(), h.ja.size() * sizeof(int));
    if (!h.a.empty()) memcpy(a, h.a.data(), h.a.size() * sizeof(double));
    return 0;
  }
  const HostCSR &c = level_csr(AMG(solver), level, which);
  if (c.ia.empty()) {
    for (int i = 0; i <= c.nrows; i++) ia[i] = 0;
    return 0;
  }
  for (int i = 0; i <= c.nrows; i++) ia[i] = c.ia[(size_t)i];
  if (!c.ja.empty()) memcpy(ja, c.ja.data(), c.ja.size() * sizeof(int));
  if (!c.a.empty()) memcpy(a, c.a.data(), c.a.size() * sizeof(double));
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelValueStorage(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int which, HYPRE_Int *kind,
                                                 HYPRE_BigInt *value_bytes) {
  API_BEGIN
  AmgLevel &L = level_ref(AMG(solver), level);
  int kd = 0;
  long long bytes = 0;
  auto of_dev = [&](const DevCSR &D) {
    kd = D.reported_value_kind();
    bytes = k::value_stream_bytes(D);
  };
  if (which == 6 || which == 8) {
    if (which == 6 ? L.has_Az : L.has_Ar) of_dev(which == 6 ? L.Az : L.Ar);
  } else if (which >= 0 && which <= 5) {
    const int op = which <= 1 ? 0 : (which == 2 || which == 4) ? 1 : 2;
    const ParCSR *M = op == 0 ? L.A : op == 1 ? L.Pm.get() : L.Rm.get();
    if (M && (which == 0 || which == 2 || which == 3)) {
      if (M->d_diag.ia.p)
        of_dev(M->d_diag);
      else
        kd = L.value_kind[op];
    } else if (M) {
      kd = L.value_kind[op] ? 2 : 0;
      if (M->d_offd.a.p) bytes = (long long)(M->d_offd.a.n + 2) * 8;
    }
  } else {
    fail(HYPRE_ERROR_ARG, "which must be 0..5, 6 or 8");
  }
  if (kind) *kind = kd;
  if (value_bytes) *value_bytes = bytes;
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelCF(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int *cf) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  const auto &v = level_ref(a, level).cf;
  for (size_t i = 0; i < v.size(); i++) cf[i] = v[i];
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelDofFunc(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int *dof) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  AmgLevel &Lv = level_ref(a, level);
  if (!dof) fail(HYPRE_ERROR_ARG, "GetLevelDofFunc: NULL argument");
  if (Lv.dof.size() != (size_t)Lv.A->nrows)
    fail(HYPRE_ERROR_ARG, "GetLevelDofFunc: the hierarchy was built with num_functions 1 and keeps no dof_func");
  const std::vector<int> &v = Lv.dof.host();
  std::copy(v.begin(), v.end(), dof);
  API_END
}
// the colouring of a level set up with relax type 40 / 41 / 42 in some slot: info = colours, colouring rounds, (block,
// colour) ranges in the C block, ranges in the F block; colour (nullable): the colour of every row in stored order
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelColours(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int info[4], HYPRE_Int *colour) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  const AmgLevel &Lv = level_ref(a, level);
  if (!info) fail(HYPRE_ERROR_ARG, "GetLevelColours: NULL argument");
  if (!Lv.mc.ready)
    fail(HYPRE_ERROR_ARG, "GetLevelColours: the level was not coloured (Setup saw no relax_type 40 / 41 / 42, or the level is "
                          "solved densely)");
  const int nr = (int)Lv.mc.range_colour.size();
  info[0] = Lv.mc.colours;
  info[1] = Lv.mc.rounds;
  info[2] = Lv.mc.ranges_c;
  info[3] = nr - Lv.mc.ranges_c;
  if (colour)
    for (int r = 0; r < nr; r++)
      for (int i = Lv.mc.range_start[(size_t)r]; i < Lv.mc.range_start[(size_t)r + 1]; i++) colour[i] = Lv.mc.range_colour[(size_t)r];
  API_END
}
// diagonal and signed l1 norms of a level as the smoothers divide by them: from the host vectors of a level set up on
// the host, from the device vectors of a level set up on the device
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelNorms(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Real *diag, HYPRE_Real *l1gs,
                                          HYPRE_Real *l1jac) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  AmgLevel &Lv = level_ref(a, level);
  const size_t n = (size_t)Lv.A->nrows;
  auto get = [&](HYPRE_Real *out, const std::vector<double> &h, const DVec<double> &d) {
    if (!out || n == 0) return;
    if (h.size() == n)
      std::copy(h.begin(), h.end(), out);
    else if (d.p)
      MI_HIP(hipMemcpy(out, d.p, n * sizeof(double), hipMemcpyDeviceToHost));
    else
      fail(HYPRE_ERROR_GENERIC, "GetLevelNorms: the level has no norms (Setup did not finish)");
  };
  get(diag, Lv.diag, Lv.d_diag);
  get(l1gs, Lv.l1gs, Lv.d_l1gs);
  get(l1jac, Lv.l1jac, Lv.d_l1jac);
  API_END
}
// markers of the two coarsening stages of an aggressive level built with agg_interp_type 5, in the level's reported
// (C-first) ordering: the C points of the final marker first, the others after, both groups in natural order
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelAggMarkers(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int *stage1, HYPRE_Int *stage2) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  AmgLevel &Lv = level_ref(a, level);
  const size_t n = Lv.agg_m2.size();
  MI_REQUIRE(n > 0 && n == (size_t)Lv.A->nrows && Lv.agg_m1.size() == n,
             "GetLevelAggMarkers: the level was not built by the two-stage interpolation on this rank, or "
             "HYPRE_MI_BoomerAMGSetKeepAggMarkers was not set before Setup");
  size_t q = 0;
  for (int pass = 0; pass < 2; pass++)
    for (size_t i = 0; i < n; i++)
      if ((Lv.agg_m2[i] == 1) == (pass == 0)) {
        if (stage1) stage1[q] = Lv.agg_m1[i];
        if (stage2) stage2[q] = Lv.agg_m2[i];
        q++;
      }
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetInterpCensus(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int out[8]) {
  API_BEGIN
  const AmgLevel &Lv = level_ref(AMG(solver), level);
  const sk::InterpCensus &c = Lv.interp_census;
  const HYPRE_Int v[8] = {c.cap16, c.cap32, c.try32_kept, c.try32_retried, c.cap512, c.cap1024, c.max_bound,
                          (c.fell_back ? 1 : 0) | (Lv.interp_by_host ? 2 : 0)};
  for (int i = 0; i < 8; i++) out[i] = v[i];
  API_END
}
// how R of `level` was made: out[0] = 0 the transpose of P / 1 approximate ideal restriction built by the device / 2 by
// the host routine; out[1] = the largest |N_i|, out[2] = the C rows with an empty N_i, out[3] = the entries the filter dropped
HYPRE_Int HYPRE_MI_BoomerAMGGetRestrictionInfo(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int out[4]) {
  API_BEGIN
  if (!out) fail(HYPRE_ERROR_ARG, "BoomerAMGGetRestrictionInfo: NULL argument");
  const AmgLevel &Lv = level_ref(AMG(solver), level);
  out[0] = Lv.restriction_kind;
  out[1] = Lv.air_info.max_m;
  out[2] = Lv.air_info.zero_rows;
  out[3] = (HYPRE_Int)Lv.air_info.dropped;
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelPerm(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int *perm) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  const AmgLevel &Lv = level_ref(a, level);
  for (int i = 0; i < Lv.A->nrows; i++) perm[i] = Lv.perm.empty() ? i : Lv.perm[(size_t)i];
  API_END
}
// the internal locality numbering of the input (order[new] = caller's local row); *applied = 0 and the identity
// when the hierarchy was built on the caller's numbering
HYPRE_Int HYPRE_MI_BoomerAMGGetInputOrdering(HYPRE_Solver solver, HYPRE_Int *applied, HYPRE_Int *order) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  if (applied) *applied = a->amg.input_order.empty() ? 0 : 1;
  if (order) {
    const int n = a->amg.L.empty() ? 0 : a->amg.L[0].n;
    for (int i = 0; i < n; i++) order[i] = a->amg.input_order.empty() ? i : a->amg.input_order[(size_t)i];
  }
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelColMap(HYPRE_Solver solver, HYPRE_Int level, HYPRE_BigInt *col_map_offd,
                                           HYPRE_BigInt *row_start) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  const ParCSR &A = *level_ref(a, level).A;
  if (col_map_offd)
    for (size_t i = 0; i < A.col_map_offd.size(); i++) col_map_offd[i] = A.col_map_offd[i];
  if (row_start) *row_start = A.row_start;
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelOffdColMap(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int which,
                                               HYPRE_BigInt *col_map_offd) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  const AmgLevel &Lv = level_ref(a, level);
  const ParCSR *M = nullptr;
  switch (which) {
    case 1: M = Lv.A; break;
    case 4: M = Lv.Pm.get(); break;
    case 5: M = Lv.Rm.get(); break;
    default: fail(HYPRE_ERROR_ARG, "which must be 1 (A), 4 (P) or 5 (R)");
  }
  if (M)
    for (size_t i = 0; i < M->col_map_offd.size(); i++) col_map_offd[i] = M->col_map_offd[i];
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGRelaxLevel(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int relax_type, HYPRE_Int points,
                                       const HYPRE_Real *f_host, HYPRE_Real *u_host) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  if (!a->amg.is_setup) fail(HYPRE_ERROR_GENERIC, "RelaxLevel: AMG is not set up");
  if (level < 0 || level >= (int)a->amg.L.size()) fail(HYPRE_ERROR_ARG, "AMG level out of range");
  if (BoomerAMG::is_mcgs(relax_type) && points != 0)
    fail(HYPRE_ERROR_ARG, "RelaxLevel: relax type 40 / 41 / 42 (multicolour Gauss-Seidel) sweeps all rows: points must be 0");
  AmgLevel &Lv = a->amg.L[(size_t)level];
  const int n = Lv.n;
  DVec<double> f((size_t)n);
  if (n) {
    f.upload(f_host, (size_t)n);
    MI_HIP(hipStreamSynchronize(ctx().stream));
    MI_HIP(hipMemcpy(Lv.u.p, u_host, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  }
  a->amg.relax(level, relax_type, points, f.p);
  MI_HIP(hipStreamSynchronize(ctx().stream));
  if (n) d2h(u_host, Lv.u.p, (size_t)n * sizeof(double), nullptr);
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGRelaxPairLevel(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int relax_type, HYPRE_Int first,
                                           HYPRE_Int zero_guess, const HYPRE_Real *f_host, HYPRE_Real *u_host) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  if (!a->amg.is_setup) fail(HYPRE_ERROR_GENERIC, "RelaxPairLevel: AMG is not set up");
  if (level < 0 || level >= (int)a->amg.L.size()) fail(HYPRE_ERROR_ARG, "AMG level out of range");
  if (first != 1 && first != -1) fail(HYPRE_ERROR_ARG, "RelaxPairLevel: first is +1 (C then F) or -1 (F then C)");
  AmgLevel &Lv = a->amg.L[(size_t)level];
  const int n = Lv.n;
  DVec<double> f((size_t)n);
  if (n) {
    f.upload(f_host, (size_t)n);
    MI_HIP(hipStreamSynchronize(ctx().stream));
    if (zero_guess)
      MI_HIP(hipMemset(Lv.u.p, 0, (size_t)n * sizeof(double)));
    else
      MI_HIP(hipMemcpy(Lv.u.p, u_host, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  }
  a->amg.relax_pair(level, relax_type, first, f.p, zero_guess != 0);
  MI_HIP(hipStreamSynchronize(ctx().stream));
  if (n) d2h(u_host, Lv.u.p, (size_t)n * sizeof(double), nullptr);
  API_END
}
// the two hooks above on nvec component-major vectors at once (n apart): the passes of a batched cycle
static void relax_multi_check(AmgSolver *a, int level, int relax_type, int nvec, const char *who) {
  if (!a->amg.is_setup) fail(HYPRE_ERROR_GENERIC, std::string(who) + ": AMG is not set up");
  if (level < 0 || level >= (int)a->amg.L.size()) fail(HYPRE_ERROR_ARG, "AMG level out of range");
  if (nvec < 2 || nvec > k::MV_MAX_BATCH) fail(HYPRE_ERROR_ARG, std::string(who) + ": nvec is 2, 3 or 4");
  if (relax_type != 3 && relax_type != 4 && relax_type != 6 && relax_type != 8 && relax_type != 13 && relax_type != 14)
    fail(HYPRE_ERROR_ARG, std::string(who) + ": only the hybrid Gauss-Seidel relax types 3, 4, 6, 8, 13, 14 work on a batch");
  if (current_comm().size != 1) fail(HYPRE_ERROR_GENERIC, std::string(who) + ": a batched pass is a one-rank path");
}
HYPRE_Int HYPRE_MI_BoomerAMGRelaxLevelMulti(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int relax_type, HYPRE_Int points,
                                            HYPRE_Int nvec, const HYPRE_Real *f_host, HYPRE_Real *u_host) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  relax_multi_check(a, level, relax_type, nvec, "RelaxLevelMulti");
  AmgLevel &Lv = a->amg.L[(size_t)level];
  const size_t len = (size_t)nvec * (size_t)Lv.n;
  BoomerAMG::MvScope batch(a->amg, nvec);
  DVec<double> f(len);
  if (len) {
    f.upload(f_host, len);
    MI_HIP(hipStreamSynchronize(ctx().stream));
    MI_HIP(hipMemcpy(Lv.u.p, u_host, len * sizeof(double), hipMemcpyHostToDevice));
  }
  a->amg.relax(level, relax_type, points, f.p);
  MI_HIP(hipStreamSynchronize(ctx().stream));
  if (len) d2h(u_host, Lv.u.p, len * sizeof(double), nullptr);
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGRelaxPairLevelMulti(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int relax_type, HYPRE_Int first,
                                                HYPRE_Int zero_guess, HYPRE_Int nvec, const HYPRE_Real *f_host,
                                                HYPRE_Real *u_host) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  relax_multi_check(a, level, relax_type, nvec, "RelaxPairLevelMulti");
  if (first != 1 && first != -1) fail(HYPRE_ERROR_ARG, "RelaxPairLevelMulti: first is +1 (C then F) or -1 (F then C)");
  AmgLevel &Lv = a->amg.L[(size_t)level];
  const size_t len = (size_t)nvec * (size_t)Lv.n;
  BoomerAMG::MvScope batch(a->amg, nvec);
  DVec<double> f(len);
  if (len) {
    f.upload(f_host, len);
    MI_HIP(hipStreamSynchronize(ctx().stream));
    if (zero_guess)
      MI_HIP(hipMemset(Lv.u.p, 0, len * sizeof(double)));
    else
      MI_HIP(hipMemcpy(Lv.u.p, u_host, len * sizeof(double), hipMemcpyHostToDevice));
  }
  a->amg.relax_pair(level, relax_type, first, f.p, zero_guess != 0);
  MI_HIP(hipStreamSynchronize(ctx().stream));
  if (len) d2h(u_host, Lv.u.p, len * sizeof(double), nullptr);
  API_END
}
// test hooks (tests/test_gpu_cycle_steps.py): one cycle with every step recorded where the cycle runs it
HYPRE_Int HYPRE_MI_BoomerAMGTraceCycle(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int nvec, HYPRE_Int collapse,
                                       const HYPRE_Real *f_host, const HYPRE_Real *u0_host, HYPRE_Int *nrecords) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  if (!f_host || !nrecords) fail(HYPRE_ERROR_ARG, "TraceCycle: NULL argument");
  if (!a->amg.is_setup) fail(HYPRE_ERROR_GENERIC, "TraceCycle: AMG is not set up");
  if (current_comm().size != 1 || a->amg.tail) fail(HYPRE_ERROR_GENERIC, "TraceCycle: one rank only");
  if (level < 0 || level >= (int)a->amg.L.size()) fail(HYPRE_ERROR_ARG, "AMG level out of range");
  if (nvec < 1 || nvec > k::MV_MAX_BATCH) fail(HYPRE_ERROR_ARG, "TraceCycle: nvec is 1, 2, 3 or 4");
  *nrecords = 0;
  a->amg.trace_cycle(level, f_host, u0_host, nvec, collapse != 0, a->last_trace);
  *nrecords = (HYPRE_Int)a->last_trace.records.size();
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetTraceRecord(HYPRE_Solver solver, HYPRE_Int i, HYPRE_Int info[5], HYPRE_Real *values) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  if (!info) fail(HYPRE_ERROR_ARG, "GetTraceRecord: NULL argument");
  if (i < 0 || i >= (HYPRE_Int)a->last_trace.records.size()) fail(HYPRE_ERROR_ARG, "GetTraceRecord: no such record");
  const CycleTrace::Record &r = a->last_trace.records[(size_t)i];
  info[0] = r.level, info[1] = r.visit, info[2] = r.step, info[3] = r.flags, info[4] = (HYPRE_Int)r.values.size();
  if (values) std::copy(r.values.begin(), r.values.end(), values);
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelCycleInfo(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int out[6]) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  if (!out) fail(HYPRE_ERROR_ARG, "GetLevelCycleInfo: NULL argument");
  if (level < 0 || level >= (int)a->amg.L.size()) fail(HYPRE_ERROR_ARG, "AMG level out of range");
  const AmgLevel &Lv = a->amg.L[(size_t)level];
  out[0] = (Lv.Rm && Lv.Rm->d_diag.rowmap.p) ? 1 : 0;
  out[1] = Lv.t_from;
  out[2] = Lv.has_Ar ? 1 : 0;
  out[3] = Lv.has_Az ? 1 : 0;
  out[4] = Lv.nc;
  out[5] = a->amg.collapsed_level;
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetCollapsedTail(HYPRE_Solver solver, HYPRE_Int *level, HYPRE_Int *n, HYPRE_Real *Bt_host) {
  API_BEGIN
  BoomerAMG &amg = AMG(solver)->amg;
  if (!level || !n) fail(HYPRE_ERROR_ARG, "GetCollapsedTail: NULL argument");
  if (amg.is_setup && !amg.host_only && amg.mv_n == 1) amg.refresh_before_cycle();  // the map of the cycle's current settings
  *level = amg.collapsed_level;
  *n = amg.collapsed_level >= 0 ? amg.collapsed_n : 0;
  const size_t len = (size_t)*n * (size_t)*n;
  if (Bt_host && len) {
    MI_HIP(hipStreamSynchronize(ctx().stream));
    d2h(Bt_host, amg.collapsed_Bt.p, len * sizeof(double), nullptr);
  }
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetGSSweepPaths(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int points, HYPRE_Int zero_guess,
                                            HYPRE_Int *on_tiles, HYPRE_BigInt *counts) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  if (!a->amg.is_setup) fail(HYPRE_ERROR_GENERIC, "GetGSSweepPaths: AMG is not set up");
  if (level < 0 || level >= (int)a->amg.L.size()) fail(HYPRE_ERROR_ARG, "AMG level out of range");
  if (points < -1 || points > 1) fail(HYPRE_ERROR_ARG, "GetGSSweepPaths: points is 0, +1 or -1");
  long long c[5];
  const bool tiles = a->amg.gs_sweep_paths(level, points, zero_guess != 0, c);
  if (on_tiles) *on_tiles = tiles ? 1 : 0;
  for (int q = 0; q < 5; q++) counts[q] = c[q];
  API_END
}
static FsaiSolver *level_fsai_or_null(HYPRE_Solver solver, int level) {
  AmgSolver *a = AMG(solver);
  if (!a->amg.is_setup) fail(HYPRE_ERROR_GENERIC, "GetLevelFSAI: AMG is not set up");
  return level_fsai(level_ref(a, level));
}
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelFSAISize(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int *nrows, HYPRE_BigInt *nnz) {
  API_BEGIN
  FsaiSolver *fs = level_fsai_or_null(solver, level);
  *nrows = fs ? fs->G.nrows : 0;
  *nnz = fs ? (HYPRE_BigInt)fs->G.nnz : 0;
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelFSAI(HYPRE_Solver solver, HYPRE_Int level, HYPRE_BigInt *ia, HYPRE_Int *ja,
                                         HYPRE_Complex *a, HYPRE_Real *omega) {
  API_BEGIN
  FsaiSolver *fs = level_fsai_or_null(solver, level);
  if (!fs) fail(HYPRE_ERROR_ARG, "GetLevelFSAI: the level has no FSAI smoother");
  const HostCSR &g = fs->host_G();
  if (ia)
    for (int i = 0; i <= g.nrows; i++) ia[i] = g.ia.empty() ? 0 : g.ia[(size_t)i];
  if (ja && !g.ja.empty()) memcpy(ja, g.ja.data(), g.ja.size() * sizeof(int));
  if (a && !g.a.empty()) memcpy(a, g.a.data(), g.a.size() * sizeof(double));
  if (omega) *omega = fs->omega;
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelFSAIInfo(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int out[8]) {
  API_BEGIN
  FsaiSolver *fs = level_fsai_or_null(solver, level);
  if (!fs) fail(HYPRE_ERROR_ARG, "GetLevelFSAIInfo: the level has no FSAI smoother");
  if (!out) fail(HYPRE_ERROR_ARG, "GetLevelFSAIInfo: no buffer");
  for (int q = 0; q < 8; q++) out[q] = fs->setup_info[q];
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelILUOrdering(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int info[5], HYPRE_Int *perm,
                                                HYPRE_Int *colour) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  if (!a->amg.is_setup) fail(HYPRE_ERROR_GENERIC, "GetLevelILUOrdering: AMG is not set up");
  IluSolver *ilu = level_ilu(level_ref(a, level));
  if (!ilu) fail(HYPRE_ERROR_ARG, "GetLevelILUOrdering: the level has no ILU smoother");
  ilu_ordering_out(ilu, info, perm, colour);
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGGetLevelCheby(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Real *out) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  if (!a->amg.is_setup) fail(HYPRE_ERROR_GENERIC, "GetLevelCheby: AMG is not set up");
  if (!out) fail(HYPRE_ERROR_ARG, "GetLevelCheby: no buffer");
  BoomerAMG *o = nullptr;
  int loc = 0;
  AmgLevel &Lv = level_ref(a, level, &o, &loc);
  o->refresh_cheby();
  const AmgLevel::Cheby &c = Lv.cheby;
  if (!c.ready) fail(HYPRE_ERROR_ARG, "GetLevelCheby: the level has no Chebyshev data (Setup saw no relax_type 16)");
  out[0] = c.eig_min, out[1] = c.eig_max, out[2] = c.lower, out[3] = c.upper, out[4] = c.theta, out[5] = c.delta;
  API_END
}
HYPRE_Int HYPRE_MI_BoomerAMGSmoothLevel(HYPRE_Solver solver, HYPRE_Int level, HYPRE_Int zero_guess,
                                        const HYPRE_Real *f_host, HYPRE_Real *u_host) {
  API_BEGIN
  AmgSolver *a = AMG(solver);
  if (!a->amg.is_setup) fail(HYPRE_ERROR_GENERIC, "SmoothLevel: AMG is not set up");
  BoomerAMG *o = nullptr;
  int loc = 0;
  AmgLevel &Lv = level_ref(a, level, &o, &loc);
  if (!Lv.smoother) fail(HYPRE_ERROR_ARG, "SmoothLevel: the level has no complex smoother");
  const int n = Lv.n;
  DVec<double> f((size_t)n);
  hipStream_t s = ctx().stream;
  if (n) {
    f.upload(f_host, (size_t)n);
    MI_HIP(hipStreamSynchronize(s));
    MI_HIP(hipMemcpy(Lv.u.p, u_host, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  }
  // one sweep: num_sweeps[0] = 1 for the call
  const int keep = o->p.num_sweeps[0];
  o->p.num_sweeps[0] = 1;
  try {
    o->relax_sweeps(loc, 0, f.p, zero_guess != 0);
  } catch (...) {
    o->p.num_sweeps[0] = keep;
    throw;
  }
  o->p.num_sweeps[0] = keep;
  MI_HIP(hipStreamSynchronize(s));
  if (n) d2h(u_host, Lv.u.p, (size_t)n * sizeof(double), nullptr);
  API_END
}
HYPRE_Int HYPRE_MI_ProfileEnable(HYPRE_Int id, HYPRE_Int capacity) {
  API_BEGIN
  ensure_init();
  if (id < 0 || id >= k::PROF_COUNT) fail(HYPRE_ERROR_ARG, "ProfileEnable: bad id");
  if (!ctx().timer) ctx().timer = new KernelTimer();
  ctx().timer->enable(id, (size_t)capacity);
  API_END
}
HYPRE_Int HYPRE_MI_ProfileKernelName(HYPRE_Int id, char *name, HYPRE_Int max_len) {
  API_BEGIN
  if (!name || max_len < 1) fail(HYPRE_ERROR_ARG, "ProfileKernelName: no buffer");
  const char *n = (ctx().timer && id >= 0 && id < k::PROF_COUNT && ctx().timer->kernel_name[id]) ? ctx().timer->kernel_name[id] : "";
  snprintf(name, (size_t)max_len, "%s", n);
  API_END
}
HYPRE_Int HYPRE_MI_SolveKernelChoice(HYPRE_Int family, HYPRE_Int xcache, HYPRE_Int tile_entries, HYPRE_Int has_fp32,
                                     HYPRE_Int has_dictionary, HYPRE_Int epilogue, HYPRE_Int level0, HYPRE_Int chunk,
                                     HYPRE_Int tiles, HYPRE_BigInt nnz, HYPRE_Int nrows, HYPRE_Int rowlen_p95, char *name,
                                     HYPRE_Int max_len) {
  API_BEGIN
  if (!name || max_len < 1) fail(HYPRE_ERROR_ARG, "SolveKernelChoice: no buffer");
  if (family != 0 && family != 1) fail(HYPRE_ERROR_ARG, "SolveKernelChoice: family must be 0 (SpMV / Jacobi) or 1 (hybrid GS)");
  if (tile_entries != k::SPMV_TILE && tile_entries != k::SPMV_TILE_WIDE) fail(HYPRE_ERROR_ARG, "SolveKernelChoice: tile_entries must be 2048 or 4096");
  if (epilogue != 0 && epilogue != 1 && epilogue != 3)
    fail(HYPRE_ERROR_ARG, "SolveKernelChoice: epilogue must be 0, 1 or 3 (the in-place colour pass)");
  if (chunk < 1 || chunk > k::GS_MAX_CHUNK) fail(HYPRE_ERROR_ARG, "SolveKernelChoice: chunk out of range");
  if (nnz < 0 || nrows < 1 || rowlen_p95 < 0) fail(HYPRE_ERROR_ARG, "SolveKernelChoice: an operator has nnz >= 0, nrows >= 1, rowlen_p95 >= 0");
  k::SolveKernelDesc d;
  d.xcache = xcache != 0;
  d.tile_entries = tile_entries;
  d.format = value_format_of(has_fp32 != 0, has_dictionary != 0);
  d.epi = epilogue;
  d.level0 = level0 != 0;
  d.chunk = chunk;
  d.tiles = tiles != 0;
  d.nnz = nnz;
  d.nrows = nrows;
  d.rowlen_p95 = rowlen_p95;
  snprintf(name, (size_t)max_len, "%s", (family == 0 ? k::choose_stream_kernel(d) : k::choose_gs_kernel(d)).name);
  API_END
}
HYPRE_Int HYPRE_MI_SolveKernelChoiceMulti(HYPRE_Int nvec, HYPRE_Int family, HYPRE_Int xcache, HYPRE_Int tile_entries,
                                          HYPRE_Int has_fp32, HYPRE_Int has_dictionary, HYPRE_Int epilogue, HYPRE_Int level0,
                                          HYPRE_Int chunk, HYPRE_Int tiles, HYPRE_BigInt nnz, HYPRE_Int nrows,
                                          HYPRE_Int rowlen_p95, char *name, HYPRE_Int max_len, HYPRE_Int *batched) {
  API_BEGIN
  if (!name || max_len < 1 || !batched) fail(HYPRE_ERROR_ARG, "SolveKernelChoiceMulti: no buffer");
  if (nvec < 1 || nvec > k::MV_MAX_BATCH) fail(HYPRE_ERROR_ARG, "SolveKernelChoiceMulti: nvec is 1, 2, 3 or 4 components per pass");
  if (family != 0 && family != 1) fail(HYPRE_ERROR_ARG, "SolveKernelChoiceMulti: family must be 0 (SpMV / Jacobi) or 1 (hybrid GS)");
  if (tile_entries != k::SPMV_TILE && tile_entries != k::SPMV_TILE_WIDE) fail(HYPRE_ERROR_ARG, "SolveKernelChoiceMulti: tile_entries must be 2048 or 4096");
  if (epilogue != 0 && epilogue != 1 && epilogue != 3)
    fail(HYPRE_ERROR_ARG, "SolveKernelChoiceMulti: epilogue must be 0, 1 or 3 (the in-place colour pass)");
  if (chunk < 1 || chunk > k::GS_MAX_CHUNK) fail(HYPRE_ERROR_ARG, "SolveKernelChoiceMulti: chunk out of range");
  if (nnz < 0 || nrows < 1 || rowlen_p95 < 0) fail(HYPRE_ERROR_ARG, "SolveKernelChoiceMulti: an operator has nnz >= 0, nrows >= 1, rowlen_p95 >= 0");
  k::SolveKernelDesc d;
  d.xcache = xcache != 0;
  d.tile_entries = tile_entries;
  d.format = value_format_of(has_fp32 != 0, has_dictionary != 0);
  d.epi = epilogue;
  d.level0 = level0 != 0;
  d.chunk = chunk;
  d.tiles = tiles != 0;
  d.nnz = nnz;
  d.nrows = nrows;
  d.rowlen_p95 = rowlen_p95;
  d.nvec = nvec;
  const k::KernelChoice c = family == 0 ? k::choose_stream_kernel(d) : k::choose_gs_kernel(d);
  snprintf(name, (size_t)max_len, "%s", c.name);
  *batched = c.batched ? 1 : 0;
  API_END
}
HYPRE_Int HYPRE_MI_ChebyKernelChoice(HYPRE_Int xcache, HYPRE_Int tile_entries, HYPRE_Int has_fp32, HYPRE_Int has_dictionary,
                                     char *name, HYPRE_Int max_len) {
  API_BEGIN
  if (!name || max_len < 1) fail(HYPRE_ERROR_ARG, "ChebyKernelChoice: no buffer");
  if (tile_entries != k::SPMV_TILE && tile_entries != k::SPMV_TILE_WIDE) fail(HYPRE_ERROR_ARG, "ChebyKernelChoice: tile_entries must be 2048 or 4096");
  k::SolveKernelDesc d;
  d.xcache = xcache != 0;
  d.tile_entries = tile_entries;
  d.format = value_format_of(has_fp32 != 0, has_dictionary != 0);
  d.epi = 2;
  snprintf(name, (size_t)max_len, "%s", k::choose_stream_kernel(d).name);
  API_END
}
HYPRE_Int HYPRE_MI_ProfileReset(void) {
  API_BEGIN
  if (ctx().timer) {
    MI_HIP(hipStreamSynchronize(ctx().stream));
    ctx().timer->reset();
  }
  API_END
}
HYPRE_Int HYPRE_MI_ProfileGet(HYPRE_Int id, long long *launches, double *total_ms, double *min_ms) {
  API_BEGIN
  *launches = 0;
  *total_ms = *min_ms = 0.0;
  if (ctx().timer) ctx().timer->collect(id, launches, total_ms, min_ms);
  API_END
}

HYPRE_Int HYPRE_MI_Laplace3D(HYPRE_Int nx, HYPRE_Int ny, HYPRE_Int nz, HYPRE_Int stencil, HYPRE_BigInt ilower,
                             HYPRE_BigInt iupper, HYPRE_BigInt *nnz_out, HYPRE_BigInt **rows_out,
                             HYPRE_BigInt **cols_out, HYPRE_Complex **vals_out, HYPRE_Complex **rhs_out) {
  API_BEGIN
  if (stencil != 7 && stencil != 27) fail(HYPRE_ERROR_ARG, "Laplace3D: stencil must be 7 or 27");
  const gidx N = (gidx)nx * ny * nz;
  if (ilower < 0 || iupper >= N || iupper < ilower - 1) fail(HYPRE_ERROR_ARG, "Laplace3D: bad row range");
  const int64_t nloc = iupper - ilower + 1;
  const double dv = (stencil == 27) ? 26.0 : 6.0;
  auto row_nnz = [&](gidx row) {
    const int x = (int)(row % nx), y = (int)((row / nx) % ny), z = (int)(row / ((gidx)nx * ny));
    const int cx = 1 + (x > 0) + (x < nx - 1), cy = 1 + (y > 0) + (y < ny - 1), cz = 1 + (z > 0) + (z < nz - 1);
    return (stencil == 27) ? cx * cy * cz : 1 + (cx - 1) + (cy - 1) + (cz - 1);
  };
  std::vector<int64_t> off((size_t)nloc + 1, 0);
  parallel_for(nloc, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) off[(size_t)i + 1] = row_nnz(ilower + i);
  });
  for (int64_t i = 0; i < nloc; i++) off[(size_t)i + 1] += off[(size_t)i];
  const int64_t nnz = off[(size_t)nloc];
  gidx *rows = (gidx *)malloc(sizeof(gidx) * (size_t)std::max<int64_t>(nnz, 1));
  gidx *cols = (gidx *)malloc(sizeof(gidx) * (size_t)std::max<int64_t>(nnz, 1));
  double *vals = (double *)malloc(sizeof(double) * (size_t)std::max<int64_t>(nnz, 1));
  double *rhs = (double *)malloc(sizeof(double) * (size_t)std::max<int64_t>(nloc, 1));
  if (!rows || !cols || !vals || !rhs) {
    free(rows), free(cols), free(vals), free(rhs);
    fail(HYPRE_ERROR_MEMORY, "Laplace3D: out of host memory");
  }
  parallel_for(nloc, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      const gidx row = ilower + i;
      const int x = (int)(row % nx), y = (int)((row / nx) % ny), z = (int)(row / ((gidx)nx * ny));
      int64_t q = off[(size_t)i];
      double sum = 0.0;
      for (int dz = -1; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
          for (int dx = -1; dx <= 1; dx++) {
            if (stencil == 7 && (std::abs(dx) + std::abs(dy) + std::abs(dz) > 1)) continue;
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
  });
  *nnz_out = nnz;
  *rows_out = rows;
  *cols_out = cols;
  *vals_out = vals;
  *rhs_out = rhs;
  API_END
}
void HYPRE_MI_Free(void *p) { free(p); }

HYPRE_Int HYPRE_MI_Laplace3DDevice(HYPRE_Int nx, HYPRE_Int ny, HYPRE_Int nz, HYPRE_Int stencil, HYPRE_BigInt ilower,
                                   HYPRE_BigInt iupper, HYPRE_BigInt *nnz_out, HYPRE_BigInt **rows_out,
                                   HYPRE_BigInt **cols_out, HYPRE_Complex **vals_out, HYPRE_Complex **rhs_out) {
  API_BEGIN
  if (stencil != 7 && stencil != 27) fail(HYPRE_ERROR_ARG, "Laplace3DDevice: stencil must be 7 or 27");
  const gidx N = (gidx)nx * ny * nz;
  if (ilower < 0 || iupper >= N || iupper < ilower - 1) fail(HYPRE_ERROR_ARG, "Laplace3DDevice: bad row range");
  int64_t nnz = 0;
  ij::laplace3d_device(nx, ny, nz, stencil, ilower, iupper, &nnz, rows_out, cols_out, vals_out, rhs_out);
  *nnz_out = nnz;
  API_END
}
void HYPRE_MI_FreeDevice(void *p) {
  if (p) (void)hipFree(p);
}

}  // extern "C"
