// Block-Jacobi ILU(k) (HYPRE_ILU type 0, level of fill k >= 0): the preconditioner / solver behind
// `preconditioner: ilu` and `method: ilu` of the driver (src/HypreSystem.cpp:328-370, :457-497).
// Every rank factorises its own diagonal block in place; rows are grouped into level sets (row i is one
// level above the deepest row it depends on), which order both the factorisation and the substitutions:
// one kernel launch per level set, every row of a set independent of the others.  For ILU(0) the factors can instead come
// from fixed-point sweeps over all entries at once (the iterative setup, types 1-4; iterative_factor below).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "kernels.hpp"
#include "solvers.hpp"

namespace mi {

namespace {
// Symbolic ILU(k) of a rank's diagonal block (ilu.c hypre_ILUSetupILUKSymbolic; oracle/oracle.c ilu_symbolic; Saad,
// Iterative Methods, alg. 10.5): row by row, level 0 on A's pattern; every kept lower entry (i,k), in ascending k,
// lets every entry (k,j), j > k, of row k propose  lev(i,j) = lev(i,k) + lev(k,j) + 1,  merged into the row's sorted
// list when that is <= fill.  Out: the pattern with A's values on A's positions and zeros on the fill.
void ilu_symbolic(const HostCSR &B, int fill, HostCSR &F) {
  const int n = B.nrows;
  F.nrows = n;
  F.ncols = B.ncols;
  F.ia.assign((size_t)n + 1, 0);
  F.ja.clear();
  F.a.clear();
  F.ja.reserve((size_t)B.nnz() * (size_t)(fill + 1));
  F.a.reserve((size_t)B.nnz() * (size_t)(fill + 1));
  std::vector<int> lv;  // level of every stored entry
  lv.reserve((size_t)B.nnz() * (size_t)(fill + 1));
  std::vector<int64_t> dpos((size_t)n, -1);
  std::vector<int> next((size_t)n + 1, n), lev((size_t)n, 0);
  std::vector<double> val((size_t)n, 0.0);
  for (int i = 0; i < n; i++) {
    int last = n;
    next[(size_t)n] = n;
    for (int64_t k = B.ia[(size_t)i]; k < B.ia[(size_t)i + 1]; k++) {  // columns ascend
      const int j = B.ja[(size_t)k];
      next[(size_t)last] = j;
      next[(size_t)j] = n;
      last = j;
      lev[(size_t)j] = 0;
      val[(size_t)j] = B.a[(size_t)k];
    }
    for (int k = next[(size_t)n]; k < i; k = next[(size_t)k]) {  // (k == n ends the list: n > i)
      if (dpos[(size_t)k] < 0) continue;
      int at = k;  // the columns row k proposes ascend
      for (int64_t q = dpos[(size_t)k] + 1; q < F.ia[(size_t)k + 1]; q++) {
        const int j = F.ja[(size_t)q];
        const int nl = lev[(size_t)k] + lv[(size_t)q] + 1;
        if (nl > fill) continue;
        while (next[(size_t)at] != n && next[(size_t)at] < j) at = next[(size_t)at];
        if (next[(size_t)at] == j) {
          if (nl < lev[(size_t)j]) lev[(size_t)j] = nl;
        } else {
          next[(size_t)j] = next[(size_t)at];
          next[(size_t)at] = j;
          lev[(size_t)j] = nl;
          val[(size_t)j] = 0.0;
        }
      }
    }
    for (int j = next[(size_t)n]; j != n; j = next[(size_t)j]) {
      if (j == i) dpos[(size_t)i] = (int64_t)F.ja.size();
      F.ja.push_back(j);
      lv.push_back(lev[(size_t)j]);
      F.a.push_back(val[(size_t)j]);
    }
    F.ia[(size_t)i + 1] = (int64_t)F.ja.size();
  }
}

// B = P D P^T for perm[q] = the row of D that becomes row q of B (inv its inverse), columns ascending in every row
void permute_block(const HostCSR &D, const std::vector<int> &perm, const std::vector<int> &inv, HostCSR &B) {
  const int n = D.nrows;
  B.nrows = n;
  B.ncols = D.ncols;
  B.ia.assign((size_t)n + 1, 0);
  B.ja.resize((size_t)D.nnz());
  B.a.resize((size_t)D.nnz());
  std::vector<std::pair<int, double>> row;
  for (int q = 0; q < n; q++) {
    const int i = perm[(size_t)q];
    row.clear();
    for (int64_t k = D.ia[(size_t)i]; k < D.ia[(size_t)i + 1]; k++)
      row.emplace_back(inv[(size_t)D.ja[(size_t)k]], D.a[(size_t)k]);
    std::sort(row.begin(), row.end(), [](const std::pair<int, double> &x, const std::pair<int, double> &y) {
      return x.first < y.first;
    });
    int64_t o = B.ia[(size_t)q];
    for (const auto &e : row) B.ja[(size_t)o] = e.first, B.a[(size_t)o] = e.second, o++;
    B.ia[(size_t)q + 1] = o;
  }
}
}  // namespace

// Multicolour ordering of the block D: the colouring runs on the device; the colours come back
// once, perm lists the rows by (colour, original index), and the host mirror is permuted for the serial passes of the
// setup (symbolic ILU(k), level sets) that follow.
void IluSolver::multicolour_order(const HostCSR &D, HostCSR &B) {
  hipStream_t s = ctx().stream;
  const int nr = D.nrows;
  int rounds = 0;
  {
    sk::DCsr Dd;
    Dd.upload(D, s);
    // Thrown before the setup's failure all-reduce, which the other ranks would then wait in: every round colours at
    // least the first uncoloured row in priority order, so no input reaches this -- it guards the loop against a defect
    // of the kernel, not against data, and is therefore not an outcome the ranks agree on.
    if (sk::ilu_multicolour(Dd, colour, rounds, s) != 0)
      fail(1, "HYPRE_ILUSetup: the multicolour ordering left rows uncoloured after " + std::to_string(nr) +
                  " rounds, one per row");
  }
  const std::vector<int> col = colour.to_host();
  int ncol = 0;
  for (int c : col) ncol = std::max(ncol, c + 1);
  std::vector<int> start((size_t)ncol + 1, 0), inv((size_t)nr);
  for (int c : col) start[(size_t)c + 1]++;
  for (int c = 0; c < ncol; c++) start[(size_t)c + 1] += start[(size_t)c];
  perm_h.resize((size_t)nr);
  for (int i = 0; i < nr; i++) {  // ascending i inside a colour
    const int q = start[(size_t)col[(size_t)i]]++;
    perm_h[(size_t)q] = i;
    inv[(size_t)i] = q;
  }
  perm.upload(perm_h);
  permute_block(D, perm_h, inv, B);
  ordering_info[0] = 2;
  ordering_info[1] = ncol;
  ordering_info[2] = rounds;
}

void IluSolver::setup(ParCSR &A, Comm &comm) {
  ensure_init();
  hipStream_t s = ctx().stream;
  if (ilu_type != 0 || level_of_fill < 0)
    fail(1, "HYPRE_ILU: this variant is not implemented -- only type 0 (block-Jacobi ILU(k)) is (got type " +
                std::to_string(ilu_type) + ", fill " + std::to_string(level_of_fill) + ")");
  if (iter_type != 0) {
    if (iter_type < 0 || iter_type > 4)
      fail(1, "HYPRE_ILU: iterative setup type " + std::to_string(iter_type) + " is not implemented (0 ... 4 are)");
    if (level_of_fill != 0)
      fail(1, "HYPRE_ILU: the iterative setup with level of fill " + std::to_string(level_of_fill) +
                  " is not implemented (it exists for ILU(0) only)");
    if (iter_option & ~63)
      fail(1, "HYPRE_ILU: iterative setup option " + std::to_string(iter_option) +
                  " is not implemented (bits 1, 2, 4, 8, 16, 32 are)");
    if (iter_max_iter < 1) fail(1, "HYPRE_ILU: iterative setup max iterations must be >= 1");
  }
  MI_REQUIRE(!A.host_diag_stale, "HYPRE_ILUSetup: the matrix has no host arrays");
  is_setup = false;
  for (int &v : ordering_info) v = 0;
  perm.release();
  colour.release();
  xp.release();
  perm_h.clear();
  HostCSR reordered, filled;
  if (reordering == 2) multicolour_order(A.diag, reordered);  // before the symbolic pass: the fill is that of B
  const HostCSR &B = reordering == 2 ? reordered : A.diag;
  if (level_of_fill > 0) ilu_symbolic(B, level_of_fill, filled);  // the factors live on the ILU(k) pattern
  const HostCSR &D = level_of_fill > 0 ? filled : B;
  // a refusal names the row in the caller's numbering
  auto caller_row = [&](long long row) { return perm_h.empty() ? row : (long long)perm_h[(size_t)row]; };
  n = D.nrows;
  // the Jacobi triangular solves of an iteratively built factor need no level set: no serial pass over the block
  levels_built = iter_type == 0 || tri_solve != 0;
  // level sets of the lower and of the upper factor
  int nl = 0, nu = 0;
  if (levels_built) {
    std::vector<int> ll((size_t)n, 0), lu((size_t)n, 0);
    for (int i = 0; i < n; i++) {
      int lv = 0;
      for (int64_t k = D.ia[(size_t)i]; k < D.ia[(size_t)i + 1] && D.ja[(size_t)k] < i; k++)
        lv = std::max(lv, ll[(size_t)D.ja[(size_t)k]] + 1);
      ll[(size_t)i] = lv;
      nl = std::max(nl, lv + 1);
    }
    for (int i = n - 1; i >= 0; i--) {
      int lv = 0;
      for (int64_t k = D.ia[(size_t)i + 1] - 1; k >= D.ia[(size_t)i] && D.ja[(size_t)k] > i; k--)
        lv = std::max(lv, lu[(size_t)D.ja[(size_t)k]] + 1);
      lu[(size_t)i] = lv;
      nu = std::max(nu, lv + 1);
    }
    auto bucket = [&](const std::vector<int> &lev, int nlev, std::vector<int> &ptr, std::vector<int> &order) {
      ptr.assign((size_t)nlev + 1, 0);
      for (int i = 0; i < n; i++) ptr[(size_t)lev[(size_t)i] + 1]++;
      for (int l = 0; l < nlev; l++) ptr[(size_t)l + 1] += ptr[(size_t)l];
      order.resize((size_t)n);
      std::vector<int> cur(ptr.begin(), ptr.end() - 1);
      for (int i = 0; i < n; i++) order[(size_t)cur[(size_t)lev[(size_t)i]]++] = i;
    };
    std::vector<int> ol, ou;
    bucket(ll, nl, lptr, ol);
    bucket(lu, nu, uptr, ou);
    order_l.upload(ol);
    order_u.upload(ou);
  } else {
    lptr.clear();
    uptr.clear();
    order_l.release();
    order_u.release();
  }
  LU.upload(D, s);
  dpos.alloc((size_t)n);
  sk::ilu_diag_positions(LU, dpos.p, s);
  if (iter_type == 0) {
    // A row without a stored diagonal or with u_jj == 0 has no ILU factorisation (HYPRE's host ILU(k) puts 1e-6 in
    // place of a tiny pivot; here the setup ends).  The first is known from the pattern, before any kernel that reads
    // a[dpos[i]] runs; the second after the last level.  One all-reduce: every rank learns of a failure anywhere.
    long long bad_row = -1;
    bool stored = true;
    for (int i = 0; i < n && bad_row < 0; i++) {
      const int *b = D.ja.data() + D.ia[(size_t)i], *e = D.ja.data() + D.ia[(size_t)i + 1];
      if (!std::binary_search(b, e, i)) bad_row = i, stored = false;  // columns ascend
    }
    if (bad_row < 0) {
      for (int l = 0; l < nl; l++)
        sk::ilu_factor_level(LU, dpos.p, order_l.p + lptr[(size_t)l], lptr[(size_t)l + 1] - lptr[(size_t)l], s);
      MI_HIP(hipGetLastError());
      bad_row = sk::ilu_zero_pivot(LU, dpos.p, s);
    }
    if (bad_row >= 0) bad_row = caller_row(bad_row);
    double err = bad_row >= 0 ? 1.0 : 0.0;
    comm.allreduce_host(&err, 1, CommDType::F64, CommOp::MAX);
    if (bad_row >= 0)
      fail(1, "HYPRE_ILUSetup: ILU(" + std::to_string(level_of_fill) + ") setup: zero pivot u_jj in row " +
                  std::to_string(bad_row) + " of this rank's block (global row " +
                  std::to_string((long long)A.row_start + bad_row) + ")" +
                  (stored ? "" : ": the row stores no diagonal entry"));
    if (err > 0.0) fail(1, "HYPRE_ILUSetup: ILU(" + std::to_string(level_of_fill) + ") setup failed on another rank");
  } else {
    iterative_factor(comm, (long long)A.row_start);
  }
  MI_HIP(hipGetLastError());
  y.alloc((size_t)n);
  t.alloc((size_t)n);
  r.alloc((size_t)n);
  z.alloc((size_t)n);
  if (reordering == 2) xp.alloc((size_t)n);
  ordering_info[3] = nl;
  ordering_info[4] = nu;
  zero_on_stream(y.p, (size_t)n * sizeof(double));
  zero_on_stream(t.p, (size_t)n * sizeof(double));
  MI_HIP(hipStreamSynchronize(s));
  is_setup = true;
  if (print_level > 0 && comm.rank == 0 && reordering == 2)
    printf("mi_hypre ILU multicolour ordering: %d colours in %d rounds\n", ordering_info[1], ordering_info[2]);
  if (print_level > 0 && comm.rank == 0 && levels_built)
    printf("mi_hypre ILU(%d): %d rows, %lld entries, %d lower / %d upper level sets, %s triangular solves\n", level_of_fill, n,
           (long long)LU.nnz, nl, nu, tri_solve ? "exact" : "Jacobi");
  else if (print_level > 0 && comm.rank == 0)
    printf("mi_hypre ILU(%d): %d rows, %lld entries, no level sets, Jacobi triangular solves\n", level_of_fill, n,
           (long long)LU.nnz);
}

// Iterative ILU(0) setup (types 1-4): x_0, then at most iter_max_iter fixed-point sweeps on this
// rank's block -- type 3 synchronous (two value buffers), 4 the same with the correction fused into the sweep, 1 and 2
// asynchronous in place (1 on LU's own values, 2 on split L / U-by-column storage) -- then the values land in LU.
// Norms are taken per sweep only when an option bit asks for them; each costs one small download.  One all-reduce at
// the end: every rank learns of a failure anywhere, and rank 0 reports the largest sweeps and norms.
void IluSolver::iterative_factor(Comm &comm, long long row0) {
  hipStream_t s = ctx().stream;
  const bool stop = iter_option & 2, want_c = stop || (iter_option & 4), want_r = iter_option & 8,
             keep = iter_option & 16, verbose = (iter_option & 1) && print_level > 0 && comm.rank == 0;
  iter_sweeps = 0;
  iter_correction = iter_residual = -1.0;
  iter_corr_hist.clear();
  iter_res_hist.clear();
  int err = 0;  // 1: zero pivot in bad_row, 2: too many entries for 32-bit slots
  long long bad_row = -1;
  if (LU.nnz > (long long)INT32_MAX - 2) err = 2;
  sk::ItiluPlan P;
  if (!err) {
    const int r = sk::itilu_plan(LU, dpos.p, iter_type != 1, P, s);
    if (r >= 0) err = 1, bad_row = r;
  }
  if (!err && P.nnz) {
    DVec<unsigned long long> st(4);
    auto as_double = [](unsigned long long b) {
      double d;
      memcpy(&d, &b, sizeof d);
      return d;
    };
    auto reset_norms = [&]() { MI_HIP(hipMemsetAsync(st.p, 0, 3 * sizeof(unsigned long long), s)); };
    MI_HIP(hipMemsetAsync(st.p + 3, 0xff, sizeof(unsigned long long), s));
    double amax = 0.0;
    if (want_r) {
      reset_norms();
      sk::itilu_abs_max(P, st.p, s);
      unsigned long long b = 0;
      d2h(&b, st.p, sizeof b, s);
      amax = as_double(b);
    }
    DVec<double> xa, xb;
    double *cur = LU.a.p, *nxt = nullptr;
    if (iter_type != 1) {
      xa.alloc((size_t)P.nnz);
      cur = xa.p;
    }
    if (iter_type >= 3) {
      xb.alloc((size_t)P.nnz);
      nxt = xb.p;
    }
    sk::itilu_start(P, cur, st.p, s);
    for (int m = 1; m <= iter_max_iter; m++) {
      if (want_c || want_r) reset_norms();
      if (iter_type >= 3) {
        sk::itilu_sweep(P, cur, nxt, iter_type == 4, st.p, s);
        if (iter_type == 3 && want_c) sk::itilu_correction(P, cur, nxt, st.p, s);
        std::swap(cur, nxt);
      } else {
        sk::itilu_async_sweep(P, cur, want_c, st.p, s);
      }
      if (want_r) sk::itilu_residual(P, cur, st.p, s);
      MI_HIP(hipGetLastError());
      iter_sweeps = m;
      if (!(want_c || want_r)) continue;
      unsigned long long h[4];
      d2h(h, st.p, sizeof h, s);
      if (want_c) {
        const double xm = as_double(h[1]);
        iter_correction = xm > 0.0 ? as_double(h[0]) / xm : as_double(h[0]);
        if (keep) iter_corr_hist.push_back(iter_correction);
      }
      if (want_r) {
        iter_residual = amax > 0.0 ? as_double(h[2]) / amax : as_double(h[2]);
        if (keep) iter_res_hist.push_back(iter_residual);
      }
      if (verbose)
        printf("mi_hypre ILU iterative setup (type %d) sweep %d: correction %.6e, residual %.6e\n", iter_type, m,
               iter_correction, iter_residual);
      if (h[3] != ~0ull) break;  // a zero pivot: reported below
      if (stop && iter_correction <= iter_tol) break;
    }
    unsigned long long piv = 0;
    d2h(&piv, st.p + 3, sizeof piv, s);
    if (piv != ~0ull) err = 1, bad_row = (long long)piv;
    if (!err && iter_type != 1) sk::itilu_scatter(P, cur, LU, s);
    MI_HIP(hipStreamSynchronize(s));  // the value buffers are released on return
  }
  double v[4] = {(double)err, (double)iter_sweeps, iter_correction, iter_residual};
  comm.allreduce_host(v, 4, CommDType::F64, CommOp::MAX);
  if (err == 1 && !perm_h.empty()) bad_row = perm_h[(size_t)bad_row];  // the caller's row
  if (err == 1)
    fail(1, "HYPRE_ILUSetup: iterative ILU(0) setup: zero pivot u_jj in row " + std::to_string(bad_row) +
                " of this rank's block (global row " + std::to_string(row0 + bad_row) + ")");
  if (err == 2)
    fail(1, "HYPRE_ILUSetup: the iterative ILU(0) setup is not implemented for more than 2^31 - 3 entries per rank (" +
                std::to_string((long long)LU.nnz) + ")");
  if (v[0] > 0.0) fail(1, "HYPRE_ILUSetup: iterative ILU(0) setup failed on another rank");
  if (print_level > 0 && comm.rank == 0)
    printf("mi_hypre ILU iterative setup (type %d, option %d): %d sweeps (max over ranks), correction %.3e, residual "
           "%.3e\n", iter_type, iter_option, (int)v[1], v[2], v[3]);
}

void IluSolver::apply(const double *rhs, double *out) {
  hipStream_t s = ctx().stream;
  MI_REQUIRE(!tri_solve || levels_built,
             "HYPRE_ILUSolve: exact triangular solves need the level sets, which a setup with trisolve 0 did not build");
  // reordering 2: LU holds the factors of B = P D P^T.  The lower substitution gathers rhs through perm, the upper one
  // leaves its result in B's numbering (xp), and one pass scatters it into out.
  const int *pm = perm.p;  // null without the ordering
  double *const res = pm ? xp.p : out;
  if (tri_solve) {
    const int nl = (int)lptr.size() - 1, nu = (int)uptr.size() - 1;
    for (int l = 0; l < nl; l++)
      sk::ilu_lower_level(LU, dpos.p, order_l.p + lptr[(size_t)l], lptr[(size_t)l + 1] - lptr[(size_t)l], pm, rhs, y.p, s);
    for (int l = 0; l < nu; l++)
      sk::ilu_upper_level(LU, dpos.p, order_u.p + uptr[(size_t)l], uptr[(size_t)l + 1] - uptr[(size_t)l], y.p, res, s);
  } else {
    // y <- rhs - L_strict y (lower_it times from y = rhs); out <- D^-1 (y - U_strict out) (upper_it times from D^-1 y)
    double *a = y.p, *b2 = t.p;
    sk::ilu_lower_jacobi(LU, dpos.p, pm, rhs, nullptr, a, s);
    for (int it = 0; it < lower_it; it++) {
      sk::ilu_lower_jacobi(LU, dpos.p, pm, rhs, a, b2, s);
      std::swap(a, b2);
    }
    // a holds y; use b2 and res alternately, finishing in res
    double *zi = (upper_it % 2 == 0) ? res : b2, *zo = (upper_it % 2 == 0) ? b2 : res;
    sk::ilu_upper_jacobi(LU, dpos.p, a, nullptr, zi, s);
    for (int it = 0; it < upper_it; it++) {
      sk::ilu_upper_jacobi(LU, dpos.p, a, zi, zo, s);
      std::swap(zi, zo);
    }
    if (zi != res) k::copy(zi, res, n, s);
  }
  if (pm) sk::ilu_unpermute(pm, xp.p, out, n, s);
  MI_HIP(hipGetLastError());
}

int IluSolver::solve(ParCSR &A, ParVector &b, ParVector &x) {
  if (!is_setup) setup(A, current_comm());
  MI_REQUIRE(b.n == n && x.n == n, "HYPRE_ILUSolve: vector size does not match the matrix");
  MI_REQUIRE(b.ncomp == x.ncomp, "HYPRE_ILUSolve: b and x differ in their number of components");
  Comm &comm = current_comm();
  hipStream_t s = ctx().stream;
  const int nc = b.ncomp;  // a multivector is treated component by component
  // preconditioner use (one application, no tolerance) on a zero guess: x = M^-1 b
  if (max_iter == 1 && tol <= 0.0 && zero_guess_hint()) {
    zero_guess_hint() = false;
    for (int c = 0; c < nc; c++) apply(b.all() + (size_t)c * (size_t)n, x.all() + (size_t)c * (size_t)n);
    num_iterations = 1;
    return 0;
  }
  zero_guess_hint() = false;
  const double bn = (tol > 0.0) ? std::sqrt(par_dot_host(comm, b.all(), b.all(), b.len(), s)) : 0.0;
  int it = 0;
  double rel = 0.0;
  // with a tolerance the residuals of all components are needed BEFORE the update (one norm over the multivector):
  // they are kept (rall: nc * n, allocated on first use) and reused by the update instead of being recomputed
  if (tol > 0.0 && nc > 1 && rall.n != (size_t)nc * (size_t)n) rall.alloc((size_t)nc * (size_t)n);
  while (it < max_iter) {
    if (tol > 0.0) {
      double rr = 0.0;
      for (int c = 0; c < nc; c++) {
        const size_t o = (size_t)c * (size_t)n;
        double *rc = (nc > 1) ? rall.p + o : r.p;
        A.matvec(comm, -1.0, x.all() + o, 1.0, b.all() + o, rc, s);
        rr += par_dot_host(comm, rc, rc, n, s);
      }
      const double rn = std::sqrt(rr);
      rel = (bn > 0.0) ? rn / bn : rn;
      if (rel <= tol) break;
    }
    for (int c = 0; c < nc; c++) {
      const size_t o = (size_t)c * (size_t)n;
      double *rc = (tol > 0.0 && nc > 1) ? rall.p + o : r.p;
      if (!(tol > 0.0)) A.matvec(comm, -1.0, x.all() + o, 1.0, b.all() + o, rc, s);
      apply(rc, z.p);
      k::axpy(1.0, z.p, x.all() + o, n, s);
    }
    it++;
  }
  num_iterations = it;
  final_rel_res = rel;
  return 0;
}

}  // namespace mi
