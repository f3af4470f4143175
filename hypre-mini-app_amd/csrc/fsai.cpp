// Factorized sparse approximate inverse (HYPRE_FSAI): the preconditioner / solver of HYPRE_FSAI* and BoomerAMG's
// complex smoother smooth_type 4.  Every rank works on its own diagonal block B (block Jacobi
// across ranks): G is sparse lower triangular with G B G^T ~ I, and one step is u += omega G^T G (f - A u).
// Setup, algo type 3 (static pattern): filtered pattern, its symbolic k-th power (device SpGEMM), one small dense
// solve per row (sk::fsai_local_solve).  Algo type 4 (adaptive pattern, this library's number): every row grows its
// pattern from the Kaporin gradient inside one kernel (sk::fsai_adaptive).  Both: G^T by the device transpose, omega
// by power iteration on G B G^T.
#include <cmath>

#include "kernels.hpp"
#include "solvers.hpp"

namespace mi {

void FsaiSolver::check_adaptive(const std::string &where, int max_steps, int max_step_size, double kap_tolerance) {
  if (max_steps < 1 || max_step_size < 1)
    fail(4, where + ": FSAI max_steps " + std::to_string(max_steps) + " / max_step_size " + std::to_string(max_step_size) +
                " is not implemented: both must be >= 1");
  if ((long long)max_steps * max_step_size + 1 > 64)
    fail(4, where + ": FSAI max_steps " + std::to_string(max_steps) + " x max_step_size " + std::to_string(max_step_size) +
                " + 1 entries in a row is not implemented: the row bound must be <= 64");
  if (!(kap_tolerance >= 0.0) || !std::isfinite(kap_tolerance))
    fail(4, where + ": FSAI kap_tolerance is not implemented for this value: it must be finite and >= 0");
}

void FsaiSolver::setup(ParCSR &A, Comm &comm, const std::string &where) {
  ensure_init();
  hipStream_t s = ctx().stream;
  is_setup = false;
  if (algo_type != 3 && algo_type != 4)
    fail(4, where + ": FSAI algo_type " + std::to_string(algo_type) +
                " is not implemented (3 = static pattern and 4 = adaptive pattern are); refusing to substitute another one");
  const bool adaptive = algo_type == 4;
  if (adaptive) check_adaptive(where, max_steps, max_step_size, kap_tolerance);
  if (!adaptive && (num_levels < 1 || num_levels > 3))
    fail(4, where + ": FSAI num_levels " + std::to_string(num_levels) + " is not implemented (1, 2 and 3 are)");
  if (!adaptive && !(threshold >= 0.0)) fail(4, where + ": FSAI threshold must be >= 0");
  if (eig_max_iters < 0) fail(4, where + ": FSAI eig_max_iters must be >= 0");
  MI_REQUIRE(A.on_device, (where + ": the matrix is not on the device").c_str());
  n = A.nrows;
  sk::DCsr B, P, Gd, Gtd;
  int rc = 0, bad_row = -1, bad_kind = 0;
  max_row = 0;
  sk::FsaiAdaptiveInfo ai;
  if (n == 0) {  // a rank without rows: empty factors, but it takes part in every collective below
    sk::fsai_local_solve(B, P, Gd, max_row, bad_row, bad_kind, s);
  } else {
    if (!A.d_diag.rowmap.p && A.d_diag.nrows == n) {
      sk::from_solve_format(A.d_diag, B, s);
    } else {
      MI_REQUIRE(!A.host_diag_stale, (where + ": the matrix has no host arrays").c_str());
      B.upload(A.diag, s);
    }
  }
  if (n > 0 && adaptive) {
    rc = sk::fsai_adaptive(B, max_steps, max_step_size, kap_tolerance, 0, Gd, ai, s);
    max_row = ai.max_row, bad_row = ai.bad_row, bad_kind = ai.bad_kind;
  } else if (n > 0) {
    // pattern: lower triangle of the k-th power of the filtered graph (values 1: no product cancels)
    sk::DCsr S;
    sk::fsai_select(B, threshold, true, num_levels == 1, S, s);
    if (num_levels == 1) {
      P = std::move(S);
    } else {
      sk::DCsr S2, S3;
      sk::spgemm(S, S, S2, s);
      if (num_levels == 3) sk::spgemm(S2, S, S3, s);
      sk::fsai_select(num_levels == 3 ? S3 : S2, 0.0, false, true, P, s);
    }
    rc = sk::fsai_local_solve(B, P, Gd, max_row, bad_row, bad_kind, s);
  }
  // every rank learns whether any failed (the others would wait in the eigenvalue estimate's all-reduces otherwise)
  {
    long long v[2] = {rc, max_row};
    comm.allreduce_host(v, 2, CommDType::I64, CommOp::MAX);
    if (v[0] == 1) rc = 1, max_row = (int)v[1];
    else if (v[0] == 2 && rc == 0) rc = 3;  // another rank's row
  }
  if (rc == 1)
    fail(4, where + ": the FSAI pattern has up to " + std::to_string(max_row) + " entries in a row (" + std::to_string(n) +
                " rows on this rank); the limit is 64 -- lower fsai_num_levels or raise fsai_threshold");
  if (rc == 2)
    fail(1, where + ": FSAI local solve failed in row " + std::to_string(bad_row) +
                (bad_kind == 1 ? " (singular local matrix)" : " (y_last <= 0: the diagonal block is not positive definite there)"));
  if (rc == 3) fail(1, where + ": FSAI local solve failed on another rank");
  const int si[8] = {0, max_row, ai.max_candidates, ai.overflow_rows, ai.stop_tolerance, ai.stop_no_candidate,
                     ai.stop_max_steps, -1};
  for (int q = 0; q < 8; q++) setup_info[q] = si[q];
  P.release();
  B.release();
  sk::transpose(Gd, Gtd, s);
  sk::to_solve_format(Gd, G, s);
  sk::to_solve_format(Gtd, Gt, s);
  t.alloc((size_t)n);
  r.alloc((size_t)n);
  if (n) {
    zero_on_stream(t.p, (size_t)n * sizeof(double));
    zero_on_stream(r.p, (size_t)n * sizeof(double));
  }
  // omega = 1 / (Rayleigh quotient of G B G^T after eig_max_iters power iterations); inner products all-reduced
  if (omega_user > 0.0) {
    omega = omega_user;
  } else if (eig_max_iters == 0) {
    omega = 1.0;
  } else {
    DVec<double> z((size_t)n);  // only for the estimate
    double *v = r.p, *w = z.p;
    sk::fsai_random_vector(n, (long long)A.row_start, 2747, v, s);  // the PMIS measures' seed
    double lambda = 0.0;
    for (int it = 0; it < eig_max_iters; it++) {
      k::spmv(Gt, v, 1.0, 0.0, nullptr, t.p, s);
      k::spmv(A.d_diag, t.p, 1.0, 0.0, nullptr, w, s);
      k::spmv(G, w, 1.0, 0.0, nullptr, t.p, s);
      const double vw = par_dot_host(comm, v, t.p, n, s);
      const double vv = par_dot_host(comm, v, v, n, s);
      const double ww = par_dot_host(comm, t.p, t.p, n, s);
      lambda = vw / vv;
      if (!(ww > 0.0)) break;
      if (n) {
        k::copy(t.p, v, n, s);
        k::scale(1.0 / std::sqrt(ww), v, n, s);
      }
    }
    if (!(lambda > 0.0) || !std::isfinite(lambda))
      fail(1, where + ": FSAI eigenvalue estimate of G A G^T is not positive (" + std::to_string(lambda) + ")");
    omega = 1.0 / lambda;
    if (n) zero_on_stream(r.p, (size_t)n * sizeof(double));
    MI_HIP(hipStreamSynchronize(s));  // z is released on return
  }
  MI_HIP(hipStreamSynchronize(s));
  host_G_ok = false;
  is_setup = true;
  if (print_level > 0 && comm.rank == 0)
    printf("mi_hypre FSAI: %d rows, G with %lld entries (at most %d per row), omega %.6g\n", n, (long long)G.nnz, max_row,
           omega);
}

void FsaiSolver::apply_add(const double *res, double *u, bool zero, int prof) {
  hipStream_t s = ctx().stream;
  const int pc = prof < 0 ? k::PROF_NONE : prof;
  k::spmv(G, res, 1.0, 0.0, nullptr, t.p, s, pc);
  // the omega-scaled update in the G^T product's epilogue: u = omega G^T t (+ u)
  k::spmv(Gt, t.p, omega, zero ? 0.0 : 1.0, zero ? nullptr : u, u, s, pc);
}

const HostCSR &FsaiSolver::host_G() {
  if (!host_G_ok) {
    sk::solve_format_to_host(G, hG, ctx().stream);
    host_G_ok = true;
  }
  return hG;
}

int FsaiSolver::solve(ParCSR &A, ParVector &b, ParVector &x) {
  if (!is_setup) setup(A, current_comm(), "HYPRE_FSAISolve");
  MI_REQUIRE(b.n == n && x.n == n, "HYPRE_FSAISolve: vector size does not match the matrix");
  MI_REQUIRE(b.ncomp == x.ncomp, "HYPRE_FSAISolve: b and x differ in their number of components");
  Comm &comm = current_comm();
  hipStream_t s = ctx().stream;
  const int nc = b.ncomp;
  const bool zero = zero_guess || zero_guess_hint();
  zero_guess_hint() = false;
  const double bn = (tol > 0.0) ? std::sqrt(par_dot_host(comm, b.all(), b.all(), b.len(), s)) : 0.0;
  int it = 0;
  double rel = 0.0;
  for (int c = 0; c < nc && zero && n > 0; c++) k::fill(x.all() + (size_t)c * (size_t)n, n, 0.0, s);
  while (it < max_iter) {
    if (tol > 0.0) {
      double rr = 0.0;
      for (int c = 0; c < nc; c++) {
        const size_t o = (size_t)c * (size_t)n;
        A.matvec(comm, -1.0, x.all() + o, 1.0, b.all() + o, r.p, s);
        rr += par_dot_host(comm, r.p, r.p, n, s);
      }
      const double rn = std::sqrt(rr);
      rel = (bn > 0.0) ? rn / bn : rn;
      if (rel <= tol) break;
    }
    for (int c = 0; c < nc; c++) {
      const size_t o = (size_t)c * (size_t)n;
      if (it == 0 && zero) {
        apply_add(b.all() + o, x.all() + o, true);
      } else {
        A.matvec(comm, -1.0, x.all() + o, 1.0, b.all() + o, r.p, s);
        apply_add(r.p, x.all() + o, false);
      }
    }
    it++;
  }
  num_iterations = it;
  final_rel_res = rel;
  return 0;
}

}  // namespace mi
