// Solver objects behind the opaque HYPRE_Solver handle.
#pragma once
#include "amg.hpp"

namespace mi {

struct SolverBase {
  enum Kind { K_GMRES, K_BICGSTAB, K_PCG, K_AMG, K_ILU, K_FSAI } kind;
  explicit SolverBase(Kind k) : kind(k) {}
  virtual ~SolverBase() {}
};

// HYPRE_PtrToParSolverFcn: int f(HYPRE_Solver, HYPRE_ParCSRMatrix, HYPRE_ParVector, HYPRE_ParVector)
typedef int (*ParSolverFcn)(void *, void *, void *, void *);

struct AmgSolver : SolverBase {
  BoomerAMG amg;
  CycleTrace last_trace;  // the records of the last HYPRE_MI_BoomerAMGTraceCycle (test hook)
  AmgSolver() : SolverBase(K_AMG) {}
};

struct KrylovSolver : SolverBase {
  double tol = 1e-6, atol = 0.0;
  int max_iter = 1000, min_iter = 0, k_dim = 5, print_level = 0, logging = 0;
  ParSolverFcn precond_solve = nullptr, precond_setup = nullptr;
  void run_precond_setup(ParCSR &A, ParVector &b, ParVector &x);
  void *precond_data = nullptr;
  int num_iterations = 0;
  double rel_residual_norm = 0.0;
  bool converged = false;
  std::vector<double> norms;  // residual history (iteration 0 = initial)
  double solve_seconds = 0.0;
  explicit KrylovSolver(Kind k) : SolverBase(k) {}
  void apply_precond(ParCSR &A, ParVector &rhs, ParVector &out);
  // matvec on every component of a multivector (krylov.cpp)
  void matvec_all(ParCSR &A, double alpha, const double *x, double beta, const double *b, double *y, int nloc, int ncomp,
                  int prof);
  // the BoomerAMG behind precond_solve when the Krylov loop may run in its level-0 ordering (krylov.cpp)
  BoomerAMG *amg_in_level_order(ParCSR &A, int n) const;
  // the loop's view of the system: the caller's objects, or (fast path) the level-0 operator of the AMG with
  // b and x permuted into bp / xp; leave_level_order scatters xp back into the caller's x
  ParVector bp, xp;
  BoomerAMG *enter_level_order(ParCSR &A_in, ParVector &b_in, ParVector &x_in, ParCSR *&A, ParVector *&b, ParVector *&x);
  void leave_level_order(BoomerAMG *amg, ParVector &x_in);
  // out = M^-1 rhs; returns where the result lives (the AMG's own level vector on the fast path unless a copy
  // into `out` is asked for)
  const double *precond_in_order(BoomerAMG *amg, ParCSR &A, ParVector &rhs, ParVector &out, bool need_copy);
};

// GMRES / COGMRES behind a level-ordered BoomerAMG keep z_j = M^-1 p_j and update x from them (krylov.cpp; the
// switch, and a test hook: the allocation of kept vector number `at` and beyond counts as failed, -1 = never)
bool &gmres_keep_directions();
int &gmres_keep_fail_at();
// How GMRES, COGMRES and FlexGMRES store their Krylov basis (MI_HYPRE_BASIS_STORAGE / HYPRE_MI_SetKrylovBasisStorage;
// DESIGN.md section 3): 0 fp64; 1 float; 2 fp64 vectors holding the float-rounded values (mode 1's reference).
// Process-wide, read at the start of a solve; one rank only.
int &krylov_basis_storage();

struct GmresSolver : KrylovSolver {
  std::vector<std::unique_ptr<ParVector>> p;
  // FlexGMRES (krylov/flexgmres.c): the preconditioned directions z_j = M^-1 p_j are kept and the
  // update is x += sum y_j z_j (no extra preconditioner call); the restart residual is recomputed
  bool flexible = false;
  // orthogonalisation: 0 modified Gram-Schmidt (GMRES, FlexGMRES); 1 / 2 = classical Gram-Schmidt with one /
  // two passes, every pass one block of inner products (ONE all-reduce) and one block update (COGMRES,
  // krylov/cogmres.c; src/HypreSystem.cpp:372-388)
  int ortho = 0;
  // also the kept directions of GMRES / COGMRES in level order; those of one component own what was a level-0
  // solution buffer of the preconditioner (same size, swapped in after the cycle)
  std::vector<std::unique_ptr<ParVector>> z;
  ParVector r, w;
  // basis storage mode 1: the basis vectors as floats (p stays empty), and the two fp64 work vectors that rotate --
  // one holds p_{i-1} widened (the preconditioner's right-hand side), the other receives A z, is orthogonalised in
  // place and scaled into the next float slot.  basis_mode: the mode the vectors held were made under
  std::vector<DVec<float>> p32;
  ParVector work[2];
  int basis_mode = 0;
  // a basis of another shape or another storage mode is dropped (Setup and Solve)
  void keep_or_drop_basis(const ParVector &b);
  // blocked MGS (one rank, ortho 0): row i = the raw Gram row of p_i, k::MGS_NB + 1 doubles
  // written by the pass that made p_i; after the k_dim + 1 rows, two alternating sets of k::MGS_NB + 1 raw inner products
  DVec<double> mgs_gram;
  GmresSolver() : KrylovSolver(K_GMRES) {}
  void setup(ParCSR &A, ParVector &b, ParVector &x);
  int solve(ParCSR &A, ParVector &b, ParVector &x);
};

struct BicgstabSolver : KrylovSolver {
  ParVector r0, r, pv, v, q, sv, t;
  BicgstabSolver() : KrylovSolver(K_BICGSTAB) {}
  void setup(ParCSR &A, ParVector &b, ParVector &x);
  int solve(ParCSR &A, ParVector &b, ParVector &x);
};

// preconditioned conjugate gradients (krylov/pcg.c; src/HypreSystem.cpp:440-455)
struct PcgSolver : KrylovSolver {
  ParVector r, pv, sv;
  int two_norm = 0;
  PcgSolver() : KrylovSolver(K_PCG) {}
  void setup(ParCSR &A, ParVector &b, ParVector &x);
  int solve(ParCSR &A, ParVector &b, ParVector &x);
};

// HYPRE_ILU, type 0 (block Jacobi) with level of fill 0: ILU(0) of this rank's diagonal block, factorised and
// applied on the device by level sets (src/HypreSystem.cpp:328-370 as preconditioner, :457-497 as solver).
// tri_solve 1: exact substitutions (one launch per level set); 0: lower/upper Jacobi sweeps (HYPRE's GPU option)
// iter_type 1-4 (fill 0 only): the factors come from fixed-point sweeps instead of the level-scheduled factorisation
// ("Iterative ILU(0) setup"); with tri_solve 0 no level set is computed then
struct IluSolver : SolverBase {
  int ilu_type = 0, level_of_fill = 0, max_iter = 20, print_level = 0, tri_solve = 1, lower_it = 5, upper_it = 5;
  double tol = 1e-7;
  // iterative setup: algorithm type (0 = exact), option bits, sweep limit, tolerance of the correction (option bit 2)
  int iter_type = 0, iter_option = 0, iter_max_iter = 100;
  double iter_tol = 1e-3;
  // what the last iterative setup did on this rank: sweeps run, the last correction / residual norm (-1: never
  // computed), and their histories (option bit 16)
  int iter_sweeps = 0;
  double iter_correction = -1.0, iter_residual = -1.0;
  std::vector<double> iter_corr_hist, iter_res_hist;
  // local reordering (HYPRE_ILUSetLocalReordering): 2 = multicolour ordering of the diagonal block (DESIGN.md section 3;
  // this library's own number); every other value factorises in the caller's ordering
  int reordering = 0;
  // what the last setup did: the reordering in force (0 or 2), colours and colouring rounds (0 without the ordering),
  // level sets of the lower and of the upper factor (0 when no level sets were built)
  int ordering_info[5] = {0, 0, 0, 0, 0};
  DVec<int> perm, colour;    // reordering 2: row q of the factorised block B = P D P^T is the caller's row perm[q]
  std::vector<int> perm_h;   // perm on the host (empty without the ordering): refusals name the caller's row
  DVec<double> xp;           // reordering 2: the result of the substitutions in B's numbering
  bool is_setup = false, levels_built = false;
  int n = 0;
  sk::DCsr LU;
  DVec<long long> dpos;
  DVec<int> order_l, order_u;            // rows sorted by level set
  std::vector<int> lptr, uptr;           // level set boundaries in order_l / order_u
  DVec<double> y, t, r, z;
  DVec<double> rall;  // residuals of all components of a multivector solve with a tolerance (on first use)
  int num_iterations = 0;
  double final_rel_res = 0.0;
  IluSolver() : SolverBase(K_ILU) {}
  // every rank of comm calls it (both setups agree on failures over comm; the iterative one also reports over it).
  // A row without a stored diagonal or an exactly zero pivot u_jj ends it with an error that names the row.
  void setup(ParCSR &A, Comm &comm);
  void iterative_factor(Comm &comm, long long row0);
  void multicolour_order(const HostCSR &D, HostCSR &B);  // reordering 2: colour, perm, ordering_info[0..2]; B = P D P^T
  void apply(const double *rhs, double *out);           // out = U^-1 L^-1 rhs (reordering 2: P^T U^-1 L^-1 P rhs)
  int solve(ParCSR &A, ParVector &b, ParVector &x);     // x += M^-1 (b - A x), max_iter times or to tol
};

// HYPRE_FSAI.  Algo type 3, the static pattern: G lower triangular on the lower triangle of
// the k-th power (k = num_levels) of the threshold-filtered graph of this rank's diagonal block, one dense local solve
// per row.  Algo type 4, the adaptive pattern: every row grows its own pattern from the Kaporin gradient (max_steps
// steps of max_step_size columns, stopped by kap_tolerance).  One step is x += omega G^T G (b - A x).  Also the
// complex smoother smooth_type 4 of BoomerAMG.
struct FsaiSolver : SolverBase {
  int algo_type = 3, num_levels = 1, eig_max_iters = 5, max_iter = 20, print_level = 0;
  double threshold = 0.01, tol = 1e-6;
  int max_steps = 3, max_step_size = 5;  // algo type 4 only
  double kap_tolerance = 1e-3;
  // how G was built (HYPRE_MI_FSAIGetSetupInfo): 0 built, largest row, largest candidate count, rows that took the
  // global-memory table, rows stopped by the tolerance / for want of candidates / by max_steps, -1 (type 3: the
  // adaptive entries are 0)
  int setup_info[8] = {0, 0, 0, 0, 0, 0, 0, -1};
  double omega_user = 0.0;  // > 0: HYPRE_FSAISetOmega, no eigenvalue estimate
  bool zero_guess = false;
  bool is_setup = false;
  int n = 0, max_row = 0;
  double omega = 1.0;
  DevCSR G, Gt;
  DVec<double> t, r;
  HostCSR hG;  // host copy of G for the inspection API (on first use)
  bool host_G_ok = false;
  int num_iterations = 0;
  double final_rel_res = 0.0;
  FsaiSolver() : SolverBase(K_FSAI) {}
  void setup(ParCSR &A, Comm &comm, const std::string &where);
  // the adaptive parameters a Setup refuses: max_steps < 1, max_step_size < 1, max_steps * max_step_size + 1 > 64,
  // kap_tolerance negative or not finite
  static void check_adaptive(const std::string &where, int max_steps, int max_step_size, double kap_tolerance);
  // u += omega G^T G res (zero: u = omega G^T G res): two launches, the update fused into the G^T product
  void apply_add(const double *res, double *u, bool zero, int prof = -1);
  int solve(ParCSR &A, ParVector &b, ParVector &x);  // x += omega G^T G (b - A x), max_iter times or to tol
  const HostCSR &host_G();
};

// the complex smoother of a level, by kind (null when the level has none or one of the other kind)
inline IluSolver *level_ilu(const AmgLevel &Lv) {
  return (Lv.smoother && Lv.smoother->kind == SolverBase::K_ILU) ? static_cast<IluSolver *>(Lv.smoother.get()) : nullptr;
}
inline FsaiSolver *level_fsai(const AmgLevel &Lv) {
  return (Lv.smoother && Lv.smoother->kind == SolverBase::K_FSAI) ? static_cast<FsaiSolver *>(Lv.smoother.get()) : nullptr;
}

}  // namespace mi
