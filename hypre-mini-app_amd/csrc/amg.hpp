// BoomerAMG-shaped preconditioner/solver object: parameters, hierarchy, V-cycle.
#pragma once
#include "parcsr.hpp"
#include "setup_kernels.hpp"

namespace mi {

struct AmgParams {
  int print_level = 0;
  int debug_flag = 0;
  int coarsen_type = 10;          // library default HMIS; the app sets 8 (HypreSystem.cpp:126)
  int interp_type = 6;            // extended+i
  double strong_threshold = 0.25; // the app sets 0.57 (HypreSystem.cpp:159)
  double max_row_sum = 0.9;
  // unknown-based systems AMG ("Systems of PDEs"): the rows belong to num_functions unknowns;
  // strength, splitting and interpolation of every level are those of the same-function operator.  1 = a scalar problem
  int num_functions = 1;
  // restriction: 0 = P^T, 1 = distance-1 approximate ideal restriction with its own strength
  // threshold theta_R and the filter phi of its rows (HYPRE_BoomerAMGSetRestriction / StrongThresholdR / FilterThresholdR)
  int restriction = 0;
  double strong_threshold_r = 0.25, filter_threshold_r = 0.0;
  double trunc_factor = 0.0;
  int pmax_elmts = 4;
  int max_levels = 25;
  int max_coarse_size = 9;
  int min_coarse_size = 0;
  int relax_type[3] = {13, 14, 9};  // down, up, coarsest
  int num_sweeps[3] = {1, 1, 1};
  int relax_order = 0;
  double relax_weight = 1.0;
  double outer_weight = 1.0;
  int cycle_type = 1;
  int max_iter = 20;
  double tol = 1e-7;
  int gs_chunk = 0;  // 0 => runtime default (ctx().gs_chunk)
  int agg_num_levels = 0, agg_interp_type = 4, agg_pmax_elmts = 0, keep_transpose = 0, rap2 = 0;
  double agg_trunc_factor = 0.0;
  // agg_interp_type 5 (two-stage extended interpolation): truncation of the two stage operators P1 and P2; 0 = none
  int agg_p12_max_elmts = 0;
  double agg_p12_trunc_factor = 0.0;
  // test hook (HYPRE_MI_BoomerAMGSetKeepAggMarkers): keep both stage markers of such levels for the inspection getter
  int keep_agg_markers = 0;
  int smooth_num_sweeps = 1;
  // complex smoother on levels < smooth_num_levels (src/HypreSystem.cpp:235-320): 5 = ILU (block-Jacobi ILU(k), the
  // IluSolver behind HYPRE_ILU) and 4 = FSAI (static pattern, the FsaiSolver behind HYPRE_FSAI) are implemented; library
  // defaults as in HYPRE
  int smooth_type = 6, smooth_num_levels = 0;
  int ilu_type = 0, ilu_level = 0, ilu_max_iter = 1, ilu_tri_solve = 1, ilu_lower_it = 5, ilu_upper_it = 5;
  // iterative ILU(0) setup of the ILU smoothers (IluSolver::iter_*; 0 = the exact factorisation)
  int ilu_iter_type = 0, ilu_iter_option = 0, ilu_iter_max_iter = 100;
  double ilu_iter_tol = 1e-3;
  int ilu_reordering = 0;  // IluSolver::reordering of the ILU smoothers: 2 = multicolour ordering, otherwise none
  // smooth_type 4 = FSAI, one step per sweep: algo type 3 = static pattern (num_levels, threshold), 4 = adaptive pattern
  // on the device (max_steps, max_step_size, kap_tolerance; this library's number)
  int fsai_algo_type = 3, fsai_num_levels = 1, fsai_eig_max_iters = 5;
  double fsai_threshold = 0.01;
  int fsai_max_steps = 3, fsai_max_step_size = 5;
  double fsai_kap_tolerance = 1e-3;
  // relax type 16 = Chebyshev: steps per sweep (1 ... 4), where the smoothed interval starts between
  // the eigenvalue bounds of D^-1 A, CG-Lanczos steps of the estimate (0 = Gershgorin); only variant 0 with scale 1 is built
  int cheby_order = 2, cheby_eig_est = 10, cheby_variant = 0, cheby_scale = 1;
  double cheby_fraction = 0.3;
  // non-Galerkin coarse operators (src/HypreSystem.cpp:161-176): drop tolerance for the coarse operator built FROM
  // level l (HYPRE's index): level_tol[l] when set (>= 0), else the global one; 0 = Galerkin
  double non_galerkin_tol = 0.0;
  std::vector<double> non_galerkin_level_tol;
  double non_galerkin_tol_for(int level) const {
    if (level < (int)non_galerkin_level_tol.size() && non_galerkin_level_tol[(size_t)level] >= 0.0)
      return non_galerkin_level_tol[(size_t)level];
    return non_galerkin_tol;
  }
  bool non_galerkin() const {
    if (non_galerkin_tol > 0.0) return true;
    for (double t : non_galerkin_level_tol)
      if (t > 0.0) return true;
    return false;
  }
  // N > 1 ranks: levels >= 1 with at most this many global rows are kept whole on every rank and cycled
  // redundantly, without halo exchanges (HYPRE_BoomerAMGSetSeqThreshold); -1 = MI_HYPRE_REDUNDANT_ROWS or 200000
  long long redundant_rows = -1;
  // value storage of the operators of levels >= value_first_level (HYPRE_MI_BoomerAMGSetValueStorage; DESIGN.md
  // section 3): 0 = fp64, 1 = fp32 stream, 2 = fp64 stream holding the fp32-rounded values.  The public setter takes
  // first_level >= 1; a redundant tail counts its levels from 0 and may hold a smaller number.
  int value_storage = 0, value_first_level = 1;
  // set for a redundant tail, whose print_level is 0: the number of its level 0 in the whole hierarchy, and whether
  // it reports the operators that keep fp64 values
  int value_level_base = 0;
  bool value_report = false;
};

struct SolverBase;

struct AmgLevel {
  ParCSR *A = nullptr;
  // complex smoother of this level on levels < smooth_num_levels: an IluSolver (smooth_type 5) or an FsaiSolver
  // (smooth_type 4); level_ilu / level_fsai (solvers.hpp) give it by kind
  std::shared_ptr<SolverBase> smoother;
  std::unique_ptr<ParCSR> A_own;
  int n = 0;
  HostCSR P, R;  // interpolation / restriction while the hierarchy is being built (moved into Pm / Rm)
  // transfer operators of the finished hierarchy: rectangular ParCSR (rows: this
  // level / next level, columns: next level / this level), diag + halo blocks
  std::unique_ptr<ParCSR> Pm, Rm;
  // device copies (natural ordering) kept between the Galerkin product and the C-first renumbering
  sk::DCsr sA, sP, sR;  // sR: only in the global hierarchy of the replicated setup (sliced on the device)
  // C-first ordered operators of a level built on the device, until setup_device moves them into the
  // solve-phase format (A->d_diag, Pm->d_diag, Rm->d_diag)
  sk::DCsr oA, oP, oR;
  // sub-operator of A for the first sweep on a zero guess (sk::zero_guess_operator): the down leg of every
  // cycle starts from u = 0, where most of A multiplies zeros
  DevCSR Az;
  bool has_Az = false;
  int Az_chunk = 0;  // the hybrid-GS chunk size Az was cut for (its "in-chunk" entries)
  // operator of the residual that follows a zero-guess C-then-F sweep (sk::zero_guess_operator mode 1): the F
  // pass leaves tvec = f - A_FC u_C for the F rows from t_from on (f itself before), so those rows need only
  // their F columns; t_valid: tvec belongs to the current u
  DevCSR Ar;
  bool has_Ar = false, t_valid = false;
  int t_from = 0;
  DVec<double> tvec;
  // C-row hand-over (level 0 of a one-rank hierarchy swept by the tile kernel): the descriptors of
  // the tiles of A->d_diag that the mat-vec after the cycle's last C pass still has to run, and the census they came from
  DVec<int> mv_tdesc;
  sk::HandoverCensus handover;
  // N > 1: rows with halo entries (ascending) and, per swept row range and operator, the largest halo-free
  // stretch, cut at the units the GS kernels write back -- a pass sweeps it while the halo is still travelling
  struct InteriorRange {
    int row_begin, row_end;
    const void *op;
    int ib, ie;
    bool ok;
  };
  std::vector<int> halo_rows;
  bool halo_rows_ready = false;
  std::vector<InteriorRange> interior_cache;
  LazyInts cf;  // +1 C, -1 F (empty on the coarsest level)
  // num_functions > 1: the unknown every row belongs to -- natural order while the hierarchy is built, the level's
  // C-first order afterwards (HYPRE_MI_BoomerAMGGetLevelDofFunc); empty otherwise
  LazyInts dof;
  // aggressive level with the two-stage interpolation (agg_interp_type 5): the markers after the first coarsening and
  // after the second one (+1 C, -1 F, -3 special F), natural order of the level; kept only when
  // AmgParams::keep_agg_markers asks for them (inspection)
  std::vector<signed char> agg_m1, agg_m2;
  // what sk::interp ran for this level's P (HYPRE_MI_BoomerAMGGetInterpCensus); interp_by_host: P came from a host
  // routine or another device routine and the census is all zeros (a level that fell back has census.fell_back)
  sk::InterpCensus interp_census;
  bool interp_by_host = true;
  // how this level's R was made (HYPRE_MI_BoomerAMGGetRestrictionInfo): 0 = the transpose of P, 1 = approximate ideal
  // restriction built by the device, 2 = by the host routine; air_info: what that routine counted
  int restriction_kind = 0;
  sk::AirInfo air_info;
  bool has_cf = false;  // the level has a C/F splitting -- a GLOBAL fact (cf itself is empty on a rank without rows)
  DVec<signed char> d_cf;
  // C-first ordering of this level: perm[new] = old local row;
  // rows [0, nc) are the C points, [nc, n) the F points.  Empty = identity.
  LazyInts perm;
  DVec<int> d_perm;
  int nc = 0;
  std::vector<double> diag, l1gs, l1jac;
  // what apply_value_storage decided for A, P and R of this level: 0 = left as built, else the mode that was applied
  int value_kind[3] = {0, 0, 0};
  DVec<double> d_diag, d_l1gs, d_l1jac;
  DVec<double> u, f, tmp, snap;
  // the same vectors for `cap` components of a multivector, component-major and n apart (batched cycle, DESIGN.md
  // section 5): allocated by the first batched cycle (BoomerAMG::mv_enter), released by Setup.  While a batched cycle
  // runs their storage pointers stand in u / f / tmp / snap / tvec above, and the level's own ones wait here.
  struct MvVectors {
    int cap = 0;
    DVec<double> u, f, tmp, snap, tvec;
  } mv;
  // relax type 16 (Chebyshev), on every level when some relax_type slot is 16 at Setup (BoomerAMG::build_cheby):
  // eigenvalue bounds of D^-1 A, the interval [lower, upper] the polynomial is built for, its centre and half width,
  // and the coefficients (a_k, b_k) of the steps of one sweep
  struct Cheby {
    bool ready = false;
    int eig_est = -1;  // the setting eig_min / eig_max were estimated with
    double eig_min = 0.0, eig_max = 0.0, lower = 0.0, upper = 0.0, theta = 0.0, delta = 0.0;
    int order = 0;
    double a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
  } cheby;
  DVec<double> cheby_d;  // the direction vector d of the sweep (step 0 writes it before any step reads it)
  // relax types 40 / 41 / 42 (multicolour Gauss-Seidel), on every level that is smoothed when some
  // relax_type slot holds one at Setup (BoomerAMG::apply_cf_ordering): the rows of the C block and of the F block are
  // sorted by colour.  range_start: the first rows of the (block, colour) ranges in stored order, and n at the end;
  // range_colour: their colours; ranges_c: how many of them lie in the C block; rounds: launches of the colouring
  struct Colours {
    bool ready = false;
    int colours = 0, rounds = 0, ranges_c = 0;
    std::vector<int> range_start, range_colour;
  } mc;
  DVec<double> ts_work;  // second work vector of the two-stage Gauss-Seidel (relax types 11 / 12), on first use
  // coarsest level dense solve (relax type 9)
  std::vector<double> Cinv_host;
  DVec<double> Cinv;    // n_local x (size*slot) padded inverse rows
  DVec<double> fgather; // size*slot
  DVec<double> fslot;   // slot
  int slot = 0;
  bool dense = false;
};

// Cycle trace (test hook, HYPRE_MI_BoomerAMGTraceCycle): what one cycle left in its vectors after
// each of its steps, copied to the host where the cycle runs them.  BoomerAMG::trace is null outside that hook, and
// every call site is `if (trace) ...`: a solve launches, synchronises and allocates what it did without it.
struct CycleTrace {
  enum Step {
    F_IN = 0,       // the level's right-hand side on entry (for a level > 0: the restricted residual)
    U_IN = 1,       // its guess on entry, when that is not zero
    U_DOWN = 2,     // u after the down sweeps
    RESID = 3,      // r = f - A u (Lv.tmp)
    U_SUB = 4,      // the next level's u after its sub-cycle(s): the correction e
    U_PROLONG = 5,  // u + P e
    U_UP = 6,       // u after the up sweeps
    U_COARSE = 7,   // the coarsest level's u after its solve
    U_COLLAPSED = 8,  // the collapsed level's u = B f
    U_SWEEP = 9     // u after one sweep of relax_sweeps (flags: which and the sweep's number)
  };
  enum Flag {
    COMPOSITE = 1,     // RESID: the mat-vec ran on Ar with tvec / f as its composite right-hand side
    FILL_SKIPPED = 2,  // F_IN: the level's u was not zero-filled before this zero-guess visit
    DENSE = 4,         // U_COARSE: the dense solve ran
    SWEPT = 8,         // U_COARSE: relaxation sweeps ran
    COLLAPSED = 16,    // F_IN / U_COLLAPSED: the visit applied the tabulated map
    ZERO_GUESS = 32,   // F_IN: the visit started from a zero guess
    SWEEP_ZERO = 64    // U_SWEEP: the sweep was told its u is zero
    // U_SWEEP: bits 8-9 = which (0 down, 1 up, 2 coarsest), bits 10.. = the sweep's number
  };
  struct Record {
    int level, visit, step, flags;
    std::vector<double> values;  // mv_n components, the level's n apart
  };
  std::vector<Record> records;
  std::vector<int> visits;    // per level: cycle() entries so far
  bool fill_skipped = false;  // set where the next level's zero-fill is decided, read by that level's F_IN
  bool dense_ran = false;     // set by relax() when the dense solve took the coarsest level
};

struct LevelBuild;  // what build_natural knows about the level it is building (amg_setup.cpp)

struct BoomerAMG {
  AmgParams p;
  std::vector<AmgLevel> L;
  bool is_setup = false, host_ready = false;
  bool host_only = false;  // set up by HYPRE_MI_BoomerAMGSetupHostOnly: nothing that needs the device exists
  // levels with at least this many rows run their sparse products / transposes / renumbering on the
  // device; -1 = everything on host threads (HYPRE_MI_BoomerAMGSetupHostOnly)
  long long device_min_rows = -1;
  bool keep_natural_R = false;  // the replicated multi-rank setup slices A, P and R = P^T in natural ordering:
                                // device-built levels keep them on the device (sA, sP, sR), host-built ones on the host
  double t_setup_start = 0.0;
  double t_phase[6] = {0, 0, 0, 0, 0, 0};  // strength, pmis, interp, galerkin, ordering, host total
  int num_iterations = 0;
  double final_rel_res = 0.0;
  double setup_seconds = 0.0;
  double global_opcx = -1.0;  // N > 1: sum over ranks, taken at the end of the (collective) Setup
  // Internal locality numbering (single rank; amg_setup.cpp locality_order): the hierarchy is built on Q A Q^T,
  // where Q groups rows into graph-compact clusters so that a tile of consecutive rows touches few distinct columns.
  // input_order[new] = caller's row; empty = identity.  Level 0's perm is composed with it, so every solve path
  // gathers / scatters caller vectors as before.
  LazyInts input_order;
  std::unique_ptr<ParCSR> Aq_own;
  sk::DCsr pending_sA0;  // Q A Q^T built on the device by setup_host, handed to level 0 by build_natural
  bool use_locality_order(const ParCSR &A) const;
  // num_functions > 1: the caller's dof_func (host or device memory, read and copied at every Setup, never freed here;
  // null = global row mod num_functions), and level 0's copy in the internal numbering on its way to build_natural
  const int *dof_func_user = nullptr;
  std::vector<int> pending_dof;
  void read_dof_func(const ParCSR &A);
  // the matrix HYPRE_BoomerAMGSetup was called with (and its assembly stamp): a Krylov solver may run on the
  // hierarchy's own level-0 copy only when it is handed that very matrix (krylov.cpp amg_in_level_order)
  const ParCSR *source_matrix = nullptr;
  unsigned long long source_stamp = 0;
  int chunk() const;
  // the communicator this hierarchy works on: the process communicator, or a private single-rank one
  // (global hierarchy of the replicated setup, redundant coarse tail)
  Comm *forced_comm = nullptr;
  std::unique_ptr<Comm> own_comm;
  Comm &my_comm() const { return forced_comm ? *forced_comm : current_comm(); }
  void use_private_self_comm();

  // ---- redundant coarse tail (N > 1): the last entry of L is a stub that only carries this rank's slice of
  // the first redundant level (natural ordering); the level itself and everything below it live in `tail`, a
  // single-rank hierarchy every rank holds and cycles for itself
  std::unique_ptr<BoomerAMG> tail;
  std::unique_ptr<ParCSR> tail_A;   // the first redundant level, global, natural ordering (tail's fine level)
  long long stop_rows = 0;          // build_natural: stop coarsening at the first level >= 1 this small
  bool stopped_by_rows = false;
  int tail_slot = 0;                // max rows of the stub over the ranks (all-gather slot)
  gidx tail_start = 0;              // this rank's first row of the redundant level
  DVec<double> tail_fslot, tail_fgather, tail_f, tail_e;
  std::vector<int> tail_map_host;
  DVec<int> tail_map, tail_pcol;    // natural id -> all-gather position; halo columns of the last P
  void tail_cycle(bool zero_guess);
  // ---- collapsed coarse tail (one rank, or the redundant tail hierarchy of N > 1): a cycle that starts from a zero
  // guess is a LINEAR map f -> u, so for the first level with at most MI_HYPRE_DENSE_TAIL_ROWS (default 1024) rows the
  // map of the whole sub-cycle (that level and everything below it) is tabulated at Setup by cycling the unit
  // vectors, and the cycle multiplies by it: one launch instead of ~9 per level (at 512^3: levels 8-11, 36 of the
  // ~75 latency-bound launches of a cycle).  Same operator, other rounding (1e-16 relative).
  // what the tabulated map depends on besides the operators: the cycle's parameters at tabulation time.  A setter that
  // runs AFTER Setup (relax types, sweeps, weights, cycle type, HYPRE_MI_SetGSChunk, HYPRE_MI_SetZeroGuessMode) changes
  // the cycle of the fine levels at once; cycle(0, ..) compares this signature and tabulates again when it differs
  // (the frozen maps used to keep the old smoother on the coarse levels silently)
  std::vector<double> collapsed_signature;
  std::vector<double> cycle_signature() const;
  int collapsed_level = -1, collapsed_n = 0;
  DVec<double> collapsed_Bt;  // column j of the map = row j here (n x n)
  void build_collapsed_tail();
  void tabulate_cycle(int level, DVec<double> &Bt);
  void apply_global(const double *f, double *e, bool zero_guess);  // one cycle, caller (natural) ordering
  long long effective_redundant_rows() const;
  // levels of the whole hierarchy (the stub counts once, as the tail's fine level) and the owner of one
  int total_levels() const { return (int)L.size() + (tail ? (int)tail->L.size() - 1 : 0); }
  BoomerAMG &owner_of(int level, int &local) {
    const int own = tail ? (int)L.size() - 1 : (int)L.size();
    if (level < own || !tail) {
      local = level;
      return *this;
    }
    local = level - own;
    return *tail;
  }
  static long long default_device_min_rows();

  // ---- setup reuse (HYPRE_MI_BoomerAMGSetSetupReuse; DESIGN.md section 3, "Setup reuse"): with mode 1 a Setup on a
  // handle that holds a finished hierarchy of the same matrix object and pattern, built by the same entry point with
  // the same structural settings, keeps the splittings, orderings, P, R and every pattern and recomputes the values
  int setup_reuse = 0;
  // the verdict of the last Setup: kind 0 never set up, 1 built from scratch, 2 refreshed; reason (kind 1): 0 reuse off,
  // 1 first Setup or the previous one failed, 2 another matrix object or pattern, 3 a structural setting changed, 4 a
  // setting the refresh does not cover, 5 more than one rank, 6 the other entry point built the hierarchy
  int setup_kind = 0, setup_reason = 0;
  bool built_ok = false, built_host_only = false;  // a finished hierarchy, and the entry point that built it
  const ParCSR *built_matrix = nullptr;
  unsigned long long built_pattern = 0;
  // everything the structure depends on, at the last build
  std::vector<double> structure_signature;
  std::vector<double> current_structure_signature(const ParCSR &A) const;
  int refresh_verdict(const ParCSR &A, bool entry_host_only) const;  // -1: refresh; else the reason of the rebuild
  // both entry points: refresh or rebuild, verdict, counters, print
  void setup_entry(ParCSR &A, bool entry_host_only);
  void validate_settings() const;  // the settings a Setup refuses, checked before a build and before a refresh
  void build_from_scratch(ParCSR &A, bool entry_host_only);
  void refresh(ParCSR &A);
  void refresh_level0(ParCSR &A);
  void refresh_coarse_operator(int level, double *seconds);  // A_{level+1} from A, P, R of `level`
  void refresh_norms_and_sub_operators(int level);
  void build_coarsest_inverse();  // relax type 9: dense inverse of the coarsest level (host)
  void upload_coarsest_inverse();

  void setup(ParCSR &A) { setup_entry(A, false); }
  // hierarchy construction: host only (threads + host collectives)
  void setup_host(ParCSR &A);
  void build_natural(ParCSR &A);      // strength / PMIS / interpolation / Galerkin loop, natural ordering
  // its steps on the state of the level being built (amg_setup.cpp; DESIGN.md section 3, "The level build")
  void level_same_function_operator(LevelBuild &b);
  void level_strength_and_coarsening(LevelBuild &b);
  void level_interpolation(LevelBuild &b);
  void level_restriction(LevelBuild &b);
  void level_galerkin_and_adopt(LevelBuild &b);
  void build_replicated(ParCSR &A);   // N > 1: global hierarchy on every rank, then this rank's row slices
  // N > 1: the same hierarchy built with O(N_global / P) per rank (amg_setup_dist.cpp); PMIS without aggressive
  // levels (the Ruge-Stueben family is sequential on the global graph: replicated path)
  void build_distributed(ParCSR &A);
  bool can_build_distributed() const;
  void make_local_transfer_operators();
  void finish_host();                 // l1 norms, coarsest-level dense inverse
  // device mirror of the hierarchy (needs a GPU)
  void setup_device();
  // p.value_storage: round (mode 2) or narrow (mode 1) the operator values of this hierarchy's levels >=
  // p.value_first_level, host arrays and -- with on_device -- the placed device operators; the last step of a setup
  void apply_value_storage(bool on_device);
  // HYPRE_BoomerAMGSolve: x is the initial guess; up to max_iter cycles
  void solve(ParCSR &A, ParVector &b, ParVector &x);

  // pieces (exposed for the parity tests).  Each level works on its own vectors
  // Lv.u / Lv.f in the level's C-first ordering.
  // u_is_zero: the caller guarantees Lv.u == 0 on entry (its halo is then known to be zero)
  void relax(int level, int type, int points, const double *f, bool u_is_zero = false);
  // wout (C-row hand-over): the C pass that ends an F-then-C pair on the tile kernel also stores (A u)_i for the C rows
  // whose only C column is their diagonal, and raises handover_done; relax_sweeps hands it to its last pair
  void relax_pair(int level, int type, int first, const double *f, bool u_is_zero = false, double *wout = nullptr);
  void relax_sweeps(int level, int which, const double *f, bool u_is_zero = false, double *wout = nullptr);
  // C-row hand-over: a Krylov loop in level order sets the vector that will take A z before it asks for the cycle that
  // computes z; cycle(0, ..) clears handover_done and raises it when the last level-0 launch was such a C pass.  Then
  // rows of handed-over tiles of L[0] hold (A z)_i and the mat-vec runs on L[0].mv_tdesc alone.
  double *handover_w = nullptr;
  bool handover_done = false;
  bool handover_wanted() const;  // the mode and level 0's census allow it
  // host-side census of the tile Gauss-Seidel kernel's sweep branches for one pass of relax / relax_pair
  bool gs_sweep_paths(int level, int points, bool u_is_zero, long long counts[5]);
  void cycle(int level, bool u_is_zero = false);
  // the recorder of the cycle trace (test hook): null but inside trace_cycle.  trace_step waits for the stream and copies
  // the level's mv_n * n values at `dev` to the host
  CycleTrace *trace = nullptr;
  void trace_step(int level, int step, const double *dev, int flags);
  // one cycle(level, u0 == null) on host arrays of nvec * n values in the level's ordering, every step recorded in `out`;
  // nvec 2..4: inside mv_enter / mv_leave; collapse false: the collapsed level cycles like any other.  One rank, no tail.
  void trace_cycle(int level, const double *f_host, const double *u0_host, int nvec, bool collapse, CycleTrace &out);
  // what cycle(0, ..) refreshes first: smoothers, Chebyshev data and the collapsed tail after a setting changed
  void refresh_before_cycle();
  // ---- batched cycle on the components of a multivector (one rank).  mv_n > 1: every level's
  // u / f / tmp / snap / tvec hold mv_n components, n apart, and relax / relax_pair / relax_sweeps / cycle work on all of
  // them -- the mat-vecs and the hybrid Gauss-Seidel passes through k::spmv_multi / k::gs_hybrid_multi, which sweep the
  // operator once for up to k::multivector_batch() components; every component gets the bits of the one-vector cycle.
  int mv_n = 1;
  // whether this hierarchy's cycle can work on a batch: one rank without a redundant tail, no complex smoother, down /
  // up relax types of the hybrid-GS family (3, 4, 6, 8, 13, 14), coarsest type 9 or of that family.  The one place
  // that decides; everything else cycles component by component
  bool mv_cycle_eligible();
  // components per pass of a multivector with ncomp components: min(ncomp, k::multivector_batch()), or 1 when the
  // cycle is not eligible; counts the pass under "mv_batched_cycles" / "mv_fallback_cycles" per group it will run
  int mv_cycle_width(int ncomp);
  void mv_enter(int nvec);  // nvec <= k::MV_MAX_BATCH
  void mv_leave();
  struct MvScope {
    BoomerAMG &amg;
    const bool on;
    MvScope(BoomerAMG &a, int nvec) : amg(a), on(nvec > 1) {
      if (on) amg.mv_enter(nvec);
    }
    ~MvScope() {
      if (on) amg.mv_leave();
    }
  };
  // complex smoothers of the levels < p.smooth_num_levels (end of setup_device); fsai_signature: the FSAI and
  // iterative-ILU parameters they were built with -- a change after Setup rebuilds them before the next cycle
  void build_smoothers();
  std::vector<double> fsai_signature;
  std::vector<double> current_fsai_signature() const;
  // Chebyshev data of every level (relax type 16 in some slot; end of build_smoothers): the eigenvalue estimate is
  // collective and runs on the device.  cheby_signature: the parameters the data was built with -- a change after Setup
  // rebuilds it before the next cycle or sweep (the bounds are estimated again only when cheby_eig_est changed)
  void build_cheby();
  bool wants_cheby() const { return p.relax_type[0] == 16 || p.relax_type[1] == 16 || p.relax_type[2] == 16; }
  std::vector<double> cheby_signature;
  std::vector<double> current_cheby_signature() const;
  // relax types 40 / 41 / 42 in some slot: Setup colours the levels and sorts their rows by (block, colour)
  static bool is_mcgs(int type) { return type >= 40 && type <= 42; }
  bool wants_mcgs() const { return is_mcgs(p.relax_type[0]) || is_mcgs(p.relax_type[1]) || is_mcgs(p.relax_type[2]); }
  void refresh_cheby();
  // cycle(level, true) never reads Lv.u before it has overwritten every row (one rank, Gauss-Seidel down sweep on
  // the zero-skipping kernels, or the dense coarsest solve): the caller need not zero-fill u first -- at 512^3 the
  // fills of a cycle are 1.6 GB of writes, 0.8 % of the solve, and one launch per level
  bool zero_cycle_ignores_u(int level);
  // renumber every level C-first (host, collective); called at the end of setup_host
  void apply_cf_ordering();
  double operator_complexity() const;
  void local_entry_counts(double &tot, double &base) const;  // this rank's share (redundant levels: 1 / size of them)
  // fill the host arrays of a level's A / P / R from the device (inspection API, coarse solve)
  void ensure_host(int level);
  // one operator: host_diag_stale -> download from `dev` (or from the solve format) -> ensure_offd_rows
  static void fetch_operator(ParCSR *M, sk::DCsr &dev);
};

// MI_HYPRE_GS_ZERO_SKIP: 0 = sweeps on a zero guess read like any other sweep, 1 = they skip the gathers of
// known zeros, 2 = they also run on the zero-guess sub-operator (AmgLevel::Az), 3 (default) = and the residual
// that follows reuses the F pass's product with the C values (AmgLevel::Ar)
int zero_skip_mode();
void set_zero_skip_mode(int mode);  // applies to hierarchies set up afterwards (mode 2) / to every later sweep (0, 1)
// MI_HYPRE_C_HANDOVER: 0 = the mat-vec after a cycle is always the full one, 1 (default) = C-row hand-over when at least
// 10 % of level 0's tiles are handed over, 2 = whenever one is
int c_handover_mode();
void set_c_handover_mode(int mode);

// set by a Krylov solver right before it calls the preconditioner with x == 0,
// consumed (and cleared) by BoomerAMG::solve
bool &zero_guess_hint();

// counters of the distributed setup (HYPRE_MI_GetCounter): largest per-rank extended sub-problem (rows), global rows
// gathered on every rank (the redundant tail only), number of distributed setups; -1 = unknown name
long long dist_setup_counter(const char *name);
void dist_setup_counters_reset();
// Setups of this process that built from scratch / refreshed ("amg_setups_full", "amg_setups_refreshed"); -1 = unknown name
long long setup_reuse_counter(const char *name);
// the reason of a rebuild in words (HYPRE_MI_BoomerAMGGetSetupKind's reasons 0 ... 6; HYPRE_MI_SetupReuseReasonText)
const char *setup_reuse_reason_text(int reason);

// host algorithms (amg_setup.cpp), exposed for tests
void host_transpose(const HostCSR &A, HostCSR &T);
void host_spgemm(const HostCSR &A, const HostCSR &B, HostCSR &C);

}  // namespace mi
