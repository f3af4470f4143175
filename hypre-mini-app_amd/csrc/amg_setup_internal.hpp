// Host setup algorithms of amg_setup.cpp that the distributed setup (amg_setup_dist.cpp) runs on its
// per-rank extended sub-problems.  Not part of any ABI.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

#include "amg.hpp"

namespace mi {
namespace hs {

constexpr int C_PT = 1, F_PT = -1, SF_PT = -3;

// strength pattern of the diag block (columns ascending, a subsequence of the matrix row)
struct Strength {
  std::vector<int64_t> ia;
  std::vector<int> ja;
};

void strength(const ParCSR &A, double theta, double max_row_sum, Strength &S);

// the same-function operator F(A) of a square block (num_functions > 1; DESIGN.md section 3, "Systems of PDEs"): row i
// keeps the entries a_ij with dof[j] == dof[i] and its diagonal, in stored order -- the host twin of
// sk::same_function_filter
void filter_same_function(const HostCSR &A, const std::vector<int> &dof, HostCSR &F);

// The strength rule of ONE row (par_strength.c), stated once for the single-rank and the distributed setup: `a` = the
// row's values, dpos = position of the diagonal among them (-1: none), `more` = further off-diagonal values that only
// count for the row sum and the row scale (the halo block of a rank-local operator).  An entry v off the diagonal is
// strong iff v < theta * min_k a_ik (a_ii >= 0; mirrored, v > theta * max_k a_ik, for a_ii < 0), and no entry is when
// |row sum| > max_row_sum * |a_ii|.
struct StrengthRule {
  bool all_weak = true, neg = false;
  double thr = 0.0;
  bool operator()(double v) const { return !all_weak && (neg ? v > thr : v < thr); }
};
inline StrengthRule strength_rule(const double *a, int64_t len, int64_t dpos, double theta, double max_row_sum,
                                  const double *more = nullptr, int64_t nmore = 0) {
  StrengthRule r;
  const double diag = dpos >= 0 ? a[dpos] : 0.0;
  double row_sum = 0.0, scale = 0.0;
  r.neg = diag < 0;
  auto upd = [&](double v) {
    if (r.neg ? v > scale : v < scale) scale = v;
  };
  for (int64_t k = 0; k < len; k++) {
    row_sum += a[k];
    if (k != dpos) upd(a[k]);
  }
  for (int64_t k = 0; k < nmore; k++) {
    row_sum += more[k];
    upd(more[k]);
  }
  r.all_weak = (std::fabs(row_sum) > std::fabs(diag) * max_row_sum) && (max_row_sum < 1.0);
  r.thr = theta * scale;
  return r;
}

// ---- three idioms of the host builders, stated once --------------------------------------------------------------
// coarse numbering: f2c[i] = the rank of C point i among the C points of the marker, -1 elsewhere; returns their number
inline int coarse_numbering(const std::vector<int> &marker, std::vector<int> &f2c) {
  f2c.assign(marker.size(), -1);
  int nc = 0;
  for (size_t i = 0; i < marker.size(); i++)
    if (marker[i] == C_PT) f2c[i] = nc++;
  return nc;
}

// Row i of D against S_i, which is a subsequence of the row's ascending columns: f(q, j, strong) for every stored entry
// q with column j, in stored order (the diagonal and the weak entries come with strong = false)
template <class F>
inline void for_each_entry_strong(const HostCSR &D, const Strength &S, int64_t i, F &&f) {
  int64_t ks = S.ia[(size_t)i];
  const int64_t kse = S.ia[(size_t)i + 1];
  for (int64_t q = D.ia[(size_t)i]; q < D.ia[(size_t)i + 1]; q++) {
    const int j = D.ja[(size_t)q];
    while (ks < kse && S.ja[(size_t)ks] < j) ks++;
    f(q, j, ks < kse && S.ja[(size_t)ks] == j);
  }
}
// the strong entries alone, f(q, j): the walk ends with S_i
template <class F>
inline void for_each_strong_entry(const HostCSR &D, const Strength &S, int64_t i, F &&f) {
  int64_t ks = S.ia[(size_t)i];
  const int64_t kse = S.ia[(size_t)i + 1];
  for (int64_t q = D.ia[(size_t)i]; q < D.ia[(size_t)i + 1] && ks < kse; q++) {
    const int j = D.ja[(size_t)q];
    while (ks < kse && S.ja[(size_t)ks] < j) ks++;
    if (ks < kse && S.ja[(size_t)ks] == j) f(q, j);
  }
}

// Rows that a parallel_for builds, collected per thread: a thread takes its part with begin(t, b), appends the entries of
// its rows [b, e) in row order to part.j (and part.a) and notes each row's length in len; assemble() lays the rows out by
// a prefix sum and one block copy per thread.  Col: int, or gidx in the distributed setup.
template <class Col>
struct RowCollector {
  struct Part {
    std::vector<Col> j;
    std::vector<double> a;
    int64_t first = -1;  // the thread's first row
  };
  std::vector<Part> part;
  std::vector<int> len;
  explicit RowCollector(int64_t nrows) : part((size_t)host_threads()), len((size_t)nrows, 0) {}
  Part &begin(int t, int64_t first_row) {
    part[(size_t)t].first = first_row;
    return part[(size_t)t];
  }
  // ia[0] is the caller's: 0, or the end of what ja (and a) hold already -- the rows are appended there
  void assemble(std::vector<int64_t> &ia, std::vector<Col> &ja, std::vector<double> *a = nullptr) const {
    const size_t n = len.size();
    ia.resize(n + 1);
    for (size_t i = 0; i < n; i++) ia[i + 1] = ia[i] + len[i];
    ja.resize((size_t)ia[n]);
    if (a) a->resize((size_t)ia[n]);
    for (const Part &p : part) {
      if (p.first < 0 || p.j.empty()) continue;
      memcpy(ja.data() + ia[(size_t)p.first], p.j.data(), p.j.size() * sizeof(Col));
      if (a) memcpy(a->data() + ia[(size_t)p.first], p.a.data(), p.a.size() * sizeof(double));
    }
  }
};

// interpolation rows of the single-rank operator A (diag block).  want_rows (optional): rows with a zero flag
// are left empty and the special-F markers of cf are kept (the caller owns them)
void build_interp(const ParCSR &A, const Strength &S, std::vector<int> &cf, int interp_type, double trunc_factor,
                  int pmax, HostCSR &P, int &nc_out, const std::vector<char> *want_rows = nullptr);

// distance-1 approximate ideal restriction (restriction 1) of a square block D with the final marker cf: -1, or the
// smallest C row with a singular local system (R is then not built); neighbourhoods of any size
int build_air_restriction(const HostCSR &D, const std::vector<int> &cf, double theta_r, double phi, HostCSR &R,
                          sk::AirInfo &info);
// FSAI with the adaptive pattern (fsai_algo_type 4) of a square block B, on the host threads: 0, or 2 when a row fails
// (info.bad_row = the smallest such row, info.bad_kind; G is then not built) -- bit for bit sk::fsai_adaptive
int build_fsai_adaptive(const HostCSR &B, int max_steps, int max_step_size, double kap_tolerance, HostCSR &G,
                        sk::FsaiAdaptiveInfo &info);
// one-point interpolation (interp_type 100); cf is handed on with special F -> F
void build_one_point_interp(const HostCSR &D, const Strength &S, std::vector<int> &cf, HostCSR &P, int &nc_out);

// classical Ruge-Stueben coarsening of a graph (first pass; second_pass: strong F-F pairs must share a C point)
void ruge_stueben(int n, const Strength &S, bool second_pass, std::vector<int> &cf);
// truncation of one interpolation row in place (trunc_factor, pmax; rescaled to the row sum, stored order kept): new length
int truncate_row(int len, int *cols, double *vals, double trunc_factor, int pmax, std::vector<char> &keep);

// Non-Galerkin drop-and-lump on the rows [row0, row0 + n) of an operator whose columns are ids of type Col (local
// int ids on one rank, global ids in the distributed setup); the rule is stated at sparsify_non_galerkin (amg_setup.cpp).
// m_i = max_{j != i} |a_ij| of the own rows; the caller fetches what it needs of the other rows before it drops.
template <class Col>
std::vector<double> offdiag_row_maxima(int n, const std::vector<int64_t> &ia, const std::vector<Col> &ja, const std::vector<double> &a,
                                       Col row0) {
  std::vector<double> m((size_t)n, 0.0);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      double mx = 0.0;
      for (int64_t k = ia[(size_t)i]; k < ia[(size_t)i + 1]; k++)
        if (ja[(size_t)k] != row0 + i && std::fabs(a[(size_t)k]) > mx) mx = std::fabs(a[(size_t)k]);
      m[(size_t)i] = mx;
    }
  });
  return m;
}
// m = offdiag_row_maxima of these rows, m_of(j) = the maximum of the row of column j (own or not)
template <class Col, class MJ>
void drop_and_lump(int n, std::vector<int64_t> &ia, std::vector<Col> &ja, std::vector<double> &a, Col row0, const std::vector<double> &m,
                   MJ m_of, double tol) {
  auto keeps = [&](int64_t i, int64_t k) {
    const Col j = ja[(size_t)k];
    const double lim = tol * std::min(m[(size_t)i], m_of(j));
    return j == row0 + i || !(std::fabs(a[(size_t)k]) < lim);
  };
  std::vector<int64_t> bia((size_t)n + 1, 0);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      int64_t c = 0;
      for (int64_t k = ia[(size_t)i]; k < ia[(size_t)i + 1]; k++) c += keeps(i, k) ? 1 : 0;
      bia[(size_t)i + 1] = c;
    }
  });
  for (int i = 0; i < n; i++) bia[(size_t)i + 1] += bia[(size_t)i];
  std::vector<Col> bja((size_t)bia[(size_t)n]);
  std::vector<double> ba((size_t)bia[(size_t)n]);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      int64_t w = bia[(size_t)i], dpos = -1;
      double lump = 0.0;
      bool first = true;
      for (int64_t k = ia[(size_t)i]; k < ia[(size_t)i + 1]; k++) {
        if (keeps(i, k)) {
          if (ja[(size_t)k] == row0 + i) dpos = w;
          bja[(size_t)w] = ja[(size_t)k];
          ba[(size_t)w++] = a[(size_t)k];
        } else {
          lump = first ? a[(size_t)k] : lump + a[(size_t)k];
          first = false;
        }
      }
      if (!first && dpos >= 0) ba[(size_t)dpos] = ba[(size_t)dpos] + lump;
    }
  });
  ia.swap(bia), ja.swap(bja), a.swap(ba);
}
// non-Galerkin sparsification of a square single-rank operator, in place (amg_setup.cpp)
void sparsify_non_galerkin(HostCSR &A, double tol);

// ---- the coarsening core: PMIS and CLJP, stated once -------------------------------------------------------------
// hypre_SeedRand / hypre_Rand (Park-Miller minimal standard)
struct ParkMiller {
  int seed;
  explicit ParkMiller(int s) : seed(s ? s : 13579) {}
  double next() {
    const int a = 16807, m = 2147483647, q = 127773, r = 2836;
    const int lo = seed % q, hi = seed / q;
    const int t = a * lo - r * hi;
    seed = (t > 0) ? t : t + m;
    return (double)seed / m;
  }
};
// the stream of ParkMiller(seed) after `skipped` draws: state seed * 16807^skipped mod (2^31 - 1)
inline ParkMiller park_miller_at(int seed, long long skipped) {
  const unsigned long long m = 2147483647ULL;
  unsigned long long base = 16807ULL, acc = (unsigned long long)ParkMiller(seed).seed % m;
  for (unsigned long long e = (unsigned long long)skipped; e; e >>= 1) {
    if (e & 1ULL) acc = (acc * base) % m;
    base = (base * base) % m;
  }
  return ParkMiller((int)acc);
}

// The algorithms below run on a GRAPH VIEW G with two implementations: LocalGraph (amg_setup.cpp: a Strength pattern
// on one rank -- int columns, no halo, no communicator, every exchange an empty inline function) and DistGraph
// (amg_setup_dist.cpp: this rank's rows with global column ids, per-entry strength flags and halo slots, a Ring).
//   n(), nh(), nnz()            rows, halo points, entries (the index space of k below)
//   first_id()                  global id of row 0: the index into the one global random stream
//   each(i, f)                  the strong entries of row i as f(k, j, h): entry k, neighbour = own row j (h < 0) or halo
//                               slot h; stops and returns true as soon as f does
//   forward / reverse / global_sum   halo copies of per-row state, folding halo contributions into the owners' rows,
//                               sum over the ranks
//   CLJP's common-C-point test: fetch_strong_halo_rows, make_marks, begin_row, mark, shares (see the views)
// Integer counts and flags are updated from several host threads with relaxed atomics: sums and "set to 0" stores
// commute, so the outcome does not depend on the schedule.

// measure_i = |S^T_i| + element first_id() + i of the random stream
template <class G>
std::vector<double> coarsen_weights(const G &g) {
  const int n = g.n();
  std::vector<int> cnt((size_t)n, 0), cnt_h((size_t)g.nh(), 0);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++)
      g.each((int)i, [&](int64_t, int j, int h) {
        __atomic_fetch_add(h < 0 ? &cnt[(size_t)j] : &cnt_h[(size_t)h], 1, __ATOMIC_RELAXED);
        return false;
      });
  });
  g.reverse(cnt_h, cnt, [](int &mine, int v) { mine += v; });
  std::vector<double> measure((size_t)n);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    if (b >= e) return;
    ParkMiller rng = park_miller_at(2747, g.first_id() + b);  // (a block starts by jump-ahead, then the recurrence)
    for (int64_t i = b; i < e; i++) measure[(size_t)i] = (double)cnt[(size_t)i] + rng.next();
  });
  return measure;
}

// First classification; returns the undecided rows (cf 0).  A row without strong entries is special F -- under CLJP
// only once its weight is below 1 (others may still depend on it); a weight below 1 means F.  init (HMIS / Falgout): the
// verdicts of the per-rank Ruge-Stueben passes.  INTERIOR rows -- no strong connection to another rank -- keep them
// (PMIS: the C points only; CLJP: all, flagged in `kept`); boundary rows are decided by the rounds.
template <class G>
std::vector<int> first_classification(const G &g, const std::vector<double> &measure, const std::vector<int> *init, bool is_cljp,
                                      std::vector<int> &cf, std::vector<char> *kept = nullptr) {
  const int n = g.n();
  cf.assign((size_t)n, 0);
  if (kept && init) kept->assign((size_t)n, 0);
  parallel_for(n, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; i++) {
      bool any = false, boundary = false;
      g.each((int)i, [&](int64_t, int, int h) {
        any = true;
        boundary = boundary || h >= 0;
        return boundary || !init;
      });
      if (init && !boundary && (is_cljp || (any && (*init)[(size_t)i] == C_PT))) {
        cf[(size_t)i] = (*init)[(size_t)i];
        if (kept) (*kept)[(size_t)i] = 1;
      } else if (!any && (!is_cljp || measure[(size_t)i] < 1.0))
        cf[(size_t)i] = SF_PT;
      else if (measure[(size_t)i] < 1.0)
        cf[(size_t)i] = F_PT;
    }
  });
  std::vector<int> graph;
  for (int i = 0; i < n; i++)
    if (cf[(size_t)i] == 0) graph.push_back(i);
  return graph;
}

// One selection round: the undecided points whose measure beats every undecided strong neighbour's (in either
// direction of the edge) become C.  Halo points that lose against one of my rows learn it from the reverse exchange.
template <class G>
void select_round(const G &g, const std::vector<int> &graph, const std::vector<double> &measure, const std::vector<double> &m_h,
                  std::vector<int> &cf, std::vector<int> &cf_h, std::vector<signed char> &tmp) {
  const int64_t ng = (int64_t)graph.size();
  std::vector<int> lose_h((size_t)g.nh(), 1);  // 0: the halo point lost a comparison against one of my rows
  parallel_for(ng, [&](int64_t b, int64_t e, int) {
    for (int64_t q = b; q < e; q++) tmp[(size_t)graph[(size_t)q]] = 1;
  });
  parallel_for(ng, [&](int64_t b, int64_t e, int) {
    for (int64_t q = b; q < e; q++) {
      const int i = graph[(size_t)q];
      const double mi_ = measure[(size_t)i];
      bool lost = false;
      g.each(i, [&](int64_t, int j, int h) {
        if ((h < 0 ? cf[(size_t)j] : cf_h[(size_t)h]) != 0) return false;
        const double mj = h < 0 ? measure[(size_t)j] : m_h[(size_t)h];
        if (mj > mi_)
          lost = true;
        else if (mi_ > mj && h < 0)
          __atomic_store_n(&tmp[(size_t)j], (signed char)0, __ATOMIC_RELAXED);
        else if (mi_ > mj)
          __atomic_store_n(&lose_h[(size_t)h], 0, __ATOMIC_RELAXED);
        return false;
      });
      if (lost) __atomic_store_n(&tmp[(size_t)i], (signed char)0, __ATOMIC_RELAXED);
    }
  });
  if constexpr (G::has_halo) {
    std::vector<int> keep((size_t)g.n(), 1);
    g.reverse(lose_h, keep, [](int &mine, int v) { mine = std::min(mine, v); });
    parallel_for(ng, [&](int64_t b, int64_t e, int) {
      for (int64_t q = b; q < e; q++)
        if (!keep[(size_t)graph[(size_t)q]]) tmp[(size_t)graph[(size_t)q]] = 0;
    });
  }
  parallel_for(ng, [&](int64_t b, int64_t e, int) {
    for (int64_t q = b; q < e; q++)
      if (tmp[(size_t)graph[(size_t)q]] == 1) cf[(size_t)graph[(size_t)q]] = C_PT;
  });
  g.forward(cf, cf_h);
}

// PMIS (par_coarsen.c hypre_BoomerAMGCoarsenPMIS; oracle/oracle.c pmis).  One global random stream indexed by the
// global row id, so the splitting does not depend on the partition.  Leaves cf (C_PT / F_PT / SF_PT) and its halo
// copy cf_h.  init: HMIS, see first_classification -- the kept C points are the first independent set.
template <class G>
void pmis(const G &g, std::vector<int> &cf, std::vector<int> &cf_h, const std::vector<int> *init = nullptr) {
  const std::vector<double> measure = coarsen_weights(g);
  std::vector<double> m_h;
  std::vector<int> graph = first_classification(g, measure, init, false, cf);
  g.forward(measure, m_h);
  g.forward(cf, cf_h);
  std::vector<signed char> tmp((size_t)g.n(), 0);
  // undecided rows that depend on a C point become F once the scan is over (the scan sees the C points only)
  auto f_sweep = [&] {
    parallel_for((int64_t)graph.size(), [&](int64_t b, int64_t e, int) {
      for (int64_t q = b; q < e; q++) {
        const int i = graph[(size_t)q];
        if (cf[(size_t)i] != 0) continue;
        const bool dep_c = g.each(i, [&](int64_t, int j, int h) { return (h < 0 ? cf[(size_t)j] : cf_h[(size_t)h]) == C_PT; });
        tmp[(size_t)i] = dep_c ? 2 : 3;
      }
    });
    std::vector<int> next;
    next.reserve(graph.size());
    for (int i : graph) {
      if (cf[(size_t)i] != 0) continue;
      if (tmp[(size_t)i] == 2)
        cf[(size_t)i] = F_PT;
      else
        next.push_back(i);
    }
    graph.swap(next);
    g.forward(cf, cf_h);
  };
  if (init) f_sweep();
  while (g.global_sum((long long)graph.size()) != 0) {
    select_round(g, graph, measure, m_h, cf, cf_h, tmp);
    f_sweep();
  }
}

// CLJP (par_coarsen.c hypre_BoomerAMGCoarsen; oracle/oracle.c cljp, cljp_from): w = |S^T_i| + the global random
// stream; rounds of { independent set of the undecided points -> C; H1: edges out of a new C point leave, w-- at their
// undecided ends; H2: an undecided row loses its edges to C points, and the edges to undecided points that share one
// of its C points, w-- there; w < 1 -> F }.  Within a round every step reads what the previous one left and the
// decrements are integers, so the round is the sequential one whatever the threads or the partition: decrements of
// halo points travel back to their owners, the weights and states of the halo points forward.
// init (Falgout): interior rows keep the verdict of the per-rank Ruge-Stueben passes and stop voting (their edges leave
// before the first selection), boundary rows are decided here, H2 runs once with the kept C points (oracle cljp_from).
template <class G>
void cljp(G &g, std::vector<int> &cf, std::vector<int> &cf_h, const std::vector<int> *init = nullptr) {
  const int n = g.n();
  g.fetch_strong_halo_rows();
  std::vector<double> measure = coarsen_weights(g), m_h;
  std::vector<char> gone((size_t)g.nnz(), 0), kept;
  std::vector<int> dec((size_t)n, 0), dec_h((size_t)g.nh(), 0);  // pending decrements of a round
  std::vector<int> graph = first_classification(g, measure, init, true, cf, &kept);
  g.forward(cf, cf_h);
  g.forward(measure, m_h);
  auto state = [&](int j, int h) { return h < 0 ? cf[(size_t)j] : cf_h[(size_t)h]; };
  auto dec_end = [&](int j, int h) {  // one decrement at the undecided end of an entry
    if (state(j, h) == 0) __atomic_fetch_add(h < 0 ? &dec[(size_t)j] : &dec_h[(size_t)h], 1, __ATOMIC_RELAXED);
  };
  if (init)  // decided points no longer vote (an interior row has no halo ends)
    parallel_for(n, [&](int64_t b, int64_t e, int) {
      for (int64_t i = b; i < e; i++)
        if (kept[(size_t)i])
          g.each((int)i, [&](int64_t k, int j, int h) {
            gone[(size_t)k] = 1;
            dec_end(j, h);
            return false;
          });
    });
  std::vector<signed char> tmp((size_t)n, 0);
  auto marks = g.make_marks();  // one per host thread
  for (int round = init ? 0 : 1;; round++) {
    if (round > 0) {
      if (g.global_sum((long long)graph.size()) == 0) break;
      select_round(g, graph, measure, m_h, cf, cf_h, tmp);
    }
    // H1 (rows of this round's C points) and H2 (undecided rows): disjoint rows, decrements collected in dec / dec_h
    parallel_for((int64_t)graph.size(), [&](int64_t b, int64_t e, int t) {
      auto &mk = marks[(size_t)t];
      for (int64_t q = b; q < e; q++) {
        const int i = graph[(size_t)q];
        if (cf[(size_t)i] == C_PT) {
          g.each(i, [&](int64_t k, int j, int h) {
            if (!gone[(size_t)k]) {
              gone[(size_t)k] = 1;
              dec_end(j, h);
            }
            return false;
          });
          continue;
        }
        g.begin_row(mk, i);
        int nc_row = 0;
        g.each(i, [&](int64_t k, int j, int h) {
          if (state(j, h) == C_PT) {
            gone[(size_t)k] = 1;
            g.mark(mk, i, k, j);
            nc_row++;
          }
          return false;
        });
        if (!nc_row) continue;
        g.each(i, [&](int64_t k, int j, int h) {
          if (!gone[(size_t)k] && state(j, h) == 0 && g.shares(mk, i, j, h)) {
            gone[(size_t)k] = 1;
            dec_end(j, h);
          }
          return false;
        });
      }
    });
    g.reverse(dec_h, dec, [](int &mine, int v) { mine += v; });
    std::fill(dec_h.begin(), dec_h.end(), 0);
    std::vector<int> next;
    next.reserve(graph.size());
    for (int i : graph) {
      if (cf[(size_t)i] == C_PT) continue;
      for (; dec[(size_t)i] > 0; dec[(size_t)i]--) measure[(size_t)i] -= 1.0;  // one at a time, as the oracle does
      if (measure[(size_t)i] < 1.0)
        cf[(size_t)i] = F_PT;
      else
        next.push_back(i);
    }
    graph.swap(next);
    g.forward(cf, cf_h);
    g.forward(measure, m_h);
  }
}

// locality numbering of a block's rows (amg_setup.cpp): order[new] = old; excluded rows (optional) come last
void locality_order(const HostCSR &D, std::vector<int> &order, const std::vector<char> *exclude);
// its pieces, shared with the device path: the seeds (ascending), and the stable sort of the final labels
// (seed rank; nseeds = never reached; LOCALITY_EXCLUDED)
constexpr int LOCALITY_EXCLUDED = -2;
constexpr int LOCALITY_MAX_ROUNDS = 64;
int locality_segment_shift(const HostCSR &D);
std::vector<int> locality_seeds(int n, int segshift, const std::vector<char> *exclude);
void locality_sort(std::vector<int> &label, int nseeds, std::vector<int> &order);  // label: seed ranks, -1, EXCLUDED (overwritten)

}  // namespace hs
}  // namespace mi
